"""Writes tests/golden/boundary_cases.npz from the boundary oracle (tests/boundary_oracle.py): six single tets of both
orientations, each with its four faces as boundary facets, a random state (mixed signs of u.n over the quadrature points),
random tractions and backflow coefficients, and the raw boundary residual and Jacobian of the flow terms; and for the same
tets random Robin data with the facet operator and right-hand side of the scalars.  tests/test_host_boundary.py regenerates every
array from here; tests/test_gpu_boundary.py runs each case through the library.

    python scripts/make_boundary_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "boundary_cases.npz")
N_EL = 6
FACES = np.array([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]], dtype=np.int32)     # the four faces, windings mixed on purpose
FACES[2] = FACES[2][[0, 2, 1]]


def random_tets(rng, n):
    """(n, 4, 3): the unit tet scaled, with jittered vertices; every second one with two vertices swapped (negative det J)."""
    ref = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    X = 0.3 * (ref[None] + 0.15 * rng.uniform(-1.0, 1.0, (n, 4, 3))) + rng.uniform(-1.0, 1.0, (n, 1, 3))
    X[1::2] = X[1::2][:, [0, 2, 1, 3]]
    return X


def build():
    import boundary_oracle as BO
    rng = np.random.default_rng(91)
    X = random_tets(rng, N_EL)
    W = rng.standard_normal((N_EL, 16))
    t = rng.standard_normal((N_EL, 4, 3, 3))
    beta = rng.uniform(0.5, 2.0, (N_EL, 4))
    beta[:, 3] = 0.0                                                      # one face with the backflow term off
    alpha = rng.uniform(0.0, 3.0, (N_EL, 4, 4))
    g = rng.standard_normal((N_EL, 4, 3, 4))
    tet = np.arange(4, dtype=np.int32)[None]
    own = np.zeros(4, np.int64)
    F, J = np.zeros((N_EL, 16)), np.zeros((N_EL, 16, 16))
    SA, Sb = np.zeros((N_EL, 16, 16)), np.zeros((N_EL, 16))
    for i in range(N_EL):
        f, j = BO.flow_raw(X[i], tet, W[i], FACES, own, t[i], beta[i])
        F[i], J[i] = f, j.toarray()
        a, b = BO.scalar_raw(X[i], tet, FACES, own, alpha[i], g[i])
        SA[i], Sb[i] = a.toarray(), b
    return dict(X=X, W=W, faces=FACES, t=t, beta=beta, F=F, J=J, alpha=alpha, g=g, scalar_A=SA, scalar_b=Sb)


if __name__ == "__main__":
    np.savez_compressed(FIXTURE, **build())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
