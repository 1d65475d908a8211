"""Writes tests/golden/scalar_cases.npz from the scalar-transport oracle (tests/scalar_oracle.py): element records of eight
jittered tets of both orientations (matrix and source vector of one species each, over a range of kappa, sigma, theta), and one
global four-species case on the 2 x 1 x 1 box (operator, right-hand side and LU solution).  tests/test_host_scalar.py
regenerates every array from here.

    python scripts/make_scalar_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "scalar_cases.npz")
N_EL = 8


def random_tets(rng, n):
    """(n, 4, 3): the unit tet scaled, with jittered vertices; every second one with two vertices swapped (negative det J)."""
    ref = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    X = 0.3 * (ref[None] + 0.15 * rng.uniform(-1.0, 1.0, (n, 4, 3))) + rng.uniform(-1.0, 1.0, (n, 1, 3))
    X[1::2] = X[1::2][:, [0, 2, 1, 3]]
    return X


def box_case():
    """The 2 x 1 x 1 box (12 nodes, 12 tets) with a random state, four diffusivities, random Dirichlet data and a source."""
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    m = M.duct_mesh((2, 1, 1), 2.0)
    rng = np.random.default_rng(72)
    n = m.num_nodes
    cmask = (rng.random((n, 4)) < 0.3).astype(np.uint8)
    cmask[0] = 1                                                        # every species has a Dirichlet node
    return dict(points=m.points, tets=m.tets, w=rng.standard_normal(4 * n), kappa=np.array([1.0, 0.1, 1e-2, 1e-4]),
                cmask=cmask, cval=rng.standard_normal((n, 4)), sigma=0.7, theta=5.0, source=rng.standard_normal((n, 4)))


def build():
    import scalar_oracle as SO
    rng = np.random.default_rng(71)
    X = random_tets(rng, N_EL)
    U = rng.standard_normal((N_EL, 4, 3))
    src = rng.standard_normal((N_EL, 4))
    kappa = 10.0 ** rng.uniform(-4.0, 0.0, N_EL)
    sigma = np.where(np.arange(N_EL) % 3 == 0, 0.0, rng.uniform(0.0, 5.0, N_EL))
    theta = np.where(np.arange(N_EL) % 3 == 0, 0.0, rng.uniform(0.0, 50.0, N_EL))
    A, S = np.zeros((N_EL, 4, 4)), np.zeros((N_EL, 4))
    for i in range(N_EL):
        a, s = SO.element(X[i][None], U[i][None], kappa[i], sigma[i], theta[i], src[i][None])
        A[i], S[i] = a[0], s[0]
    out = dict(el_X=X, el_U=U, el_src=src, el_kappa=kappa, el_sigma=sigma, el_theta=theta, el_A=A, el_S=S)
    c = box_case()
    Ab, b, _ = SO.assemble(c["points"], c["tets"], c["w"], c["kappa"], c["cmask"], c["cval"], c["sigma"], c["theta"], c["source"])
    sol = SO.solve(c["points"], c["tets"], c["w"], c["kappa"], c["cmask"], c["cval"], c["sigma"], c["theta"], c["source"])
    out.update({f"box_{k}": np.asarray(v) for k, v in c.items()})
    out.update(box_A=Ab.toarray(), box_b=b, box_c=sol)
    return out


if __name__ == "__main__":
    np.savez_compressed(FIXTURE, **build())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
