"""Writes tests/golden/shape_cases.npz: a few disconnected random cells with a random state and a random dof vector lam,
and the oracle's per-cell shape gradients d(lam_e . F_e)/dX_e (tests/shape_oracle.py: autograd through the CPU forms) for
every reading of the form the GPU kernel has.  tests/test_host_shape.py regenerates every array from here.

    python scripts/make_shape_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "shape_cases.npz")
N_CELLS, RE, NU2D = 12, 7.0, 0.05
SIGMA, THETA = 3.0, 11.0
VARIANT = dict(ci=20.0, lsic=0.7, pspg=-1.0, one_point=True)


def build():
    import shape_oracle as SO
    from oracle import forms_literal as FL
    out = {}
    pts, tets, w, lam = SO.random_cells(N_CELLS, 3, seed=11)
    d = np.random.default_rng(12).standard_normal(4 * len(pts))
    out.update(pts3=pts, tets=tets, w3=w, lam3=lam, d3=d, Re=np.float64(RE), sigma=np.float64(SIGMA), theta=np.float64(THETA))
    X, W, L, D = SO._cells3(pts, tets, w, lam, d)
    for c in (False, True):
        out[f"g3_steady_c{int(c)}"] = SO.tet_cell_gradients(X, W, L, 0.0 * D, RE, corrected_convection=c)
        out[f"g3_transient_c{int(c)}"] = SO.tet_cell_gradients(X, W, L, D, RE, SIGMA, THETA, corrected_convection=c)
    old = dict(FL.VARIANT)
    FL.VARIANT.update(VARIANT)
    try:
        out["g3_variant_c0"] = SO.tet_cell_gradients(X, W, L, 0.0 * D, RE)
    finally:
        FL.VARIANT.update(old)
    out["variant"] = np.array([VARIANT["ci"], VARIANT["lsic"], VARIANT["pspg"], float(VARIANT["one_point"])])
    pts2, tris, w2, lam2 = SO.random_cells(N_CELLS, 2, seed=13)
    p3 = np.zeros((len(pts2), 3))
    p3[:, :2] = pts2
    X2, W2, L2 = SO._cells2(p3, tris, w2, lam2)
    out.update(pts2=pts2, tris=tris, w2=w2, lam2=lam2, nu2=np.float64(NU2D), g2=SO.tri_cell_gradients(X2, W2, L2, NU2D))
    return out


if __name__ == "__main__":
    np.savez_compressed(FIXTURE, **build())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
