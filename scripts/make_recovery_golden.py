"""Writes tests/golden/recovery_cases.npz: for a Delaunay duct and a jittered triangle mesh a random state w and the oracle's
recovered gradient G, derived fields D and Zienkiewicz-Zhu indicator eta2 (tests/recovery_oracle.py).  The meshes come from the
package's seeded meshers (``meshes()``, which the GPU tests call too); the triangle mesh's arrays are stored as well.
tests/test_host_recovery.py regenerates every array from here.

    python scripts/make_recovery_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "recovery_cases.npz")


def meshes():
    """name -> (points (n, d), cells (E, d+1)): delaunay_duct_mesh(n=6), and rectangle_mesh(7, 5) with its interior nodes moved
    by up to 0.2 of a cell."""
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
    d = M.delaunay_duct_mesh(n=6)
    r = M2.rectangle_mesh(7, 5)
    p = r.points.copy()
    inner = np.setdiff1d(np.arange(len(p)), np.unique(r.facets))
    p[inner] += 0.2 * np.array([1.0 / 7, 1.0 / 5]) * np.random.default_rng(31).uniform(-1.0, 1.0, (len(inner), 2))
    return {"duct": (d.points, d.tets), "tri": (p, r.tris)}


def build():
    import recovery_oracle as RO
    out = {}
    for k, (name, (pts, cells)) in enumerate(meshes().items()):
        w = np.random.default_rng(32 + k).standard_normal(4 * len(pts))
        G = RO.recover(pts, cells, w)
        out.update({f"{name}_w": w, f"{name}_G": G, f"{name}_D": RO.derived(G), f"{name}_eta2": RO.indicator(pts, cells, w, G)[0]})
        if name == "tri":
            out.update(tri_points=np.asarray(pts, dtype=np.float64), tri_cells=np.asarray(cells, dtype=np.int32))
    return out


if __name__ == "__main__":
    np.savez_compressed(FIXTURE, **build())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
