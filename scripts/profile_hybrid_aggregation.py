"""amg_aggregation = 0 / 2 / 3 (the hybrid) through FlowProblem, two-stream channel: per mesh and value the marked fraction of
the hybrid (numpy restatement of tests/test_host_hybrid_aggregation.py on the handle's strength and the value-0 map), the Stokes
BiCGStab count, BiCGStab iterations and ms per Newton step, and the first pc_setup after the Stokes assembly (hierarchy build
included, host clock).  Meshes: the five of profiles/mesh_quality_aggregation.txt, the half-jittered channel of the tests, config
4u (Delaunay channel h = 1/47) and config 4b (body-fitted nozzle channel, lc 0.02) at Re 50; then the first pc_setup of the
10 M-tet duct with 3 against 0.  Output: profiles/hybrid_aggregation.txt.

    python scripts/profile_hybrid_aggregation.py [--only NAME ...] [--no-duct]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from stabilized_navier_stokes_flow_fenicsx_amd import _lib, bcs as B, mesh as M  # noqa: E402
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem  # noqa: E402
from test_host_hybrid_aggregation import half_jittered_channel, hybrid_map  # noqa: E402


def channel(m):
    return m, B.channel_bcs(m, *B.two_stream_profiles(0.5))


def meshes():
    yield "structured 140x35x35", lambda: channel(M.channel_mesh((140, 35, 35)))
    yield "delaunay bcc h=1/28 seed 0", lambda: channel(M.delaunay_channel_mesh(28, seed=0))
    yield "delaunay cubic h=1/35 seed 0", lambda: channel(M.delaunay_channel_mesh(35, lattice="cubic", seed=0))
    yield "delaunay bcc h=1/28 seed 1", lambda: channel(M.delaunay_channel_mesh(28, seed=1))
    yield "delaunay cubic h=1/35 seed 1", lambda: channel(M.delaunay_channel_mesh(35, lattice="cubic", seed=1))
    yield "half-jittered 48x12x12", lambda: channel(half_jittered_channel()[0])
    yield "config 4u (bcc h=1/47)", lambda: channel(M.delaunay_channel_mesh(47, lattice="bcc"))

    def cfg4b():
        from stabilized_navier_stokes_flow_fenicsx_amd import nozzle_mesh as NM
        m, bcs, _ = NM.channel_from_image_bodyfitted(os.path.join(ROOT, "tests", "golden", "inlet_PlusF_final.png"), 0.5, 0.02)
        return m, bcs
    yield "config 4b (nozzle lc 0.02)", cfg4b


def first_setup(m, bcs, v):
    P = FlowProblem(m, bcs, reynolds=50.0, amg_aggregation=v)
    P.jacobian(None, "stokes")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P.pc_setup()
    torch.cuda.synchronize()
    return P, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--no-duct", action="store_true")
    a = ap.parse_args()
    for name, make in meshes():
        if a.only and not any(o in name for o in a.only):
            continue
        m, bcs = make()
        cols, frac = [], None
        for v in (0, 2, 3):
            P, t_setup = first_setup(m, bcs, v)
            if v == 0:
                g = P.export(_lib.EXPORT_AGG0, torch.int32, m.num_nodes).cpu().numpy()
            if v == 3:
                s = P.export(_lib.EXPORT_STRENGTH, torch.float32, P.sizes()["nnzb"]).cpu().numpy()
                rp, ci, _ = (t.cpu().numpy() for t in P.bsr())
                _, _, marked, F = hybrid_map(rp, ci, s, g, m.num_nodes)
                frac = (marked.mean(), F.mean())
            P.close()
            P = FlowProblem(m, bcs, reynolds=50.0, amg_aggregation=v)
            U, r = P.stokes_solve()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w, n = P.newton_solve(U.clone())
            torch.cuda.synchronize()
            t_newton = time.perf_counter() - t0
            P.close()
            steps = max(1, n.its)
            cols.append(f"{v}: {r.its:4d} / {n.ksp_its / steps:6.1f} its, {1e3 * t_newton / steps:7.1f} ms/step, setup {1e3 * t_setup:7.1f} ms"
                        f" (newton {n.its} reason {n.reason})")
        print(f"{name:30s} {m.num_tets:8d} tets  marked {frac[0]:.4f} dissolved {frac[1]:.3f} | " + " | ".join(cols), flush=True)
    if not a.no_duct:
        m = M.duct_mesh((300, 75, 75), 4.0)
        bcs = B.duct_bcs(m)
        out = []
        for v in (0, 3, 0, 3):
            P, t = first_setup(m, bcs, v)
            out.append(f"{v}: {1e3 * t:.1f} ms")
            P.close()
        print(f"10M duct {m.num_tets} tets: first pc_setup " + ", ".join(out), flush=True)


if __name__ == "__main__":
    main()
