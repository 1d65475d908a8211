"""Set-up cost of the fine-level aggregation by operator strength, host matcher (amg_aggregation = 1) against the device build (2),
with the default geometric aggregation (0) as the floor, on the structured duct (300 x 75 x 75 cells = 10.1 M tets by default).

Per value: the first sns_pc_setup after the Stokes assembly (hierarchy build included, host clock) and the first Stokes solve of a
fresh handle (assembly + set-up + solve).  For 1 the host matcher alone is timed again on the exported strength
(sns_host_aggregate_strength: what the hierarchy build runs), and the maps of 1 and 2 are compared.  Run the device build's kernels
under `rocprofv3 --kernel-trace --stats -- python scripts/profile_device_aggregation.py --values 2` for the kernel times
(k_agg_*, k_scan_*, k_strength*).  Output: profiles/device_strength_aggregation.txt."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stabilized_navier_stokes_flow_fenicsx_amd import _lib, bcs as B, mesh as M  # noqa: E402
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--values", type=int, nargs="+", default=[0, 1, 2])
    a = ap.parse_args()
    t0 = time.perf_counter()
    m = M.duct_mesh(tuple(a.cells), 4.0)
    bcs = B.duct_bcs(m)
    print(f"duct {a.cells}: {m.num_tets} tets, {m.num_nodes} nodes (mesh {time.perf_counter() - t0:.1f} s)", flush=True)
    maps = {}
    for v in a.values:
        P = FlowProblem(m, bcs, reynolds=50.0, amg_aggregation=v)
        P.jacobian(None, "stokes")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P.pc_setup()
        torch.cuda.synchronize()
        t_setup = time.perf_counter() - t0
        line = f"amg_aggregation={v}: first pc_setup {1e3 * t_setup:8.1f} ms"
        if v >= 1:
            maps[v] = P.export(_lib.EXPORT_AGG0, torch.int32, m.num_nodes).cpu().numpy()
            line += f"  aggregates {int(maps[v].max()) + 1}"
        if v == 1:
            s = P.export(_lib.EXPORT_STRENGTH, torch.float32, P.sizes()["nnzb"]).cpu().numpy()
            rp, ci, _ = (t.cpu().numpy() for t in P.bsr())
            t0 = time.perf_counter()
            _lib.host_aggregate_strength(rp, ci, s)
            line += f"  host matcher alone {1e3 * (time.perf_counter() - t0):8.1f} ms"
            del s, rp, ci
        P.close()
        P = FlowProblem(m, bcs, reynolds=50.0, amg_aggregation=v)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, r = P.stokes_solve()
        torch.cuda.synchronize()
        line += f"  first stokes_solve {1e3 * (time.perf_counter() - t0):8.1f} ms ({r.its} its, reason {r.reason})"
        P.close()
        print(line, flush=True)
    if 1 in maps and 2 in maps:
        print(f"maps of 1 and 2 identical: {bool((maps[1] == maps[2]).all())}", flush=True)


if __name__ == "__main__":
    main()
