"""What the symbolic hierarchy build leaves behind, as text that two builds of libsns.so can be diffed on.

    python scripts/hierarchy_build_report.py --lib PATH/libsns.so STEP

STEP: serial | team-duct | team-cavity | team-window | setup-time.  Every handle prints, per rank: hierarchy() rows and blocks,
cycle(), sha256 of SNS_EXPORT_AGG0, every level's damping as a hex float, the Stokes and Newton iteration counts and reasons; and
once per case sns_live_device_bytes after the first set-up (team cases: read by rank 0 between two barriers, all ranks' handles
together).  setup-time prints host wall times (sns_create to the end of the first pc_setup on the benchmark's mesh, five fresh
handles) and is not meant to be diffed.  scripts/hierarchy_build_compare.sh runs the steps on two libraries and diffs."""
import argparse
import hashlib
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REP = dict(amg_coarse_size=24, amg_replicate_rows=1 << 20, amg_dense_rows=0)
REP_DENSE = dict(amg_replicate_rows=1 << 20)


def _describe(P, n_local):
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    hier, cyc = P.hierarchy(), P.cycle()
    agg = P.export(_lib.EXPORT_AGG0, torch.int32, n_local).cpu().numpy()
    return (f"rows {[h['rows'] for h in hier]} blocks {[h['blocks'] for h in hier]} "
            f"cycle {[(c['kind'], c['pre'], c['post']) for c in cyc]} agg0 {hashlib.sha256(agg.tobytes()).hexdigest()[:16]}")


def _omegas(P):
    return " ".join(float(h["omega"]).hex() for h in P.hierarchy())


def _walk(P, n_local, live=None):
    """First set-up (Stokes operator), Stokes solve, Newton solve: the lines of one handle."""
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    P.jacobian(None, "stokes")
    P.pc_setup()
    lines = ["  " + _describe(P, n_local), "  first set-up omega " + _omegas(P)]
    if live is not None:
        lines.append(f"  live device bytes after the first set-up {live()}")
    U, r = P.stokes_solve()
    lines.append(f"  stokes its {r.its} reason {r.reason} omega {_omegas(P)}")
    w, n = P.newton_solve(U.clone())
    lines.append(f"  newton its {n.its} ksp {n.ksp_its} reason {n.reason} omega {_omegas(P)}")
    return lines


def serial():
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, bcs as B, mesh as M, mesh2d as M2
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    lib = _lib.load()
    small = dict(amg_dense_rows=0, amg_coarse_size=8)
    m1, m2 = M.duct_mesh((6, 3, 3), 4.0, jitter=0.2), M.duct_mesh((16, 8, 8), 4.0, jitter=0.2)
    cases = [("duct (6, 3, 3) small coarsest", m1, B.duct_bcs(m1).flatten(), dict(small)),
             ("duct (16, 8, 8) small coarsest", m2, B.duct_bcs(m2).flatten(), dict(small))]
    cases += [(f"duct (16, 8, 8) amg_aggregation {a}", m2, B.duct_bcs(m2).flatten(), dict(amg_aggregation=a)) for a in range(4)]
    m2d = M2.rectangle_mesh(24)
    cases.append(("2-D cavity 24 x 24", m2d, M2.cavity2d_bcs(m2d).flatten(), dict(small)))
    for name, m, bcs, kw in cases:
        base = lib.sns_live_device_bytes()
        re = 20.0 if getattr(m, "dim", 3) == 2 else 50.0
        P = FlowProblem(m, bcs, reynolds=re, **kw)
        print(f"serial {name}")
        print("\n".join(_walk(P, len(m.points), live=lambda: lib.sns_live_device_bytes() - base)), flush=True)
        P.close()


def _team_case(name, nranks, make, kw):
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import Team
    lib = _lib.load()
    base = lib.sns_live_device_bytes()
    team = Team(nranks)
    gate = threading.Barrier(nranks)
    live = [None]

    def work(rank, team):
        P = make(rank, team, kw)

        def read_live():                       # every rank's first set-up is done; nobody allocates until rank 0 has read
            gate.wait(timeout=120)
            if rank == 0:
                live[0] = lib.sns_live_device_bytes() - base
            gate.wait(timeout=120)
            return live[0]

        lines = _walk(P, P.n_local, live=read_live)
        P.close()
        return lines

    outs = team.run(work)
    team.close()
    print(f"team {name} {nranks} ranks {kw}")
    for rank, lines in enumerate(outs):
        print(f" rank {rank}")
        print("\n".join(lines))
    sys.stdout.flush()


def team_duct():
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M, partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh((24, 6, 6), 4.0, jitter=0.1)
    mask, g = B.duct_bcs(m).flatten()
    for nranks in (2, 3, 4):
        owner = PT.rcb_partition(m.points, nranks)

        def make(rank, team, kw):
            part = PT.build_local_part(m, mask, g, owner, rank, nranks)
            return FlowProblem(part.mesh, (part.bc_mask, part.bc_val), reynolds=12.0, part=part, group=team, **kw)

        for tag, kw in (("plain", {}), ("-rep", REP), ("-rep-dense", REP_DENSE)):
            _team_case(f"duct (24, 6, 6) {tag}", nranks, make, kw)


def team_cavity():
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M, partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.cavity_mesh(12, jitter=0.1)
    mask, g = B.cavity_bcs(m).flatten()
    for nranks in (2, 3, 4):
        owner = PT.rcb_partition(m.points, nranks)

        def make(rank, team, kw):
            part = PT.build_local_part(m, mask, g, owner, rank, nranks)
            return FlowProblem(part.mesh, (part.bc_mask, part.bc_val), reynolds=12.0, part=part, group=team, **kw)

        for tag, kw in (("plain", {}), ("-rep", REP), ("-rep-dense", REP_DENSE)):
            _team_case(f"cavity 12^3 RCB {tag}", nranks, make, kw)


def team_window():
    """The window cycle of tests/test_gpu_parity.py::test_window_cycle_with_exact_coarse_sweeps: a partitioned level 1 with M = A P."""
    from stabilized_navier_stokes_flow_fenicsx_amd import partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    cells = (96, 24, 24)
    for nranks in (2, 4):
        def make(rank, team, kw):
            return FlowProblem.from_part(PT.duct_slab_part(cells, 4.0, rank, nranks), group=team, reynolds=40.0, **kw)

        for exact in (1, 0):
            _team_case("duct (96, 24, 24) slabs, windows", nranks, make, dict(amg_replicate_rows=2000, halo_windows=1, amg_exact_sweeps=exact))


def setup_time():
    """Host wall time of the one-off symbolic build on the benchmark's mesh: sns_create to the end of the first pc_setup."""
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh((300, 75, 75), 4.0)
    bcs = B.duct_bcs(m).flatten()
    total, build = [], []
    for k in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = FlowProblem(m, bcs, reynolds=200.0, ksp_type="bicgstab", pc_type="amg", snes_max_it=1)
        t1 = time.perf_counter()
        P.jacobian(None, "stokes")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        P.pc_setup()                           # the hierarchy is built here (lazily), then the first numeric set-up
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        rows = [h["rows"] for h in P.hierarchy()]
        P.close()
        total.append(t3 - t0)
        build.append(t3 - t2)
        print(f"handle {k}: create {t1 - t0:.3f} s, assemble {t2 - t1:.3f} s, first pc_setup with the build {t3 - t2:.3f} s, "
              f"create to end of first pc_setup {t3 - t0:.3f} s, rows {rows}", flush=True)
    for name, v in (("create to end of first pc_setup", total), ("first pc_setup with the build", build)):
        print(f"{name}: min {min(v):.3f} median {float(np.median(v)):.3f} max {max(v):.3f} s")


STEPS = {"serial": serial, "team-duct": team_duct, "team-cavity": team_cavity, "team-window": team_window, "setup-time": setup_time}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the libsns.so to load")
    ap.add_argument("step", choices=sorted(STEPS))
    args = ap.parse_args()
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    _lib.LIB_PATH = os.path.abspath(args.lib)              # (before the first load)
    STEPS[args.step]()
