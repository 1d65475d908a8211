"""Implicit time stepping (sns_set_time_term / sns_time_step, solver.solve_unsteady): the numbers behind DESIGN.md's section
on the transient form.

  A  assembly cost on the 10 M-tet duct of bench.py (300 x 75 x 75 cells, Re 200, state = the Stokes solution):
     sns_bench_assemble (Jacobian + residual, HIP events around `reps` back-to-back assemblies after one warm-up call),
     steady against transient, fused and staged path, alternated three times in one process; median and spread
  B  DFG 2D-2 (Re 100) on the one-cell slab, BDF2, theta = 4/dt^2 against theta = 0: max C_d, max C_l, St, Newton and Krylov
     iterations per step, and the node-to-node pressure oscillation max |p_top - p_bottom| / max |p| of the last state

    python scripts/profile_transient.py [--out FILE] [--sections AB] [--level 2] [--dt 0.01] [--steps 600]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, drivers as D, mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transient_stepping.txt"))
    ap.add_argument("--sections", default="AB")
    ap.add_argument("--cells", default="300,75,75")
    ap.add_argument("--level", type=float, default=2)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    fh = open(args.out, "a" if args.append else "w")

    def emit(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    if "A" in args.sections:
        cells = tuple(int(c) for c in args.cells.split(","))
        m = M.duct_mesh(cells, 4.0)
        P = FlowProblem(m, B.duct_bcs(m), reynolds=200.0)
        U, rs = P.stokes_solve()
        d = U * (-1.5 / 0.01)
        emit(f"A  assembly, {m.num_tets} tets, sns_bench_assemble (J + F), reps 5 after one warm-up; ms per assembly")
        for fused in (1, 0):
            P.set_options(assembly_fused=fused)
            t = {"steady": [], "transient": []}
            for rep in range(3):
                P.clear_time_term()
                t["steady"].append(P.bench_assemble(U, reps=5))
                P.set_time_term(1.5 / 0.01, 4.0 / 0.01 ** 2, d)
                t["transient"].append(P.bench_assemble(U, reps=5))
            P.clear_time_term()
            s, tr = np.array(t["steady"]), np.array(t["transient"])
            emit(f"   {'fused ' if fused else 'staged'}  steady {np.median(s):8.3f} ({s.min():.3f} .. {s.max():.3f})   transient "
                 f"{np.median(tr):8.3f} ({tr.min():.3f} .. {tr.max():.3f})   ratio of medians {np.median(tr) / np.median(s):.3f}")
        P.close()
        del P, U, d
        torch.cuda.empty_cache()

    if "B" in args.sections:
        emit(f"B  DFG 2D-2 on the slab, level {args.level}, BDF2, dt {args.dt}, {args.steps} steps "
             "(Schaefer-Turek: max C_d 3.22-3.24, max C_l 0.99-1.01, St 0.295-0.305; not expected to be met by P1-P1 here)")
        for tc in (4.0, 0.0):
            r = D.run_dfg2d2_slab(args.level, args.dt, args.steps, theta_coeff=tc, verbose=False)
            its = np.array([q["its"] for q in r["records"]], dtype=np.float64)
            kits = np.array([q["ksp_its"] for q in r["records"]], dtype=np.float64)
            p = r["w"].view(-1, 4)[:, 3].cpu().numpy()
            half = len(p) // 2                            # extrude_tri_mesh: bottom plane's nodes first, the top plane's in the same order
            xy = r["points"][:, :2]
            assert np.array_equal(xy[:half], xy[half:]) and np.all(r["points"][half:, 2] > r["points"][:half, 2])
            osc = np.abs(p[half:] - p[:half]).max() / max(np.abs(p).max(), 1e-300)
            sign_changes = int((np.diff(np.sign(r["cl"][len(r["cl"]) // 2:])) != 0).sum()) if len(r["cl"]) else 0
            emit(f"   theta = {tc:g}/dt^2: {r['n_tets']} tets, {len(r['t'])} of {args.steps} steps converged, {r['seconds']:.1f} s; max C_d "
                 f"{r['cd_max']:.4f}  max C_l {r['cl_max']:.4f}  St {r['strouhal']:.4f} ({r['crossings']} upward crossings, "
                 f"{sign_changes} sign changes of C_l in the second half)")
            emit(f"      Newton its / step mean {its.mean():.2f} max {its.max():.0f}; Krylov its / step mean {kits.mean():.1f} max "
                 f"{kits.max():.0f}; last reason {r['records'][-1]['reason']}; |p_top - p_bottom|max / |p|max {osc:.3e}")
    fh.close()


if __name__ == "__main__":
    main()
