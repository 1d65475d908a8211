"""Residual-based boundary forces (sns_residual_moments) against the boundary integral of the traction, from the same solutions.

  A  DFG 2D-1 on the 2-D UGN path, levels 2 / 4 / 8 / 16 (mesh2d.drag_lift_2d vs mesh2d.drag_lift_2d_reaction)
  B  DFG 2D-1 on the 3-D tet path (one-cell slab, mesh2d.dfg2d_slab_problem), levels 4 / 8 / 16, the form as written
     (corrected_convection = 0) and the consistent convection (= 1)
  C  DFG 3D-1Z pillar (mesh.dfg_pillar_mesh, body-centred), W/24, W/32, W/40, both forms; residual-based force with the rim nodes
     (obstacle nodes that also lie on the no-slip walls z = 0, H) at weight 1 and at weight 1/2
  D  the perturbation table of test_what_the_reference_constants_tell_apart (level-4 slab) with both functionals
  E  cost on the 10 M-tet duct of bench.py (300 x 75 x 75 cells): phi = outlet-plane indicator, phi = 1, one sns_residual;
     HIP events around the call (which itself synchronises twice), median of 7 after a warm-up

    python scripts/profile_reaction.py [--out profiles/reaction.txt] [--sections ABCDE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU = 1e-3


def main():
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, functionals as Fn, mesh as M, mesh2d as M2
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reaction.txt"))
    ap.add_argument("--sections", default="ABCDE")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    fh = open(args.out, "w")
    cdr, clr = M2.DFG2D_CD_REF, M2.DFG2D_CL_REF

    def emit(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    def pct(c, r):
        return f"{100 * (c / r - 1):+.4f} %"

    emit("Residual-based (variationally consistent) boundary force F = -R_raw(w)(phi e_c) vs the boundary integral of the")
    emit("traction, both from the same discrete solution.  Reference constants: C_d 5.57953523384, C_l 0.010618948146")
    emit("(DFG_2D_Validation.py:202-203).  Produced by scripts/profile_reaction.py.")

    def slab_solve(n, corrected=0, ksp_max_it=10000, **variant):
        m3, (mask, g), thick = M2.dfg2d_slab_problem(n)
        P = FlowProblem(m3, (mask, g), reynolds=1.0 / NU, corrected_convection=corrected, snes_atol=1e-15, snes_rtol=1e-11,
                        snes_stol=1e-12, ksp_rtol=1e-10, ksp_max_it=ksp_max_it)
        if variant:
            P.set_form_variant(**variant)
        U, rs = P.stokes_solve()
        U.view(-1, 4)[:, 3] *= NU
        w, rn = P.newton_solve(U.clone())
        ob = m3.meta["tags"]["obstacle"]
        if rn.reason > 0:
            s = Fn.drag_lift_coefficients(Fn.boundary_traction_force(m3, w.cpu().numpy(), NU, ob), Lc=0.1 * thick)
            r = Fn.drag_lift_coefficients(Fn.reaction_force(P, w, ob), Lc=0.1 * thick)
        else:
            s = r = (float("nan"), float("nan"))
        P.close()
        return m3.num_tets, s, r, rn

    if "A" in args.sections:
        emit("\n== A. DFG 2D-1, 2-D UGN path ==")
        emit(f"{'level':>5} {'tris':>9} | {'C_d surface':>12} {'err':>10} | {'C_d residual':>12} {'err':>10} | "
             f"{'C_l surface':>12} {'err':>9} | {'C_l residual':>12} {'err':>9}")
        errs = []
        for n in (2, 4, 8, 16):
            m = M2.dfg_2d_mesh(n)
            mask, g = M2.dfg2d_bcs(m).flatten()
            P = FlowProblem(m, (mask, g), reynolds=1.0 / NU)
            U, _ = P.stokes_solve()
            U.view(-1, 4)[:, 3] *= NU
            w, _ = P.newton_solve(U)
            cd, cl = M2.drag_lift_2d(m, w.cpu().numpy(), NU)
            cdx, clx = M2.drag_lift_2d_reaction(P, w)
            P.close()
            errs.append((abs(cd - cdr), abs(cdx - cdr), abs(cl - clr), abs(clx - clr)))
            emit(f"{n:>5} {m.num_cells:>9} | {cd:12.7f} {pct(cd, cdr):>10} | {cdx:12.7f} {pct(cdx, cdr):>10} | "
                 f"{cl:12.8f} {pct(cl, clr):>9} | {clx:12.8f} {pct(clx, clr):>9}")
        for k, name in ((0, "C_d surface"), (1, "C_d residual"), (2, "C_l surface"), (3, "C_l residual")):
            e = [x[k] for x in errs]
            emit(f"  observed order {name}: " + ", ".join(f"{np.log2(e[i] / e[i + 1]):.2f}" for i in range(3))
                 + f"  (levels 2->4, 4->8, 8->16; 4->16 averaged: {np.log2(e[1] / e[3]) / 2:.2f})")

    if "B" in args.sections:
        emit("\n== B. DFG 2D-1 on the 3-D tet path (one-cell slab), per unit depth ==")
        for corrected in (0, 1):
            emit(f"-- corrected_convection = {corrected} ({'consistent' if corrected else 'as written'})")
            errs = []
            for n in (4, 8, 16):
                nt, (cd, cl), (cdx, clx), rn = slab_solve(n, corrected)
                errs.append((abs(cd - cdr), abs(cdx - cdr)))
                emit(f"{n:>5} {nt:>9} | C_d surface {cd:.7f} ({pct(cd, cdr)}), residual {cdx:.7f} ({pct(cdx, cdr)}) | "
                     f"C_l surface {cl:.8f} ({pct(cl, clr)}), residual {clx:.8f} ({pct(clx, clr)})")
            emit("  observed C_d order (4->8, 8->16): surface " + ", ".join(f"{np.log2(errs[i][0] / errs[i + 1][0]):.2f}" for i in range(2))
                 + "; residual " + ", ".join(f"{np.log2(errs[i][1] / errs[i + 1][1]):.2f}" for i in range(2)))

    if "C" in args.sections:
        emit("\n== C. DFG 3D-1Z pillar (body-centred Delaunay), Re 20; literature C_d 6.05-6.25, C_l 0.008-0.010 ==")
        for n, corrected in ((24, 0), (32, 0), (40, 0), (24, 1), (32, 1), (40, 1)):
            m = M.reorder_for_locality(M.dfg_pillar_mesh(n, lattice="bcc"))[0]
            t = m.meta["tags"]
            P = FlowProblem(m, B.dfg_bcs(m), reynolds=1.0 / NU, corrected_convection=corrected)
            U, _ = P.stokes_solve()
            w, rn = P.newton_solve(U.clone())
            if rn.reason <= 0:
                emit(f"  W/{n}, corrected_convection = {corrected}: Newton failed ({rn.reason})")
                P.close()
                continue
            cd, cl = Fn.drag_lift_coefficients(Fn.boundary_traction_force(m, w.cpu().numpy(), NU, t["obstacle"]))
            r1 = Fn.drag_lift_coefficients(Fn.reaction_force(P, w, t["obstacle"]))
            rh = Fn.drag_lift_coefficients(Fn.reaction_force(P, w, t["obstacle"], rim_tags=(t["wall"],), rim_weight=0.5))
            r0 = Fn.drag_lift_coefficients(Fn.reaction_force(P, w, t["obstacle"], rim_tags=(t["wall"],), rim_weight=0.0))
            nrim = int(np.count_nonzero(Fn.tag_node_weights(m, t["obstacle"], rim_tags=(t["wall"],), rim_weight=0.5) == 0.5))
            emit(f"  W/{n}, corrected_convection = {corrected}: {m.num_tets} tets, {len(m.facet_nodes(t['obstacle']))} obstacle nodes ({nrim} on the rim) | surface C_d "
                 f"{cd:.5f} C_l {cl:.5f} | residual rim 1: C_d {r1[0]:.5f} C_l {r1[1]:.5f} | rim 1/2: C_d {rh[0]:.5f} "
                 f"C_l {rh[1]:.5f} | rim 0: C_d {r0[0]:.5f} C_l {r0[1]:.5f}")
            P.close()

    if "D" in args.sections:
        emit("\n== D. What the reference constants tell apart, level-4 slab, both functionals (C_d) ==")
        lo = slab_solve(4, 1)
        hi = slab_solve(4, 0)
        emit(f"  bracket [consistent, as written]: surface [{pct(lo[1][0], cdr)}, {pct(hi[1][0], cdr)}]; "
             f"residual [{pct(lo[2][0], cdr)}, {pct(hi[2][0], cdr)}]")
        for name, kw in (("C_I 4", dict(c_inverse=4.0)), ("no G:G", dict(c_inverse=0.0)), ("LSIC off", dict(lsic_scale=0.0)),
                         ("LSIC x4", dict(lsic_scale=4.0)), ("1-point", dict(one_point_quadrature=True)),
                         ("C_I 144", dict(c_inverse=144.0))):
            _, s, r, rn = slab_solve(4, 0, **kw)
            ins = (lambda v, a, b: "inside" if min(a, b) <= v <= max(a, b) else "OUTSIDE")
            emit(f"  {name:9s} surface C_d {s[0]:.6f} ({pct(s[0], cdr)}, {ins(s[0], lo[1][0], hi[1][0])} the bracket) | "
                 f"residual C_d {r[0]:.6f} ({pct(r[0], cdr)}, {ins(r[0], lo[2][0], hi[2][0])} the bracket)")

    if "E" in args.sections:
        emit("\n== E. cost on the 10 M-tet duct (300 x 75 x 75 cells, bench.py's mesh) ==")
        m = M.duct_mesh((300, 75, 75), 4.0)
        t = m.meta["tags"]
        mask, g = B.duct_bcs(m).flatten()
        P = FlowProblem(m, (mask, g), reynolds=100.0)
        rng = np.random.default_rng(0)
        w = torch.from_numpy(rng.normal(size=4 * m.num_nodes)).cuda()
        w[torch.from_numpy(mask.astype(bool)).cuda()] = torch.from_numpy(g[mask.astype(bool)]).cuda()
        F = P.zeros()
        outlet = torch.from_numpy(Fn.tag_node_weights(m, t["outlet"])).cuda()
        one = torch.ones(m.num_nodes, dtype=torch.float64, device="cuda")

        def timed(f, reps=7):
            f()
            ts, wall = [], []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                ts.append(e0.elapsed_time(e1))
            return float(np.median(ts)), float(np.median(wall))

        for name, f in (("phi = outlet plane", lambda: P.residual_moments(w, outlet)),
                        ("phi = 1", lambda: P.residual_moments(w, one)),
                        ("phi = outlet plane, Stokes", lambda: P.residual_moments(w, outlet, "stokes")),
                        ("sns_residual (NS)", lambda: P.residual(w, out=F))):
            ev, wl = timed(f)
            emit(f"  {name:28s} {ev:8.3f} ms (events), {wl:8.3f} ms (host clock)   [{m.num_tets} tets, {int(outlet.sum().item())} outlet nodes]")
        P.close()
    fh.close()


if __name__ == "__main__":
    main()
