"""Writes profiles/complex_shift.txt: the cost record of the stability analysis with a complex or negative shift (k_mass_pass<., ., 2>,
k_cdot8, k_caxpy8; sns_shifted_apply, sns_shifted_solve, sns_stability_arnoldi_shifted; solver.linear_stability(shift=complex)).

  0  per kernel of the feature, the VGPR / SGPR / scratch / LDS / occupancy figures of the gfx950 compile
     (scripts/profile_hessian.py's reader); needs hipcc, no GPU
  1  bytes of one complex operator application against the four separate passes, and the memory of the inner solver; arithmetic
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets): ms of one sns_shifted_apply against 2 sns_spmv + 2 sns_mass_apply (the
     four passes it replaces, entry points the library had before), and the pair pass's share against the two mass passes --
     warm-up, device-event timing, median and range of the repeats
  B  there, linear_stability(shift=complex) for pc_shift = |s| and pc_shift = max(Re s, 0): wall time, inner iterations, restarts,
     converged modes
  C  the same on the DFG slab at Re 100 at a shift near the unstable pair, beside the real-shift figures of
     profiles/krylov_schur.txt
  D  bench.py's headline line against the parent commit: measured outside this script (alternating runs), quoted with --bench-note
Without a GPU sections A to C say "not measured".

    python scripts/profile_complex_shift.py [--cells 300 75 75] [--repeats 20] [--shift -0.5 1.0] [--skip-duct] [--skip-dfg]
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "complex_shift.txt")
KERNELS = (("sns_stability.hip", "k_mass_pass"), ("sns_kernels.hip", "k_cdot8"), ("sns_kernels.hip", "k_caxpy8"))


def _progress(what):
    print(f"[profile_complex_shift] {what}", file=sys.stderr, flush=True)


def _event_ms(fn, repeats):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def _fmt(ms):
    return f"{ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})"


def time_operator(P, w, repeats):
    """One complex operator application against the passes it replaces, on the problem's assembled matrix."""
    import torch
    x = torch.complex(torch.cos(0.3 * torch.arange(P.ndof, dtype=torch.float64, device=P.device)),
                      torch.sin(0.7 * torch.arange(P.ndof, dtype=torch.float64, device=P.device)))
    xp = P._planar(x)
    xr, xi = xp[:P.ndof], xp[P.ndof:]
    yp, t = torch.empty_like(xp), P.zeros()
    lib, h = P.lib, P.h
    ptr = lambda v: v.data_ptr()

    def fused(c_im):
        assert lib.sns_shifted_apply(h, ptr(w), -1.0, c_im, 0, ptr(xp), ptr(yp)) == 0

    def spmv2():
        assert lib.sns_spmv(h, ptr(xr), ptr(t)) == 0 and lib.sns_spmv(h, ptr(xi), ptr(t)) == 0

    def mass2():
        assert lib.sns_mass_apply(h, ptr(w), ptr(xr), ptr(t)) == 0 and lib.sns_mass_apply(h, ptr(w), ptr(xi), ptr(t)) == 0

    full, a2, b2 = _event_ms(lambda: fused(2.0), repeats), _event_ms(spmv2, repeats), _event_ms(mass2, repeats)
    return [f"   sns_shifted_apply (2 operator passes + the pair pass, one call)   {_fmt(full)}",
            f"   2 x sns_spmv (two calls, each with its stream sync)              {_fmt(a2)}",
            f"   2 x sns_mass_apply (two calls)                                   {_fmt(b2)}",
            f"   the four separate passes {a2[0] + b2[0]:.3f} ms (without the vector operations that combine them) against {full[0]:.3f} ms: "
            f"x {(a2[0] + b2[0]) / full[0]:.2f}; the pair pass alone, by difference, {full[0] - a2[0]:.3f} ms against {b2[0]:.3f} ms for the two mass passes"]


def time_stability(P, S, w, shift, n_modes, m, restarts):
    import torch
    L = []
    for label, pc in (("|s|", abs(shift)), ("max(Re s, 0)", max(shift.real, 0.0))):
        P.reset_timings()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = S.linear_stability(P, w, n_modes=n_modes, shift=shift, m=m, max_restarts=restarts, pc_shift=pc)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        solves = r.m_done + 1 if r.restarts == 0 else None
        L.append(f"   pc_shift = {label} = {pc:.3g}: wall {sec:.2f} s; m_done {r.m_done}, reason {r.reason}, restarts {r.restarts}, {r.ksp_its} inner "
                 f"iterations" + (f" over {solves} solves ({r.ksp_its / solves:.1f} each)" if solves else "") +
                 f"; {int(r.converged.sum())} of {len(r.converged)} modes converged (true residual <= 1e-7); leading "
                 f"{', '.join(f'{l.real:+.4f}{l.imag:+.4f}i' for l in r.eigenvalues[:4])}; the handle's Krylov timer {P.timings().krylov_ms / 1e3:.2f} s")
        _progress(f"linear_stability pc_shift {label} done")
    return L


def measure_duct(cells, repeats, shift, m, restarts):
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    msh = M.duct_mesh(tuple(cells), 4.0)
    P = S.FlowProblem(msh, B.duct_bcs(msh).flatten(), reynolds=100.0, gmres_restart=60)
    U, _ = P.stokes_solve()
    w, rn = P.newton_solve(U.clone())
    _progress("duct: Newton done")
    head = [f"   duct {cells[0]} x {cells[1]} x {cells[2]}, {msh.num_nodes} nodes, {msh.num_tets} tets, ndof {msh.num_dofs}; state: Newton from the "
            f"Stokes solution at Re 100, {rn.its} iterations, reason {rn.reason}; gmres_restart 60"]
    P.jacobian(w)
    A_sec = head + [f"   3 warm-up calls, device events around each group of calls, median (min .. max) of {repeats}"] + time_operator(P, w, repeats)
    B_sec = time_stability(P, S, w, shift, 6, m, restarts)
    P.close()
    return A_sec, B_sec


def measure_dfg(n_level, shift, m, restarts):
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    m3, (mask, g), _ = M2.dfg2d_slab_problem(n_level, u_max=1.5)
    P = S.FlowProblem(m3, (mask, g), reynolds=1000.0, corrected_convection=1, snes_atol=1e-13, snes_rtol=1e-10, snes_stol=1e-12, ksp_rtol=1e-8,
                      gmres_restart=60)
    U, _ = P.stokes_solve()
    U.view(-1, 4)[:, 3] *= 1e-3
    w, rn = S.newton_with_reynolds_continuation(P, U)
    _progress("DFG slab: steady state done")
    L = [f"   slab level {n_level}, {m3.num_nodes} nodes, {m3.num_tets} tets, 1/nu = 1000 (physical Re 100); Newton reason {rn.reason}; shift {shift}"]
    L += time_stability(P, S, w, shift, 4, m, restarts)
    P.close()
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shift", type=float, nargs=2, default=[-0.5, 1.0], help="the duct's shift (re, im)")
    ap.add_argument("--dfg-shift", type=float, nargs=2, default=[2.0, 17.0])
    ap.add_argument("--dfg-level", type=float, default=1)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--restarts", type=int, default=20)
    ap.add_argument("--skip-duct", action="store_true")
    ap.add_argument("--skip-dfg", action="store_true")
    ap.add_argument("--bench-note", default=None, help="a file whose lines are quoted as section D")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from profile_hessian import resource_usage
    L = ["Complex and negative shifts of the stability analysis (sns_shifted_apply, sns_shifted_solve, sns_stability_arnoldi_shifted): resource usage and cost",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    scratch = 0
    for unit in sorted({u for u, _ in KERNELS}):
        for r in resource_usage(unit):
            if any(u == unit and k in r["name"] for u, k in KERNELS):
                L.append("   %-52s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
                scratch = max(scratch, r.get("ScratchSize", 0))
    L.append(f"   scratch over the kernels of the feature: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: a kernel spills"))
    L.append("   k_mass_pass<corrected, transposed, NP>: the single-vector passes (NP = 1) hold 118 - 134 VGPRs; the second part (NP = 2) costs the difference")
    L.append("1  Bytes and memory -- arithmetic, not measured")
    L.append("   one complex operator application reads the operator twice (two passes) and the mesh data of the mass pass ONCE; the four "
             "separate passes read the mesh data twice and need three more vector passes to combine c B x into y")
    L.append("   cfgmres holds (2 r + 1) planar vectors of 2 ndof doubles: at gmres_restart r = 30 and the 10.1 M-tet duct (ndof 7.0 M) 6.8 GB, "
             "at r = 60 13.5 GB; the Arnoldi basis stays real, (m + 1) ndof doubles")
    import torch
    gpu = torch.cuda.is_available()
    if gpu and not a.skip_duct:
        A_sec, B_sec = measure_duct(a.cells, a.repeats, complex(*a.shift), a.m, a.restarts)
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: one complex operator application against the four separate passes")
        L += A_sec
        L.append(f"B  MEASURED there: linear_stability(n_modes=6, shift={complex(*a.shift)}, m={a.m}, max_restarts={a.restarts}, ksp_rtol=1e-10), "
                 "one run each, host timer around the call")
        L += B_sec
    else:
        why = " (no GPU where this file was written)" if not gpu else " (skipped)"
        L.append("A  one sns_shifted_apply against 2 sns_spmv + 2 sns_mass_apply at the 300 x 75 x 75 duct, and what fusing the pair pass gains: not measured" + why)
        L.append("B  linear_stability(shift=complex) there, inner iteration counts under the AMG preconditioner and wall time for pc_shift = |s| "
                 "and max(Re s, 0), and which of the two is the better default: not measured" + why)
    if gpu and not a.skip_dfg:
        L.append(f"C  MEASURED on {torch.cuda.get_device_name(0)}: the DFG slab at Re 100 (real-shift figures: profiles/krylov_schur.txt, profiles/stability.txt)")
        L += measure_dfg(a.dfg_level, complex(*a.dfg_shift), a.m, a.restarts)
    else:
        L.append("C  linear_stability(shift near 2 + 17i) on the DFG slab at Re 100 against the real-shift run of profiles/krylov_schur.txt: not measured"
                 + (" (no GPU where this file was written)" if not gpu else " (skipped)"))
    if a.bench_note and os.path.exists(a.bench_note):
        L.append("D  bench.py's headline line against the parent commit (alternating runs)")
        L += ["   " + ln.rstrip() for ln in open(a.bench_note)]
    else:
        L.append("D  bench.py's headline line against the parent commit in alternating runs: not measured here (the benchmark's path -- Newton, "
                 "BiCGStab, the V-cycle -- runs no code of this feature)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
