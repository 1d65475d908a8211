"""Writes profiles/stability_left.txt: the cost record of the left stability modes (k_mass_pass<., true, 1>, sns_stability_arnoldi_left,
solver.linear_stability(left=True), solver.eigenvalue_reynolds_sensitivity).

  0  per kernel, the VGPR / SGPR / scratch / occupancy figures of the gfx950 compile, the transposed pass beside the forward one
     (scripts/profile_stability.py's reader); needs hipcc, no GPU
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets) of profiles/stability.txt: ms of one B^T pass and one B pass on the
     same mesh in the same process -- warm-up, device-event timing, median and range of the repeats -- and their ratio beside
     the bytes either pass loads per (row, cell)
  B  there, linear_stability at m = 32 (ksp_rtol 1e-10) right-only and with left=True: wall time, Krylov iterations of either
     process, how many of the modes found a partner
  C  there, eigenvalue_reynolds_sensitivity of the leading paired mode: wall time, the two Newton solves' share, the value
  D  the DFG slab at Re 100 (the unstable pair of profiles/stability.txt): left modes, d lambda / d Re and the Re_c estimate
  E  the headline lines of bench.py for the parent and for this change, from the file given with --bench-lines (recorded by
     whoever ran them; this script does not run the benchmark)
Without a GPU sections A-D say "not measured".

    python scripts/profile_stability_left.py [--cells 300 75 75] [--repeats 20] [--skip-duct] [--skip-dfg] [--bench-lines FILE]
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
OUT = os.path.join(ROOT, "profiles", "stability_left.txt")

# what one (row, cell) visit loads, from the kernels' text: the tet's 4 vertex ids, 4 x 3 coordinates, 4 x 3 velocities, the 4
# mask words, and 4 x 3 entries of x (B x) or 4 x 4 entries of z (B^T z, the pressure too)
BYTES_B = 16 + 96 + 96 + 16 + 96
BYTES_BT = 16 + 96 + 96 + 16 + 128


def _progress(what):
    print(f"[profile_stability_left] {what}", file=sys.stderr, flush=True)


def _event_ms(fn, repeats):
    import torch
    for _ in range(3):
        assert fn() == 0
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def measure_duct(cells, repeats, m_steps):
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    m = M.duct_mesh(tuple(cells), 4.0)
    P = S.FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=100.0)
    _progress("duct problem built")
    U, _ = P.stokes_solve()
    w, rn = P.newton_solve(U.clone())
    _progress("Newton done")
    L = [f"   duct {cells[0]} x {cells[1]} x {cells[2]}, {m.num_nodes} nodes, {m.num_tets} tets; state: Newton from the Stokes solution at Re 100, "
         f"{rn.its} iterations, reason {rn.reason}"]
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(m.num_dofs)).cuda()
    y = P.zeros()
    lib, h, ptr = P.lib, P.h, (lambda t: t.data_ptr())
    ms_b = _event_ms(lambda: lib.sns_mass_apply(h, ptr(w), ptr(x), ptr(y)), repeats)
    ms_t = _event_ms(lambda: lib.sns_mass_apply_transpose(h, ptr(w), ptr(x), ptr(y)), repeats)
    _progress("passes timed")
    ratio = ms_t[0] / ms_b[0]
    L.append(f"   3 warm-up calls, device events around each call (launch to stream sync), median (min .. max) of {repeats}")
    L.append(f"   sns_mass_apply            {ms_b[0]:9.3f} ms ({ms_b[1]:.3f} .. {ms_b[2]:.3f})")
    L.append(f"   sns_mass_apply_transpose  {ms_t[0]:9.3f} ms ({ms_t[1]:.3f} .. {ms_t[2]:.3f})")
    L.append(f"   B^T pass / B pass = {ratio:.3f}; bytes loaded per (row, cell): {BYTES_BT} against {BYTES_B} (x {BYTES_BT / BYTES_B:.3f}: the pressure entries of z)")
    if ratio < 1.0:
        L.append('   below 1 although it loads 10 % more per visit: its quadrature loop carries u and tau alone (the Galerkin sum is closed-form, grad z is formed outside), where the forward pass interpolates x and forms three products per point; counters not measured')
    elif ratio > BYTES_BT / BYTES_B:
        L.append('   above what the extra pressure loads account for: one wave per SIMD fewer (134 against 118-120 VGPRs) leaves less latency hiding for the same gathers; counters not measured')
    B_sec = []
    walls = {}
    for left in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = S.linear_stability(P, w, n_modes=6, shift=0.0, m=m_steps, left=left)
        torch.cuda.synchronize()
        walls[left] = time.perf_counter() - t0
        _progress(f"linear_stability left={left} done")
        if not left:
            B_sec.append(f"   right only: wall {walls[left]:.2f} s; m_done {r.m_done}, reason {r.reason}, {r.ksp_its} Krylov iterations; {int(r.converged.sum())} of {len(r.converged)} modes converged")
        else:
            B_sec.append(f"   left=True:  wall {walls[left]:.2f} s; right {r.ksp_its} + left {r.left_ksp_its} Krylov iterations (left m_done {r.left_m_done}, reason {r.left_reason}); "
                         f"{int(r.left_converged.sum())} of {len(r.converged)} modes have a converged left partner")
            B_sec.append(f"   left=True / right only = {walls[True] / walls[False]:.2f} (the second process runs on the transposed hierarchy, set up once more)")
            for lam, ok in zip(r.eigenvalues, r.left_converged):
                B_sec.append(f"      lambda = {lam.real:+.6f} {lam.imag:+.6f}i   {'paired' if ok else 'NO left partner'}")
    C_sec = []
    paired = [k for k, ok in enumerate(r.left_converged) if ok]
    if paired:
        k = paired[0]
        P.reset_timings()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dlam, Re_c = S.eigenvalue_reynolds_sensitivity(P, w, r, k=k)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        tm = P.timings()
        C_sec.append(f"   mode {k}, rel_step 1e-3: wall {sec:.2f} s (two Newton solves, 2 x 2 operator passes and mass passes, one assembly to restore); "
                     f"of it Krylov {tm.krylov_ms / 1e3:.2f} s, assembly {tm.assemble_ms / 1e3:.2f} s, set-up {tm.pc_setup_ms / 1e3:.2f} s (the handle's timers)")
        C_sec.append(f"   d lambda / d Re = {dlam.real:+.6e} {dlam.imag:+.6e}i; Re_c estimate {Re_c:.4g} (a stable duct mode: the estimate is an extrapolation, recorded, not a finding)")
        C_sec.append(f"   against two more analyses of {walls[False]:.2f} s each for a finite difference of eigenvalues: x {2.0 * walls[False] / sec:.1f}")
    else:
        C_sec.append("   no mode with a converged left partner at this m: not measured")
    P.close()
    return L, B_sec, C_sec


def measure_dfg(n_level):
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    m3, (mask, g), thick = M2.dfg2d_slab_problem(n_level, u_max=1.5)
    P = S.FlowProblem(m3, (mask, g), reynolds=1000.0, corrected_convection=1, snes_atol=1e-13, snes_rtol=1e-10, snes_stol=1e-12, ksp_rtol=1e-8)
    U, _ = P.stokes_solve()
    U.view(-1, 4)[:, 3] *= 1e-3
    w, rn = S.newton_with_reynolds_continuation(P, U)
    _progress("DFG slab: steady state done")
    t0 = time.perf_counter()
    r = S.linear_stability(P, w, n_modes=6, shift=0.0, m=64, left=True)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    L = [f"   slab level {n_level}, {m3.num_nodes} nodes, {m3.num_tets} tets, 1/nu = 1000 (physical Re = U_mean D / nu = 100); Newton reason {rn.reason}; "
         f"linear_stability(left=True, m=64) {sec:.2f} s, right {r.ksp_its} + left {r.left_ksp_its} Krylov its"]
    for lam, lamL, ok in zip(r.eigenvalues, r.left_eigenvalues, r.left_converged):
        L.append(f"      lambda = {lam.real:+.6f} {lam.imag:+.6f}i   " + (f"left Ritz value differs by {abs(lam - lamL):.1e}" if ok else "NO left partner"))
    paired = [k for k, ok in enumerate(r.left_converged) if ok]
    if paired:
        k = paired[0]
        t0 = time.perf_counter()
        dlam, Re_c = S.eigenvalue_reynolds_sensitivity(P, w, r, k=k)
        torch.cuda.synchronize()
        L.append(f"   mode {k}: d lambda / d(1/nu) = {dlam.real:+.6e} {dlam.imag:+.6e}i in {time.perf_counter() - t0:.2f} s; linear estimate of the crossing 1/nu = {Re_c:.1f}, "
                 f"i.e. physical Re_c = {0.1 * Re_c:.1f} (the literature's onset of shedding behind a confined cylinder lies well below 100; a linear "
                 "extrapolation over that distance on this coarse slab is an indication, not a result)")
        wm = S.structural_sensitivity(P, w, r, k)
        top = int(wm.argmax())
        L.append(f"   wavemaker of mode {k}: maximum {float(wm.max()):.3e} at node {top}, x = {m3.points[top][0]:.3f}, y = {m3.points[top][1]:.3f} "
                 "(the cylinder's centre is at (0.2, 0.2), its radius 0.05)")
    P.close()
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--dfg-level", type=float, default=1)
    ap.add_argument("--skip-duct", action="store_true")
    ap.add_argument("--skip-dfg", action="store_true")
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from profile_stability import resource_usage
    L = ["Left stability modes (sns_mass_apply_transpose, sns_stability_arnoldi_left, linear_stability(left=True), eigenvalue_reynolds_sensitivity): resource usage and measurements",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_usage()
    for r in rows:
        L.append("   %-40s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    scratch = max(r.get("ScratchSize", 0) for r in rows if "k_mass_pass<" in r["name"] and ", true, 1>" in r["name"])
    L.append(f"   scratch of the transposed pass k_mass_pass<., true, 1>: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: the pass spills"))
    L.append("   the transposed pass holds grad z (12 values) beside the metric where the forward pass holds none: more VGPRs, one wave per SIMD fewer; "
             "capped at 128 VGPRs (__launch_bounds__(256, 4)) it spills 36 bytes/lane, so it is not capped")
    import torch
    gpu = torch.cuda.is_available()
    if gpu and not a.skip_duct:
        A_sec, B_sec, C_sec = measure_duct(a.cells, a.repeats, a.steps)
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: one B^T pass and one B pass, same mesh, same process")
        L += A_sec
        L.append(f"B  MEASURED there: linear_stability(n_modes=6, shift=0, m={a.steps}, ksp_rtol=1e-10), one run each, host timer around the call")
        L += B_sec
        L.append("C  MEASURED there: eigenvalue_reynolds_sensitivity, one run, host timer around the call")
        L += C_sec
    else:
        why = " (no GPU where this file was written)" if not gpu else " (skipped)"
        L.append("A  one B^T pass beside one B pass at the 300 x 75 x 75 duct: not measured" + why)
        L.append("B  linear_stability right-only and with left=True there: not measured")
        L.append("C  eigenvalue_reynolds_sensitivity there: not measured")
    if gpu and not a.skip_dfg:
        L.append(f"D  MEASURED on {torch.cuda.get_device_name(0)}: DFG slab at Re 100, steady state by Newton with Reynolds continuation")
        L += measure_dfg(a.dfg_level)
    else:
        L.append("D  left modes and the Re_c estimate of the DFG slab at Re 100: not measured")
    if a.bench_lines and os.path.exists(a.bench_lines):
        L.append("E  python bench.py, headline lines as recorded from the runs named below (MEASURED on the MI355X; the spread between runs is 3 %, DESIGN.md)")
        L += ["   " + ln.rstrip("\n") for ln in open(a.bench_lines)]
    else:
        L.append("E  python bench.py, parent against this change: not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
