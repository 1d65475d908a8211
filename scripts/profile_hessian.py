"""Writes profiles/hessian.txt: the cost record of the Hessian pass (k_state_gradient, sns_jacobian_state_gradient) and the two
eigenvalue sensitivities built on it (solver.eigenvalue_base_flow_sensitivity, solver.eigenvalue_forcing_sensitivity).

  0  per kernel of csrc/sns_hessian.hip, the VGPR / AGPR / SGPR / scratch / occupancy figures of the gfx950 compile, beside
     k_shape_tet of csrc/sns_shape.hip (the kernel whose shape it takes); needs hipcc, no GPU
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets) of profiles/stability_left.txt: ms of one Hessian pass beside
     sns_mass_apply_transpose and sns_residual in the same process -- warm-up, device-event timing, median and range
  B  there, linear_stability(left=True) at m = 32, then the two sensitivity functions of the leading paired mode: wall time,
     Krylov iterations of the two adjoint solves
  C  the DFG slab at Re 100 (the unstable pair of profiles/stability.txt): the forcing sensitivity of the leading mode and
     where its growth-rate part is largest
  D  the headline lines of bench.py for the parent and for this change, from the file given with --bench-lines (recorded by
     whoever ran them; this script does not run the benchmark)
Without a GPU sections A-C say "not measured".

    python scripts/profile_hessian.py [--cells 300 75 75] [--repeats 20] [--skip-duct] [--skip-dfg] [--bench-lines FILE]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "hessian.txt")


def _progress(what):
    print(f"[profile_hessian] {what}", file=sys.stderr, flush=True)


def resource_usage(unit):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"-I{ROOT}/include", f"-I{CSRC}",
           "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, unit), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"name": name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


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


class _CountingSolves:
    """Counts the Krylov iterations of FlowProblem.adjoint_solve while active."""

    def __init__(self, P):
        self.P, self.its, self.orig = P, [], P.adjoint_solve

    def __enter__(self):
        def counted(g, x0=None):
            y, res = self.orig(g, x0)
            self.its.append(res.its)
            return y, res
        self.P.adjoint_solve = counted
        return self

    def __exit__(self, *exc):
        del self.P.adjoint_solve


def _sensitivities(P, w, r, S, points):
    import torch
    paired = [k for k, ok in enumerate(r.left_converged) if ok]
    if not paired:
        return ["   no mode with a converged left partner: not measured"]
    k = paired[0]
    L = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gw = S.eigenvalue_base_flow_sensitivity(P, w, r, k)
    torch.cuda.synchronize()
    L.append(f"   eigenvalue_base_flow_sensitivity, mode {k} (lambda = {r.eigenvalues[k].real:+.6f} {r.eigenvalues[k].imag:+.6f}i): wall {time.perf_counter() - t0:.3f} s "
             f"(eight Hessian passes, two mass passes); max |grad_w lambda| = {float(gw.abs().max()):.3e}")
    with _CountingSolves(P) as cnt:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gf = S.eigenvalue_forcing_sensitivity(P, w, r, k, density=True)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
    L.append(f"   eigenvalue_forcing_sensitivity(density=True): wall {sec:.2f} s (the base-flow sensitivity, one assembly, two adjoint solves at ksp_rtol 1e-10 with "
             f"{' + '.join(map(str, cnt.its))} Krylov iterations, 2 + 8 transposed mass passes)")
    g3 = gf.view(-1, 4)[:, :3]
    mag = torch.linalg.vector_norm(g3.real, dim=1)
    top = int(mag.argmax())
    x = points[top]
    L.append(f"   largest |Re grad_f lambda| (growth rate, per unit volume) = {float(mag[top]):.4e} at node {top}, x = ({x[0]:.3f}, {x[1]:.3f}, {x[2]:.3f}); "
             f"largest |Im grad_f lambda| = {float(torch.linalg.vector_norm(g3.imag, dim=1).max()):.4e}")
    return L


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
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal(m.num_dofs)).cuda()
    z = torch.from_numpy(rng.standard_normal(m.num_dofs)).cuda()
    y = P.zeros()
    lib, h, ptr = P.lib, P.h, (lambda t: t.data_ptr())
    ms_h = _event_ms(lambda: lib.sns_jacobian_state_gradient(h, ptr(w), ptr(x), ptr(z), 1.0, 0.7, ptr(y)), repeats)
    ms_t = _event_ms(lambda: lib.sns_mass_apply_transpose(h, ptr(w), ptr(z), ptr(y)), repeats)
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    ms_r = _event_ms(lambda: lib.sns_residual(h, _lib.FORM_NS, ptr(w), ptr(y)), repeats)
    _progress("passes timed")
    L.append(f"   3 warm-up calls, device events around each call (launch to stream sync), median (min .. max) of {repeats}")
    L.append(f"   sns_jacobian_state_gradient {ms_h[0]:9.3f} ms ({ms_h[1]:.3f} .. {ms_h[2]:.3f})   element pass + gather, (c_jac, c_mass) = (1, 0.7)")
    L.append(f"   sns_mass_apply_transpose    {ms_t[0]:9.3f} ms ({ms_t[1]:.3f} .. {ms_t[2]:.3f})")
    L.append(f"   sns_residual                {ms_r[0]:9.3f} ms ({ms_r[1]:.3f} .. {ms_r[2]:.3f})")
    L.append(f"   Hessian pass / B^T pass = {ms_h[0] / ms_t[0]:.2f}, / residual = {ms_h[0] / ms_r[0]:.2f}; it visits each cell once (the owner-computes passes visit it "
             "once per incident row), loads 4 x (3 + 4 + 4 + 4) doubles and stores 16 per cell, and runs at one wave per SIMD; counters not measured")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = S.linear_stability(P, w, n_modes=6, shift=0.0, m=m_steps, left=True)
    torch.cuda.synchronize()
    Bs = [f"   linear_stability(left=True, m={m_steps}): wall {time.perf_counter() - t0:.2f} s, right {r.ksp_its} + left {r.left_ksp_its} Krylov iterations, "
          f"{int(r.left_converged.sum())} of {len(r.converged)} modes paired"]
    _progress("linear_stability done")
    Bs += _sensitivities(P, w, r, S, m.points)
    P.close()
    return L, Bs


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
    L = [f"   slab level {n_level}, {m3.num_nodes} nodes, {m3.num_tets} tets, 1/nu = 1000 (physical Re = U_mean D / nu = 100); Newton reason {rn.reason}; "
         f"linear_stability(left=True, m=64) {time.perf_counter() - t0:.2f} s"]
    L += _sensitivities(P, w, r, S, m3.points)
    L.append("   (the cylinder's centre is at (0.2, 0.2), its radius 0.05; a steady force where Re grad_f lambda is large and opposed to it lowers the growth rate)")
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
    L = ["The Hessian pass (sns_jacobian_state_gradient) and the eigenvalue sensitivities to base flow and forcing: resource usage and measurements",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_usage("sns_hessian.hip") + [r for r in resource_usage("sns_shape.hip") if "k_shape_tet" in r["name"]]
    for r in rows:
        L.append("   %-40s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    scratch = max(r.get("ScratchSize", 0) for r in rows if "k_state_gradient" in r["name"])
    L.append(f"   scratch of k_state_gradient: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: the pass spills"))
    L.append("   k_state_gradient holds three P1 fields with their gradients (state, x, z) and the adjoints of grad u and grad p: all 256 VGPRs and 58-60 "
             "AGPRs as spill space, no scratch memory, one wave per SIMD; capped at two waves per SIMD (__launch_bounds__(256, 2)) it spills "
             "228 / 244 bytes per lane to scratch memory, so it is not capped")
    import torch
    gpu = torch.cuda.is_available()
    if gpu and not a.skip_duct:
        A_sec, B_sec = measure_duct(a.cells, a.repeats, a.steps)
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: one Hessian pass beside the transposed mass pass and the residual, same mesh, same process")
        L += A_sec
        L.append("B  MEASURED there: the two sensitivity functions of the leading paired mode, one run each, host timer around the call")
        L += B_sec
    else:
        why = " (no GPU where this file was written)" if not gpu else " (skipped)"
        L.append("A  one Hessian pass beside sns_mass_apply_transpose and sns_residual at the 300 x 75 x 75 duct: not measured" + why)
        L.append("B  the two sensitivity functions there: not measured")
    if gpu and not a.skip_dfg:
        L.append(f"C  MEASURED on {torch.cuda.get_device_name(0)}: DFG slab at Re 100, steady state by Newton with Reynolds continuation")
        L += measure_dfg(a.dfg_level)
    else:
        L.append("C  the forcing sensitivity of the DFG slab's leading mode at Re 100: not measured")
    if a.bench_lines and os.path.exists(a.bench_lines):
        L.append("D  python bench.py, headline lines as recorded from the runs named below (MEASURED on the MI355X; the spread between runs is 3 %, DESIGN.md)")
        L += ["   " + ln.rstrip("\n") for ln in open(a.bench_lines)]
    else:
        L.append("D  python bench.py, parent against this change: not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
