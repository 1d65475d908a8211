"""Writes profiles/stability.txt: the cost record of the linear stability analysis (csrc/sns_stability.hip).

  0  per kernel, the VGPR / SGPR / scratch / LDS figures of the gfx950 compile (-Rpass-analysis=kernel-resource-usage); needs
     hipcc, no GPU
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets): ms of the mass pass beside sns_residual and sns_spmv in the same
     run -- warm-up, device-event timing, median and range of the repeats
  B  there, one m = 32 analysis at the Newton state (Re 100, ksp_rtol 1e-10): wall time, the solves (the handle's Krylov
     timer), assembly and set-up (its timers), the mass passes (33 x the median of A), and what is left: orthogonalisation,
     the vector kernels around it and the host reads
  C  the leading eigenvalues of the coarse DFG slab (mesh2d.dfg2d_slab_problem) at Re 20 and Re 100
Without a GPU sections A-C say "not measured".

    python scripts/profile_stability.py [--cells 300 75 75] [--repeats 20] [--skip-duct] [--skip-dfg]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "stability.txt")


def resource_usage():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"-I{ROOT}/include", f"-I{CSRC}",
           "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "sns_stability.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"name": name.replace("(anonymous namespace)::", "").split("(")[0]}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


def _progress(what):
    print(f"[profile_stability] {what}", file=sys.stderr, flush=True)


def measure_duct(cells, repeats, m_steps):
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh(tuple(cells), 4.0)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=100.0)
    _progress("duct problem built")
    U, rs = P.stokes_solve()
    _progress("Stokes start done")
    w, rn = P.newton_solve(U.clone())
    _progress("Newton done")
    L = [f"   state: Newton from the Stokes solution at Re 100, {rn.its} iterations, reason {rn.reason}"]
    x = torch.from_numpy(np.random.default_rng(0).standard_normal(m.num_dofs)).cuda()
    y, F = P.zeros(), P.zeros()
    P.jacobian(w, "ns")
    ptr = lambda t: t.data_ptr()
    lib, h = P.lib, P.h
    calls = {"sns_mass_apply": lambda: lib.sns_mass_apply(h, ptr(w), ptr(x), ptr(y)),
             "sns_residual": lambda: lib.sns_residual(h, 1, ptr(w), ptr(F)),
             "sns_spmv": lambda: lib.sns_spmv(h, ptr(x), ptr(y))}
    ms = {}
    for name, fn in calls.items():
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
        ms[name] = (statistics.median(ts), min(ts), max(ts))
    _progress("passes timed")
    # one analysis
    P.set_options(ksp_rtol=1e-10)
    P.reset_timings()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    V, H, res = P.stability_arnoldi(w, shift=0.0, m=m_steps)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    tm = P.timings()
    analysis = dict(wall=wall, krylov=tm.krylov_ms, assemble=tm.assemble_ms, setup=tm.pc_setup_ms, its=res.ksp_its, m_done=res.m_done,
                    reason=res.reason, mass=(res.m_done + 1) * ms["sns_mass_apply"][0])
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import ritz_pairs
    lam, _, est = ritz_pairs(H, res.m_done, 0.0)
    analysis["lam"] = [(complex(l), float(e)) for l, e in zip(lam, est) if e <= 1e-7][:4]
    n, E = m.num_nodes, m.num_tets
    P.close()
    return n, E, ms, analysis, L


def measure_dfg(n_level):
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh2d as M2
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, linear_stability, newton_with_reynolds_continuation
    L = []
    for label, u_max in (("Re 20 (2D-1: steady)", 0.3), ("Re 100 (2D-2: periodic)", 1.5)):
        m3, (mask, g), thick = M2.dfg2d_slab_problem(n_level, u_max=u_max)
        P = FlowProblem(m3, (mask, g), reynolds=1000.0, corrected_convection=1, snes_atol=1e-13, snes_rtol=1e-10, snes_stol=1e-12,
                        ksp_rtol=1e-8)
        U, rs = P.stokes_solve()
        U.view(-1, 4)[:, 3] *= 1e-3
        w, rn = newton_with_reynolds_continuation(P, U)
        _progress(f"DFG slab {label}: steady state done")
        t0 = time.perf_counter()
        r = linear_stability(P, w, n_modes=6, shift=0.0, m=64)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        L.append(f"   {label}: slab level {n_level}, {m3.num_nodes} nodes, {m3.num_tets} tets; Newton reason {rn.reason} ({rn.its} its); "
                 f"m_done {r.m_done}, reason {r.reason}, {r.ksp_its} Krylov its, {sec:.2f} s")
        for lam, est, ok in zip(r.eigenvalues, r.estimates, r.converged):
            L.append(f"      lambda = {lam.real:+.6f} {lam.imag:+.6f}i   frequency Im/2pi = {lam.imag / 6.283185307179586:.6f}   estimate {est:.1e}"
                     f"   {'converged' if ok else 'NOT converged'}")
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
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    L = ["Linear stability analysis (sns_mass_apply, sns_stability_arnoldi): resource usage and measurements",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_usage()
    for r in rows:
        L.append("   %-40s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    L.append("   scratch of the new kernels: %d bytes/lane" % max(r.get("ScratchSize", 0) for r in rows))
    L.append("   form: one pass, owner-computes; the 4 lanes of a row split the row's cells and sum their partial rows in a fixed order")
    import torch
    gpu = torch.cuda.is_available()
    if gpu and not a.skip_duct:
        n, E, ms, an, notes = measure_duct(a.cells, a.repeats, a.steps)
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: duct {a.cells[0]} x {a.cells[1]} x {a.cells[2]}, {n} nodes, {E} tets; 3 warm-up calls, "
                 f"device events around each call (launch to stream sync), median (min .. max) of {a.repeats}")
        L += notes
        for k, (med, lo, hi) in ms.items():
            L.append(f"   {k:16s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})")
        ratio = ms["sns_mass_apply"][0] / ms["sns_residual"][0]
        L.append(f"   mass pass / sns_residual = {ratio:.2f}" + ("" if ratio <= 1.0 else
                 "   SLOWER than the residual: the residual runs one lane per tet and gathers 16 doubles per (node, cell), the mass pass"
                 " recomputes the cell's geometry and tau once per (node, cell) -- four times per tet -- to stay free of element scratch"))
        L.append("   (sns_residual at a state that satisfies its Dirichlet data takes the one-lane-per-tet pass and no lifting; profiles/recovery.txt"
                 " timed it at a random state, 5.7 ms.  Not measured: the pass under a form variant or a viscosity field, counters, a shift > 0)")
        L.append(f"B  MEASURED there: one analysis, m = {a.steps}, shift 0, ksp_rtol 1e-10 (one run, host timer around the call)")
        rest = an["wall"] - an["krylov"] - an["assemble"] - an["setup"] - an["mass"]
        L.append(f"   wall {an['wall']:.1f} ms; m_done {an['m_done']}, reason {an['reason']}, {an['its']} Krylov iterations over {an['m_done'] + 1} solves")
        L.append(f"   solves (the handle's Krylov timer) {an['krylov']:.1f} ms; assembly {an['assemble']:.1f} ms; set-up {an['setup']:.1f} ms")
        L.append(f"   mass passes {an['mass']:.1f} ms (= {an['m_done'] + 1} x the median of A, not timed inside the run)")
        L.append(f"   rest {rest:.1f} ms: orthogonalisation (2 passes per step, chunks of 8), norms, scalings, one host read per step (by subtraction)")
        for lam, est in an["lam"]:
            L.append(f"   converged pair: lambda = {lam.real:+.6f} {lam.imag:+.6f}i   estimate {est:.1e}")
    else:
        L.append("A  times at the 300 x 75 x 75 duct: not measured" + (" (no GPU where this file was written)" if not gpu else " (skipped)"))
        L.append("B  cost of one m = 32 analysis there: not measured")
    if gpu and not a.skip_dfg:
        L.append(f"C  MEASURED on {torch.cuda.get_device_name(0)}: DFG slab, steady state by Newton with Reynolds continuation, linear_stability(n_modes=6, shift=0, m=64)")
        L.append("   the benchmark's own facts: 2D-1 (Re 20) is steady, 2D-2 (Re 100) periodic -- the leading real part must be < 0 and > 0; recorded, not pinned in a test")
        L += measure_dfg(a.dfg_level)
    else:
        L.append("C  leading eigenvalues of the DFG slab at Re 20 and Re 100: not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
