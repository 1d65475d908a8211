"""Writes profiles/rawjac.txt: the cost record of the raw-Jacobian pass (k_raw_jacobian_apply, sns_raw_jacobian_apply) and the
accuracy of solver.dirichlet_sensitivity against the oracle's exact discrete gradient.

  0  per instantiation of csrc/sns_rawjac.hip, the VGPR / AGPR / SGPR / scratch / occupancy figures of the gfx950 compile; needs
     hipcc, no GPU.  --keep-compile-section takes the section from the existing record instead of compiling (for a run on a
     GPU machine, where compiling costs GPU time)
  A  on an MI355X, at a duct of --cells: ms of one pass per direction beside bench_assemble's Jacobian time on the same handle,
     in the same process -- warm-up, device-event timing, median and range -- for the plain form, corrected_convection, and a
     time term
  B  there, duct633: solver.dirichlet_sensitivity (pressure difference, reaction drag) against tests/rawjac_oracle.py's exact
     discrete gradient, relative 2-norm error of the whole vector
  C  the headline lines of bench.py for the parent and for this change, from the file given with --bench-lines (recorded by
     whoever ran them; this script does not run the benchmark)
Without a GPU sections A and B say "not measured".

    python scripts/profile_rawjac.py [--cells 200 50 50] [--repeats 20] [--keep-compile-section] [--bench-lines FILE] [--out FILE]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "rawjac.txt")
HEAD_A = "A. one pass beside the Jacobian assembly"


def _progress(what):
    print(f"[profile_rawjac] {what}", file=sys.stderr, flush=True)


def resource_usage(unit):
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"-I{ROOT}/include", f"-I{CSRC}",
           "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, unit), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"name": name.replace("void ", "").split("(")[0]}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


def compile_section():
    L = ["0. gfx950 compile of csrc/sns_rawjac.hip (template arguments: form 1 = NS, 3 = UGN 2-D; corrected, TT, VL, EV)",
         f"   {'kernel':58s} VGPRs AGPRs SGPRs scratch occupancy LDS"]
    rows = resource_usage("sns_rawjac.hip")
    for r in rows:
        L.append(f"   {r['name']:58s} {r.get('VGPRs', -1):5d} {r.get('AGPRs', 0):5d} {r.get('TotalSGPRs', -1):5d} {r.get('ScratchSize', -1):7d} "
                 f"{r.get('Occupancy', -1):9d} {r.get('LDS Size', 0):3d}")
    scratch = max(r.get("ScratchSize", 0) for r in rows)
    L.append(f"   scratch: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: the pass spills"))
    L.append("   The 3-D instantiations sit at 256 VGPRs, one wave per SIMD, as k_fused_lift's heavier variants do (profiles/external_fields.txt):")
    L.append("   the block code holds the metric, the state at the quadrature points and one 4 x 4 block at once.  The AGPRs are the")
    L.append("   allocator's spill space in the register file; nothing goes to memory.")
    return L


def kept_compile_section():
    if not os.path.exists(OUT):
        return ["0. gfx950 compile: no earlier record to keep"]
    keep, on = [], False
    for ln in open(OUT).read().splitlines():
        if ln.startswith("0. "):
            on = True
        elif ln.startswith(HEAD_A[:3]):
            break
        if on:
            keep.append(ln)
    while keep and not keep[-1].strip():
        keep.pop()
    return keep


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


def timing_section(cells, repeats):
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    L = [f"{HEAD_A}: duct {cells[0]} x {cells[1]} x {cells[2]}, {repeats} repeats"]
    _progress("mesh")
    m = M.duct_mesh(tuple(cells), 4.0)
    mask, g = B.duct_bcs(m).flatten()
    L.append(f"   {m.num_nodes} nodes, {m.num_tets} tets; per call: median (min .. max) ms by device events, the call's stream synchronisation included")
    for name, opt, tt in (("plain", {}, False), ("corrected_convection", dict(corrected_convection=1), False), ("time term", {}, True)):
        _progress(name)
        P = FlowProblem(m, (mask, g), reynolds=100.0, **opt)
        U, res = P.stokes_solve()
        assert res.reason > 0
        if tt:
            P.set_time_term(3.0, 40.0, U)
        x = torch.cos(0.5 + 0.61 * torch.arange(P.ndof, dtype=torch.float64, device=P.device))
        y = P.zeros()
        fwd = _event_ms(lambda: P.raw_jacobian_apply(U, x, out=y), repeats)
        bwd = _event_ms(lambda: P.raw_jacobian_apply(U, x, transpose=True, out=y), repeats)
        asm = P.bench_assemble(U, "ns", reps=max(3, repeats // 4))
        L.append(f"   {name:22s} J0 x {fwd[0]:8.3f} ({fwd[1]:.3f} .. {fwd[2]:.3f})   J0^T x {bwd[0]:8.3f} ({bwd[1]:.3f} .. {bwd[2]:.3f})   "
                 f"Jacobian assembly (bench_assemble) {asm:8.3f}   ratio {fwd[0] / asm:.2f} / {bwd[0] / asm:.2f}")
        P.close()
    L.append("   Expectation: about 1 x the assembly -- the same 16 blocks per tet, each formed once.  Each block is formed by the lane")
    L.append("   that needs it, so the metric and the quadrature-point scalars of a tet are computed once per (row, cell, b), as in")
    L.append("   k_fused_offdiag; the pass stores 4 doubles per row where the assembly stores the blocks.")
    return L


def accuracy_section():
    import numpy as np
    import torch
    import rawjac_oracle as RO
    import stability_oracle as SO
    from stabilized_navier_stokes_flow_fenicsx_amd import functionals as Fn
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, dirichlet_sensitivity
    c = SO.case("duct633")
    m = c.mesh
    P = FlowProblem(m, (c.mask, c.g), reynolds=c.Re, ksp_rtol=1e-12, snes_rtol=1e-12, snes_atol=1e-12, snes_stol=1e-12)
    w, nres = P.newton_solve(torch.from_numpy(c.w).cuda())
    J0 = RO.raw_jacobian(m.points, m.tets, c.w, c.Re)
    wall = m.meta["tags"]["wall"]
    z = np.zeros(len(c.w))
    z[0::4] = Fn.tag_node_weights(m, wall)
    gp = Fn.pressure_difference_gradient(m, np.array([0.5, 0.03, -0.02]), np.array([1.5, 0.03, -0.02]))
    L = ["B. solver.dirichlet_sensitivity on duct633 against the oracle's exact discrete gradient (relative 2-norm error, whole vector)"]
    for name, grad_o, grad in (("pressure difference", gp, torch.from_numpy(gp).cuda()),
                               ("reaction drag", -(J0.T @ z), Fn.reaction_force_gradient(P, w, wall)[0])):
        ref, _ = RO.dirichlet_gradient(J0, c.mask, grad_o)
        dJ, _, res = dirichlet_sensitivity(P, w, grad)
        err = np.linalg.norm(dJ.cpu().numpy() - ref) / np.linalg.norm(ref)
        L.append(f"   {name:20s} {err:.2e}   (adjoint solve: {res.its} its, reason {res.reason}; the test's bound is 1e-6)")
    P.close()
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[200, 50, 50])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--keep-compile-section", action="store_true")
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    L = ["Cost record of the raw-Jacobian pass (written by scripts/profile_rawjac.py)", ""]
    L += kept_compile_section() if a.keep_compile_section else compile_section()
    L.append("")
    gpu = False
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        pass
    if gpu:
        L += timing_section(a.cells, a.repeats) + [""] + accuracy_section()
    else:
        L += [f"{HEAD_A}: not measured (no GPU)", "", "B. solver.dirichlet_sensitivity against the exact discrete gradient: not measured (no GPU)"]
    L.append("")
    L.append("C. bench.py headline lines (parent, this change)")
    if a.bench_lines and os.path.exists(a.bench_lines):
        L += ["   " + ln.rstrip() for ln in open(a.bench_lines) if ln.strip()]
    else:
        L.append("   not recorded")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
