"""Writes profiles/recovery.txt: the cost record of gradient recovery (csrc/sns_recover.hip).

  0  per kernel, the VGPR / SGPR / scratch / LDS figures of the gfx950 compile (-Rpass-analysis=kernel-resource-usage); needs
     hipcc, no GPU
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets): ms of recover_gradient (G + D, D only), error_indicator (G given)
     and, in the same run, sns_residual -- warm-up, device-event timing, median of the repeats -- and each kernel's
     algorithmic bytes over its time as a fraction of the 8 TB/s HBM peak
Without a GPU section A says "not measured".

    python scripts/profile_recovery.py [--cells 300 75 75] [--repeats 20]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "recovery.txt")
HBM_PEAK = 8.0e12


def resource_usage():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"-I{ROOT}/include", f"-I{CSRC}",
           "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "sns_recover.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            cur = {"name": name.split("(")[0]}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


def algorithmic_bytes(n, E, dim):
    """Bytes each kernel must move once: k_recover reads the lists (8 (n+1) + 4 (dim+1) E), the connectivity (16 E), pts (24 n)
    and w (32 n) and writes G (96 n) and / or D (48 n); k_zz reads the connectivity, pts, the velocity of w (24 n), 72 n of G
    and writes 16 E."""
    base = 8 * (n + 1) + 4 * (dim + 1) * E + 16 * E + 24 * n + 32 * n
    return {"recover G+D": base + 144 * n, "recover D": base + 48 * n, "indicator": 16 * E + 24 * n + 24 * n + 72 * n + 16 * E}


def measure(cells, repeats):
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh(tuple(cells), 4.0)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=100.0)
    w = torch.from_numpy(np.random.default_rng(0).standard_normal(m.num_dofs)).cuda()
    n, E = m.num_nodes, m.num_tets
    G = torch.empty(n, 4, 3, dtype=torch.float64, device="cuda")
    D = torch.empty(n, 6, dtype=torch.float64, device="cuda")
    e2, g2, F = torch.empty(E, dtype=torch.float64, device="cuda"), torch.empty(E, dtype=torch.float64, device="cuda"), P.zeros()
    ptr = lambda t: None if t is None else t.data_ptr()
    lib, h = P.lib, P.h
    calls = {"recover G+D": lambda: lib.sns_recover_gradient(h, ptr(w), ptr(G), ptr(D)),
             "recover D": lambda: lib.sns_recover_gradient(h, ptr(w), None, ptr(D)),
             "indicator": lambda: lib.sns_error_indicator(h, ptr(w), ptr(G), ptr(e2), ptr(g2)),
             "sns_residual": lambda: lib.sns_residual(h, 1, ptr(w), ptr(F))}
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
    P.close()
    return n, E, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    L = ["Gradient recovery (sns_recover_gradient, sns_error_indicator): resource usage and measurements",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_usage()
    for r in rows:
        L.append("   %-28s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    L.append("   scratch of the new kernels: %d bytes/lane" % max(r.get("ScratchSize", 0) for r in rows))
    L.append("   form: one pass, owner-computes (4 lanes per node, every lane recomputes the cell geometry); the two-pass alternative"
             " (per-cell kernel into Fe + gather) was not built, so there is no second time to compare")
    import torch
    if torch.cuda.is_available():
        n, E, ms = measure(a.cells, a.repeats)
        by = algorithmic_bytes(n, E, 3)
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: duct {a.cells[0]} x {a.cells[1]} x {a.cells[2]}, {n} nodes, {E} tets; 3 warm-up calls, "
                 f"device events around each call (launch to stream sync), median (min .. max) of {a.repeats}")
        for k, (med, lo, hi) in ms.items():
            s = f"   {k:14s} {med:9.3f} ms ({lo:.3f} .. {hi:.3f})"
            if k in by:
                s += f"   algorithmic bytes {by[k] / 1e6:.1f} MB -> {by[k] / (med * 1e-3) / 1e12:.3f} TB/s = {100 * by[k] / (med * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s"
            L.append(s)
        L.append("   (error_indicator with G given; each time includes the call's stream synchronise)")
    else:
        L.append("A  times at the 300 x 75 x 75 duct: not measured (no GPU where this file was written)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
