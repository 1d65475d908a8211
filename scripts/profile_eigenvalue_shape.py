"""Writes profiles/eigenvalue_shape.txt: the cost record of the eigenvalue shape pass (k_eigshape_tet,
sns_jacobian_shape_gradient) beside the two kernels it descends from.

  0  per instantiation of k_eigshape_tet (csrc/sns_eigshape.hip), the VGPR / AGPR / SGPR / scratch / occupancy figures of the
     gfx950 compile, beside k_shape_tet (csrc/sns_shape.hip) and k_state_gradient (csrc/sns_hessian.hip); needs hipcc, no GPU
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets) of profiles/hessian.txt, in ONE process: ms of one call of
     sns_jacobian_shape_gradient, sns_residual_shape_gradient and sns_jacobian_state_gradient -- each an element kernel, its
     gather and a stream synchronise -- the three alternated, 3 warm-up rounds, device events, median and range
  B  the element kernels alone, from the kernel statistics of a rocprofv3 --kernel-trace --stats run of this script's
     --calls-only mode (a run of its own: tracing slows the host), given with --kernel-stats FILE
     (rocprofv3's result database, or its kernel-statistics CSV)
Without a GPU section A says "unmeasured"; without --kernel-stats section B does.

    rocprofv3 --kernel-trace --stats -d DIR -o eigshape -- python scripts/profile_eigenvalue_shape.py --calls-only
    python scripts/profile_eigenvalue_shape.py [--cells 300 75 75] [--repeats 20] [--kernel-stats DIR/eigshape_results.db]
                                               [--recorded-calls FILE]
"""
import argparse
import csv
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "eigenvalue_shape.txt")
KERNELS = ("k_eigshape_tet", "k_shape_tet", "k_state_gradient")


def _progress(what):
    print(f"[profile_eigenvalue_shape] {what}", file=sys.stderr, flush=True)


def resource_rows():
    from profile_hessian import resource_usage
    rows = []
    for unit in ("sns_eigshape.hip", "sns_shape.hip", "sns_hessian.hip"):
        rows += [r for r in resource_usage(unit) if any(k in r["name"] for k in KERNELS)]
    return rows


def _setup(cells):
    """The duct problem with a smooth divergence-free-looking state and two random vectors: the passes' cost does not depend on
    the values, so no Newton solve is spent on it."""
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    m = M.duct_mesh(tuple(cells), 4.0)
    P = S.FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=100.0)
    _progress("duct problem built")
    p = m.points
    w = np.zeros((m.num_nodes, 4))
    w[:, 0] = (1.0 - (2.0 * p[:, 1]) ** 2) * (1.0 - (2.0 * p[:, 2]) ** 2)
    w[:, 1] = 0.05 * np.sin(3.0 * p[:, 0]) * np.cos(2.0 * p[:, 2])
    w[:, 2] = 0.05 * np.cos(2.0 * p[:, 0]) * np.sin(3.0 * p[:, 1])
    w[:, 3] = 0.1 * (4.0 - p[:, 0])
    rng = np.random.default_rng(0)
    vec = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()
    return m, P, vec(w), vec(rng.standard_normal(m.num_dofs)), vec(rng.standard_normal(m.num_dofs))


def _calls(P, w, x, z):
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib
    lib, h, ptr = P.lib, P.h, (lambda t: t.data_ptr())
    gX = torch.empty(P.n_local, 3, dtype=torch.float64, device="cuda")
    g = P.zeros()
    return [("sns_jacobian_shape_gradient", lambda: lib.sns_jacobian_shape_gradient(h, ptr(w), ptr(x), ptr(z), 1.0, 0.7, ptr(gX))),
            ("sns_residual_shape_gradient", lambda: lib.sns_residual_shape_gradient(h, _lib.FORM_NS, ptr(w), ptr(z), ptr(gX))),
            ("sns_jacobian_state_gradient", lambda: lib.sns_jacobian_state_gradient(h, ptr(w), ptr(x), ptr(z), 1.0, 0.7, ptr(g)))]


def measure_calls(cells, repeats, timed=True):
    import torch
    m, P, w, x, z = _setup(cells)
    calls = _calls(P, w, x, z)
    for _ in range(3):
        for _, fn in calls:
            assert fn() == 0
    ts = {name: [] for name, _ in calls}
    for _ in range(repeats):                                # alternated: a drift of the clocks hits all three alike
        for name, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert fn() == 0
            b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b))
    P.close()
    _progress("calls timed")
    if not timed:
        return []
    med = {k: statistics.median(v) for k, v in ts.items()}
    L = [f"   duct {cells[0]} x {cells[1]} x {cells[2]}, {m.num_nodes} nodes, {m.num_tets} tets; a smooth state, random x and z (the cost does not depend on the values)",
         f"   3 warm-up rounds, then {repeats} rounds of the three calls alternated; device events around each call (launch to stream sync); median (min .. max)"]
    for name, _ in calls:
        L.append(f"   {name:30s} {med[name]:9.3f} ms ({min(ts[name]):.3f} .. {max(ts[name]):.3f})   element kernel + gather")
    new = med["sns_jacobian_shape_gradient"]
    L.append(f"   shape pass / residual shape gradient = {new / med['sns_residual_shape_gradient']:.2f}, / Hessian pass = {new / med['sns_jacobian_state_gradient']:.2f}")
    return L


def kernel_stats(path):
    """(name, calls, mean ms, min ms, max ms) of the three element kernels from what rocprofv3 --kernel-trace --stats left: its
    kernel-statistics CSV (--output-format csv) or its result database (the default; the ``kernels`` view: name, duration ns)."""
    per = {}
    if path.endswith(".db"):
        import sqlite3
        con = sqlite3.connect(path)
        for name, dur in con.execute("select name, duration from kernels"):
            if any(k in name for k in KERNELS):
                per.setdefault(name, []).append(float(dur) * 1e-6)
        con.close()
        rows = [(n, len(v), statistics.mean(v), min(v), max(v)) for n, v in per.items()]
    else:
        rows = []
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                low = {k.strip().lower(): v for k, v in row.items()}
                if any(k in low.get("name", "") for k in KERNELS):
                    rows.append((low["name"], int(low["calls"]), float(low["averagens"]) * 1e-6, float(low["minns"]) * 1e-6, float(low["maxns"]) * 1e-6))
    short = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("sns::", "")
    return sorted((short(n), c, m, lo, hi) for n, c, m, lo, hi in rows)


def recorded_section_a(path):
    """The lines of section A of an earlier output of this script (written where a GPU was)."""
    lines = open(path).read().split("\n")
    start = next((i for i, ln in enumerate(lines) if ln.startswith("A  MEASURED")), None)
    if start is None:
        return []
    end = next(i for i in range(start + 1, len(lines) + 1) if i == len(lines) or lines[i].startswith("B  "))
    return lines[start:end]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls-only", action="store_true", help="run the calls and write nothing (the program of a rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel-statistics CSV or its result database (.db)")
    ap.add_argument("--recorded-calls", default=None, help="an earlier output of this script written on a GPU: its section A is carried over")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.calls_only:
        measure_calls(a.cells, a.repeats, timed=False)
        return
    L = ["The eigenvalue shape pass (sns_jacobian_shape_gradient): resource usage and measurements",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_rows()
    for r in rows:
        L.append("   %-40s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    scratch = max(r.get("ScratchSize", 0) for r in rows if "k_eigshape_tet" in r["name"])
    L.append(f"   scratch of k_eigshape_tet: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: the pass spills"))
    L.append("   k_eigshape_tet holds three P1 fields with their gradients (state, x, z), the adjoints of all six gradients and of G: all 256 VGPRs and "
             "190-195 AGPRs as spill space, no scratch memory, one wave per SIMD.  The single cell function (per-cell constants first, then the "
             "quadrature loop) met the target of 0 bytes of scratch as first written; the split into a J part and a B part was not needed and not tried")
    import torch
    gpu = torch.cuda.is_available()
    if gpu:
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: one call of the shape pass beside the residual shape gradient and the Hessian pass, same mesh, same process")
        L += measure_calls(a.cells, a.repeats)
    elif a.recorded_calls and os.path.exists(a.recorded_calls) and recorded_section_a(a.recorded_calls):
        L += recorded_section_a(a.recorded_calls)
    else:
        L.append("A  one call of sns_jacobian_shape_gradient beside sns_residual_shape_gradient and sns_jacobian_state_gradient at the 300 x 75 x 75 duct: "
                 "unmeasured (no GPU where this file was written)")
        L.append("   sns_jacobian_shape_gradient: unmeasured   sns_residual_shape_gradient: unmeasured   sns_jacobian_state_gradient: unmeasured   ratios: unmeasured")
    stats = kernel_stats(a.kernel_stats) if a.kernel_stats and os.path.exists(a.kernel_stats) else []
    if stats:
        L.append("B  MEASURED: the element kernels alone, rocprofv3 --kernel-trace --stats of the --calls-only mode (a run of its own, same mesh): mean (min .. max) over the calls, warm-up included")
        for name, calls, mean, lo, hi in stats:
            L.append(f"   {name:40s} {mean:9.3f} ms ({lo:.3f} .. {hi:.3f})   {calls} calls")
        mean = {}
        for name, calls, m_, _, _ in stats:
            key = next(k for k in KERNELS if k in name)
            mean.setdefault(key, []).append(m_)
        if all(k in mean for k in KERNELS):
            e = statistics.mean(mean["k_eigshape_tet"])
            L.append(f"   k_eigshape_tet / k_shape_tet = {e / statistics.mean(mean['k_shape_tet']):.2f}, / k_state_gradient = {e / statistics.mean(mean['k_state_gradient']):.2f}")
    else:
        L.append("B  the element kernels alone (k_eigshape_tet, k_shape_tet, k_state_gradient; rocprofv3 kernel statistics): unmeasured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
