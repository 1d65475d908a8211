"""Writes profiles/scalar_transport.txt: the cost record of the scalar-transport assembly (csrc/sns_scalar.hip).

  0  the VGPR / SGPR / scratch / occupancy figures of the gfx950 compile (-Rpass-analysis=kernel-resource-usage); needs hipcc,
     no GPU
  A  on an MI355X, per mesh (default: the 300 x 75 x 75 duct, 10.1 M tets, and the 100 x 25 x 25 duct for machines short of
     memory): ms of sns_scalar_system -- the handle's device events around the pass, 3 warm-up calls, median (min .. max) of the
     repeats -- beside the same handle's NS Jacobian assembly (sns_bench_assemble, one timed assembly per repeat), their ratio
     against the yardstick of 1.25, and the iterations and wall time of one steady four-species solve at the Stokes state
Without a GPU section A says "not measured".

    python scripts/profile_scalar.py [--cells 300 75 75 --cells 100 25 25] [--repeats 20]
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
OUT = os.path.join(ROOT, "profiles", "scalar_transport.txt")
KAPPA = (1e-1, 1e-2, 1e-3, 1e-4)
YARDSTICK = 1.25


FINDING = [
    "B  FINDING where the ratio is above the yardstick (first measured at 2.07 on the 10.1 M-tet duct, 1.79 on the 375 k-tet one; reasoned from the code and the two times, not from counters): the",
    "   scalar pass is not bound by its stores.  It writes the same vals array as the NS assembly at about half the NS pass's rate, so the",
    "   strided 32-byte stores the yardstick allowed for are not what it waits for.  What differs is the shape of the work: the NS route",
    "   runs one lane per off-diagonal SLOT (about 14 lanes per node, each over the 4-6 contributions of its slot) plus 4 lanes per node",
    "   for the diagonal block; this pass runs 4 lanes per ROW, and every lane walks the ~15 slots of its row and all their contributions",
    "   one after the other -- about 90 element evaluations in a chain per lane, each behind a dependent gather (c_idx -> tet -> points /",
    "   velocities), at 4 waves per SIMD (126 VGPRs).  It exposes a quarter of the NS route's lanes with chains several times as long, and",
    "   it evaluates the cell geometry 64 times per tet (16 contributions x 4 species lanes) where the NS route does it 16 times.  The",
    "   remedy is the other shape the design allowed: slot-owner lanes that evaluate the geometry once per contribution and all four",
    "   species' entries from it (the whole 128-byte block stored by one lane), plus a row pass for the right-hand side.  Not done here:",
    "   the assembly is 3 % of the steady solve it serves at 10 M tets (11.5 ms of 388 ms), and the record was to come first.",
]


def resource_usage():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"-I{ROOT}/include", f"-I{CSRC}",
           "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "sns_scalar.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            k = re.search(r"\bk_\w+", name)
            cur = {"name": k.group(0) if k else name}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


def spread(ts):
    return statistics.median(ts), min(ts), max(ts)


def measure(cells, repeats):
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.drivers import inner_stream_inlet_data
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh(tuple(cells), 4.0)
    P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=100.0)
    U, sres = P.stokes_solve()
    mask, val = inner_stream_inlet_data(m)
    bcs = (np.repeat(mask, 4, axis=1), np.repeat(val, 4, axis=1))
    ns, sc = [], []
    for _ in range(3):
        P.bench_assemble(U, "ns", reps=1)
    for _ in range(repeats):
        ns.append(P.bench_assemble(U, "ns", reps=1))
    for i in range(3 + repeats):
        t0 = P.timings().assemble_ms
        P.scalar_system(U, KAPPA, bcs)
        if i >= 3:
            sc.append(P.timings().assemble_ms - t0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c, res = P.scalar_solve(U, KAPPA, bcs)
    torch.cuda.synchronize()
    solve_s = time.perf_counter() - t0
    out_nodes = m.facet_nodes(m.meta["tags"]["outlet"])
    co = c[torch.as_tensor(out_nodes, device=c.device)]
    rng = [(float(co[:, k].min()), float(co[:, k].max())) for k in range(4)]
    n, E, nnzb = m.num_nodes, m.num_tets, P.sizes()["nnzb"]
    P.close()
    return dict(n=n, E=E, nnzb=nnzb, ns=spread(ns), sc=spread(sc), stokes_its=sres.its, its=res.its, reason=res.reason,
                rnorm=res.rnorm, solve_s=solve_s, outlet=rng)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, action="append")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    meshes = a.cells or [[300, 75, 75], [100, 25, 25]]
    L = ["Scalar transport (sns_scalar_system, sns_scalar_solve): resource usage and measurements",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_usage()
    for r in rows:
        L.append("   %-28s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    L.append("   scratch of the new kernels: %d bytes/lane" % max(r.get("ScratchSize", 0) for r in rows))
    L.append("   form: one pass, owner-computes (4 lanes per row = the 4 species; a lane walks the row's slots and their contributions,"
             " recomputes the cell geometry per contribution, stores 32 bytes of every block); the slot-owner + row-pass alternative"
             " was not built, so there is no second time to compare")
    import torch
    if torch.cuda.is_available():
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: 3 warm-up calls, device events around each assembly, median (min .. max) of "
                 f"{a.repeats}; kappa = {KAPPA}, inlet-stream indicator as inlet data of all four species, Stokes state, default options")
        for cells in meshes:
            r = measure(cells, a.repeats)
            ratio = r["sc"][0] / r["ns"][0]
            L.append(f"   duct {cells[0]} x {cells[1]} x {cells[2]}: {r['n']} nodes, {r['E']} tets, {r['nnzb']} blocks")
            L.append("      sns_scalar_system   %9.3f ms (%.3f .. %.3f)   vals written: %.1f MB" % (*r["sc"], r["nnzb"] * 128 / 1e6))
            L.append("      NS Jacobian (bench) %9.3f ms (%.3f .. %.3f)" % r["ns"])
            L.append(f"      ratio scalar / NS   {ratio:9.3f}   (yardstick {YARDSTICK}: {'within' if ratio <= YARDSTICK else 'ABOVE -- a finding, see below'})")
            L.append(f"      steady 4-species solve: {r['its']} iterations, reason {r['reason']}, |r| {r['rnorm']:.3e}, {r['solve_s']:.3f} s wall "
                     f"(assembly + set-up + Krylov; the Stokes solve before it took {r['stokes_its']} iterations)")
            L.append("      concentration at the outlet (min, max) per species: " + ", ".join("(%.4f, %.4f)" % t for t in r["outlet"]))
        L += FINDING
    else:
        L.append("A  times: not measured (no GPU where this file was written)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
