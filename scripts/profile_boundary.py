"""Writes profiles/boundary_terms.txt: the cost record of the boundary terms (csrc/sns_boundary.hip).

  0  the VGPR / SGPR / LDS / scratch / occupancy figures of the gfx950 compile (-Rpass-analysis=kernel-resource-usage); needs
     hipcc, no GPU
  A  nothing set: on an MI355X, on the 300 x 75 x 75 duct (10.1 M tets), sns_bench_assemble (NS Jacobian with residual) and the
     bench.py headline of THIS tree and of a tree of the parent commit (--parent DIR: a checkout with its library built), run
     alternately in one session, each run a process of its own; beside them the spread of the parent's own repeats
  B  terms set: the same assembly with t and beta on the inlet and outlet facets; the added time as a share of the assembly
  C  what is not measured
Without a GPU (or without --parent) the sections say "not measured".  profiles/boundary_terms_first_session.txt is the output of
an earlier session of the same day (without --slab), kept beside the record because the two sessions differ in whether the
head's assembly median falls inside the parent's spread of three medians (0.29 % wide there, 0.11 % here).

    python scripts/profile_boundary.py [--parent DIR] [--runs 3] [--cells 300 75 75] [--slab]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
OUT = os.path.join(ROOT, "profiles", "boundary_terms.txt")

# one process of a tree (cwd = the tree): the duct, 3 warm-up assemblies, `repeats` timed ones (device events inside
# sns_bench_assemble, one assembly each); with terms = 1 the same again with t and beta on the inlet and outlet facets
WORKER = r"""
import json, sys
import numpy as np
sys.path.insert(0, ".")
from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
cells, repeats, terms = tuple(int(x) for x in sys.argv[1:4]), int(sys.argv[4]), int(sys.argv[5])
m = M.duct_mesh(cells, 4.0)
P = FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=200.0)
w = P.g_dev.clone()
def timed():
    for _ in range(3):
        P.bench_assemble(w, "ns", reps=1)
    return [P.bench_assemble(w, "ns", reps=1) for _ in range(repeats)]
out = dict(n=m.num_nodes, E=m.num_tets, off=timed())
if terms:
    tags = m.meta["tags"]
    ids = np.concatenate([m.find(tags["inlet"]), m.find(tags["outlet"])])
    rng = np.random.default_rng(0)
    P.set_boundary_facets(ids)
    P.set_boundary_flow(traction=rng.normal(size=(len(ids), 3, 3)), backflow=rng.uniform(0.5, 2.0, len(ids)))
    out.update(on=timed(), facets=len(ids))
    P.clear_boundary_terms()
    out.update(off_again=timed())
P.close()
print("RESULT " + json.dumps(out))
"""


def resource_usage():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", f"-I{ROOT}/include", f"-I{CSRC}",
           "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "sns_boundary.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = [], None
    for ln in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            k = re.search(r"\bk_\w+(<\w+>)?", name)
            cur = {"name": k.group(0) if k else name}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


def run_worker(tree, cells, repeats, terms):
    p = subprocess.run([sys.executable, "-c", WORKER, *map(str, cells), str(repeats), str(int(terms))], cwd=tree, capture_output=True,
                       text=True, timeout=400)
    for ln in p.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise RuntimeError(f"worker in {tree} gave no result (rc {p.returncode}): {p.stderr[-800:]}")


def run_bench(tree, steps, warmup):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                       capture_output=True, text=True, timeout=500)
    for ln in reversed(p.stdout.splitlines()):
        if ln.startswith("{"):
            d = json.loads(ln)
            return float(d["value"]), float(d["ms_per_step"])
    raise RuntimeError(f"bench.py in {tree} gave no result line (rc {p.returncode}): {p.stderr[-800:]}")


def med(ts):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slab", action="store_true", help="also the unsteady slab run with and without beta (long)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    L = ["Boundary terms (sns_set_boundary_facets, sns_set_boundary_flow, sns_set_boundary_scalar): resource usage and measurements",
         "=" * 118,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = resource_usage()
    for r in rows:
        L.append("   %-32s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    scratch = max(r.get("ScratchSize", 0) for r in rows if r["name"].startswith(("k_boundary_flow", "k_boundary_scalar")))
    L.append(f"   scratch of the two kernels of the pass (k_boundary_flow, k_boundary_scalar): {scratch} bytes/lane"
             + ("" if scratch == 0 else "  -- NOT 0 as expected"))
    import torch
    gpu = torch.cuda.is_available()
    if gpu and a.parent:
        name = torch.cuda.get_device_name(0)
        c = a.cells
        L.append(f"A  NOTHING SET, MEASURED on {name}: duct {c[0]} x {c[1]} x {c[2]}; parent commit and this tree alternately, {a.runs} runs each, every run a "
                 f"process of its own; sns_bench_assemble: 3 warm-up, median (min .. max) of {a.repeats} single timed assemblies (NS Jacobian with "
                 f"residual, fused route); bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}")
        rec = {"parent": [], "head": []}
        for i in range(a.runs):
            for who, tree in (("parent", a.parent), ("head", ROOT)):
                w = run_worker(tree, c, a.repeats, False)
                v, ms = run_bench(tree, a.steps, a.warmup)
                rec[who].append((statistics.median(w["off"]), v, ms))
                L.append(f"   run {i + 1} {who:6s}: assembly {med(w['off'])} ms   bench {v:.3f} M-DOF/s, {ms:.3f} ms per step   ({w['E']} tets)")
                print(L[-1], flush=True)
        for k, label, fmt in ((0, "assembly median, ms", "%.3f"), (1, "bench headline, M-DOF/s", "%.3f"), (2, "bench ms per step", "%.3f")):
            pa, he = [r[k] for r in rec["parent"]], [r[k] for r in rec["head"]]
            inside = min(pa) <= statistics.median(he) <= max(pa)
            L.append(f"   {label:26s} parent {' '.join(fmt % x for x in pa)} (spread {fmt % min(pa)} .. {fmt % max(pa)} = "
                     f"{100.0 * (max(pa) - min(pa)) / statistics.median(pa):.2f} %)   head {' '.join(fmt % x for x in he)}   head's median "
                     f"{'within' if inside else 'OUTSIDE'} the parent's spread ({100.0 * (statistics.median(he) / statistics.median(pa) - 1.0):+.2f} % "
                     f"against the parent's median)")
        L.append("   nothing new is launched with nothing set (assemble() asks BoundaryState::flow_on() and returns): no existing number can move by the code")
    else:
        L.append("A  nothing set, parent against this tree: not measured (needs a GPU and --parent)")
    if gpu:
        w = run_worker(ROOT, a.cells, a.repeats, True)
        off, on = statistics.median(w["off"]), statistics.median(w["on"])
        L.append(f"B  TERMS SET, MEASURED: the same assembly with t and beta on the {w['facets']} inlet and outlet facets (every facet's beta > 0; the state is the "
                 f"Dirichlet data extended by zero: the inlet's points take the inflow branch, the outlet's contribute nothing)")
        L.append(f"   nothing set   {med(w['off'])} ms")
        L.append(f"   terms set     {med(w['on'])} ms")
        L.append(f"   cleared again {med(w['off_again'])} ms")
        L.append(f"   added time {on - off:+.3f} ms = {100.0 * (on - off) / off:+.2f} % of the assembly it rides on (one launch over "
                 f"{w['facets']} facets' rows against {w['E']} tets; no threshold)")
    else:
        L.append("B  terms set: not measured (no GPU where this file was written)")
    if a.slab and gpu:
        L.append("C  THE UNSTEADY DFG 2D-2 SLAB RUN (drivers.run_dfg2d2_slab) with and without backflow_beta, MEASURED as far as the lines below go; NOT "
                 "MEASURED: the point where the run without the term diverges, unless a line below shows it")
    else:
        L.append("C  NOT MEASURED: the unsteady DFG 2D-2 slab run (drivers.run_dfg2d2_slab) with and without backflow_beta up to the point where the "
                 "run without it diverges; --slab runs it")
    if a.slab and gpu:
        from stabilized_navier_stokes_flow_fenicsx_amd import drivers as D
        seen = []
        for beta in (0.0, 1.0):
            try:
                r = D.run_dfg2d2_slab(2, 0.01, 800, backflow_beta=beta, verbose=False)
                seen.append((len(r["t"]), r["cd_max"], r["cl_max"], r["strouhal"]))
                L.append(f"   slab level 2, dt 0.01, beta {beta}: {len(r['t'])} of 800 steps converged, max C_d {r['cd_max']:.4f} max C_l {r['cl_max']:.4f} "
                         f"St {r['strouhal']:.4f}, {r['seconds']:.1f} s")
            except Exception as e:                                   # a run that gives up is the record
                L.append(f"   slab level 2, dt 0.01, beta {beta}: stopped with {type(e).__name__}: {str(e)[:200]}")
        if len(seen) == 2 and seen[0] == seen[1]:
            L.append("   the two runs agree in every digit: no quadrature point of the outlet saw u.n < 0 in these steps, so the term never acted, and the run "
                     "without it did not diverge -- the divergence the term is for is NOT shown by this record")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
