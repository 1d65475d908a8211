"""External fields (sns_set_body_force, sns_set_element_viscosity, sns_set_mixture): the records of profiles/external_fields.txt.

  0  resource usage (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; no GPU needed) of every viscosity-field (EV)
     instantiation of csrc/sns_kernels.hip beside its time-term (TT) and viscosity-law (VL) counterparts, and -- with --parent DIR,
     the csrc directory of a checkout of the parent commit -- every kernel of the parent against its figures in this tree
  A  on the (100, 25, 25) duct, state = the Stokes solution: ms per sns_bench_assemble call (Jacobian + residual), five repeats
     of 100 calls each, fields off, a time term alone (TT) and both fields under the same time term (EV), EV / TT as a ratio;
     with --parent-times FILE... (each written by `--times-only FILE --tree PARENT_CHECKOUT` in the same session, alternating
     with `--times-only` runs of this tree given as --bracketed FILE...) the fields-off time against the parent's own spread
  B  Newton / BiCGStab / scalar iteration counts of solver.solve_coupled_flow on that duct at viscosity ratios 1, 4 and 20

    python scripts/profile_fields.py [--out FILE] [--sections 0AB] [--parent DIR] [--parent-times FILE...] [--bracketed FILE...] [--measured FILE]
    python scripts/profile_fields.py --times-only FILE [--tree DIR]

Sections A and B need a GPU.  --measured FILE takes their text from an earlier run of this script on a GPU machine
(--sections AB --out FILE) instead of measuring; without either they are written as "unmeasured".  Nothing is estimated.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS, LENGTH, RE, KAPPA = (100, 25, 25), 4.0, 10.0, 0.004
KEYS = ("VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS Size")
NS_KERNEL = r"k_(element|fused_\w+|residual_tet)<"


def resource_usage(csrc):
    """{demangled kernel: {key: value}} of csrc/sns_kernels.hip."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
           "-I" + os.path.join(csrc, "..", "..", "include"), "-I" + csrc, "-Wno-unused-result", "-c",
           os.path.join(csrc, "sns_kernels.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n") if names else []
    rows, cur, i = {}, None, 0
    for ln in err.splitlines():
        if "Function Name:" in ln:
            cur = re.sub(r"^void sns::|[(].*", "", dem[i])
            i += 1
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur and m.group(1).strip() in KEYS:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    return rows


def smooth_m(points):
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    return 0.5 + 0.5 * np.tanh(3.0 * (0.3 - np.sqrt(y * y + z * z))) * np.cos(0.7 * x)


def assemble_times(tree, fields, repeats=5, reps=100):
    """ms per sns_bench_assemble call, ``repeats`` times, with the package of ``tree``: fields off and, with ``fields``, under a
    time term alone and under the same term with both fields."""
    sys.path.insert(0, tree)
    import torch  # noqa: F401
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh(CELLS, LENGTH)
    P = FlowProblem(m, B.duct_bcs(m), reynolds=RE)
    U, _ = P.stokes_solve()
    out = {}
    for name in (("off", "tt", "ev") if fields else ("off",)):
        if name == "tt":
            P.set_time_term(30.0, 1600.0, U * (-30.0))
        if name == "ev":
            P.set_mixture(smooth_m(m.points), float(np.log(4.0)), (0.0, -2.0, 0.0))
        P.bench_assemble(U, "ns", reps=3)                                  # warm-up
        out[name] = [P.bench_assemble(U, "ns", reps=reps) for _ in range(repeats)]
    P.close()
    return out, m.num_tets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "external_fields.txt"))
    ap.add_argument("--sections", default="0AB")
    ap.add_argument("--parent", default=None, help="csrc directory of a checkout of the parent commit")
    ap.add_argument("--parent-times", default=None, nargs="+", help="one file per run of --times-only on the parent")
    ap.add_argument("--bracketed", default=None, nargs="+", help="--times-only runs of THIS tree made between the parent's runs")
    ap.add_argument("--measured", default=None)
    ap.add_argument("--times-only", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.times_only:
        t, nt = assemble_times(args.tree, fields=False)
        json.dump(dict(off=t["off"], tets=nt), open(args.times_only, "w"))
        print(t)
        return
    fh = open(args.out, "w")

    def emit(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    def row(name, r):
        emit(f"   {name:52s} {r.get('VGPRs', 0):5d} {r.get('AGPRs', 0):5d} {r.get('ScratchSize', 0):7d} {r.get('Occupancy', 0):3d} {r.get('LDS Size', 0):6d}")

    if "0" in args.sections:
        emit("External fields (sns_set_body_force, sns_set_element_viscosity, sns_set_mixture): resource usage and measurements")
        emit("=" * 78)
        new = resource_usage(os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc"))
        emit("0  Resource usage of csrc/sns_kernels.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
        emit("   template arguments: k_element / k_fused_* <form, corrected convection, time term, viscosity law, viscosity field>, k_residual_tet without the form")
        emit("   per new (EV) instantiation: its time-term (TT) counterpart, itself, its viscosity-law (VL) counterpart; a body force runs the TT instantiations")
        emit(f"   {'kernel':52s} {'VGPRs':>5s} {'AGPRs':>5s} {'scratch':>7s} {'occ':>3s} {'LDS':>6s}")
        ev = [k for k in new if re.match(NS_KERNEL, k) and k.endswith(", true, false, true>")]
        scratch = []
        for k in ev:
            row(k.replace(", true, false, true>", ", true, false, false>"), new[k.replace(", true, false, true>", ", true, false, false>")])
            row(k, new[k])
            row(k.replace(", true, false, true>", ", false, true, false>"), new[k.replace(", true, false, true>", ", false, true, false>")])
            if new[k].get("ScratchSize", 0) > 0:
                scratch.append(k)
        emit(f"   new instantiations: {len(ev)}; with scratch: {len(scratch)} {scratch if scratch else ''}")
        if args.parent:
            old = resource_usage(args.parent)
            same = diff = 0
            for k, v in old.items():
                kk = re.sub(r">$", ", false>", k) if re.match(NS_KERNEL, k) else k
                if new.get(kk) == v:
                    same += 1
                else:
                    diff += 1
                    emit(f"   DIFFERS {k}: parent {v} this tree {new.get(kk)}")
            emit(f"   kernels of the parent's sns_kernels.hip: {same + diff}; identical VGPR / AGPR / scratch / occupancy / LDS figures in this "
                 f"tree (the instantiation without a viscosity field): {same}; different: {diff}")
        else:
            emit("   figures of the parent's kernels against this tree: unmeasured (no --parent checkout given)")
    if args.measured:
        fh.write(open(args.measured).read())
        fh.close()
        return
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    if "A" in args.sections:
        if not gpu:
            emit("A  sns_bench_assemble on the (100, 25, 25) duct, fields off / TT / EV / parent: unmeasured (no GPU)")
        else:
            t, nt = assemble_times(ROOT, fields=True)
            off, tt, ev = np.array(t["off"]), np.array(t["tt"]), np.array(t["ev"])
            emit(f"A  {nt} tets, ms per sns_bench_assemble call (Jacobian + residual, fused path, state = the Stokes solution; five repeats of 100 calls)")
            emit(f"   fields off  {off.tolist()}  median {np.median(off):.4f}")
            emit(f"   TT          {tt.tolist()}  median {np.median(tt):.4f}   (time term sigma 30 theta 1600; what a body force runs)")
            emit(f"   EV          {ev.tolist()}  median {np.median(ev):.4f}   (the same term, mixture fields: viscosity ratio 4, buoyancy (0, -2, 0))")
            emit(f"   EV / TT: {np.median(ev) / np.median(tt):.3f}, TT / off: {np.median(tt) / np.median(off):.3f} (medians; recorded, not bounded)")
            if args.parent_times:
                runs = [json.load(open(f))["off"] for f in args.parent_times]
                p = np.array([x for r in runs for x in r])
                # the comparison with the parent uses this tree's fields-off runs that sit BETWEEN the parent's runs where there are
                # any (the per-process medians drift by a few % over a session, more than the spread inside one process)
                mine = [json.load(open(f))["off"] for f in args.bracketed] if args.bracketed else [off.tolist()]
                cmp_off = np.array([x for r in mine for x in r])
                if args.bracketed:
                    emit(f"   fields off, one process per list, each between two of the parent's runs  {mine}  median {np.median(cmp_off):.4f}")
                inside = p.min() <= np.median(cmp_off) <= p.max()
                emit(f"   parent commit, same session, one process per list (in the order given, this tree's runs in between)  {runs}  "
                     f"spread {p.min():.4f} .. {p.max():.4f}")
                emit(f"   fields-off median inside the parent's spread: {'yes' if inside else 'NO'}; fields off / parent (medians) {np.median(cmp_off) / np.median(p):.4f}")
            else:
                emit("   fields off against the parent commit: unmeasured (no --parent-times given)")
    if "B" in args.sections:
        if not gpu:
            emit("B  iteration counts of the coupled duct at viscosity ratios 1, 4, 20: unmeasured (no GPU)")
        else:
            sys.path.insert(0, ROOT)
            from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
            from stabilized_navier_stokes_flow_fenicsx_amd.drivers import inner_stream_inlet_data
            from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem, solve_coupled_flow
            m = M.duct_mesh(CELLS, LENGTH)
            P = FlowProblem(m, B.duct_bcs(m), reynolds=RE)
            U, sres = P.stokes_solve()
            emit(f"B  the same duct, Re {RE}, kappa {KAPPA}, default options, solver.solve_coupled_flow (rtol 1e-8) from the Stokes solution "
                 f"({sres.its} BiCGStab iterations); scalar Dirichlet data = drivers.inner_stream_inlet_data")
            for ratio in (1.0, 4.0, 20.0):
                _, _, recs = solve_coupled_flow(P, U, (KAPPA,), inner_stream_inlet_data(m), log_viscosity_ratio=float(np.log(ratio)))
                emit(f"   viscosity ratio {ratio:g}: {len(recs)} outer steps, {'converged' if recs[-1]['converged'] else 'NOT converged'}; Newton "
                     f"iterations {[r['newton_its'] for r in recs]}, BiCGStab iterations {[r['ksp_its'] for r in recs]}, scalar "
                     f"iterations {[r['scalar_its'] for r in recs]}; reasons Newton {[r['newton_reason'] for r in recs][-1]} scalar "
                     f"{[r['scalar_reason'] for r in recs][-1]}; last change {recs[-1]['change']}")
            emit("   The AMG hierarchy (aggregation, smoother damping) has NOT been tuned for the viscosity contrast.")
            P.close()
    fh.close()


if __name__ == "__main__":
    main()
