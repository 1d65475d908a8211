"""Viscosity law (sns_set_viscosity_law): the records of profiles/viscosity_law.txt.

  0  resource usage (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; no GPU needed) of every law-on instantiation
     of csrc/sns_kernels.hip beside its law-off counterpart, and -- with --parent DIR, the csrc directory of a checkout of
     the parent commit -- the law-off kernels' figures against the parent's
  A  on the (100, 25, 25) duct, state = the Stokes solution: ms per sns_bench_assemble call (Jacobian + residual), three
     repeats each, law off and law on; with --parent-times FILE... (each written by `--times-only FILE --tree PARENT_CHECKOUT`
     in the same session, before and after a `--times-only` run of this tree given as --bracketed) the law-off time against
     the parent's own spread
  B  Newton / BiCGStab iteration counts on that duct from the Stokes start, Newtonian against law-on

    python scripts/profile_viscosity.py [--out FILE] [--sections 0AB] [--parent DIR] [--parent-times FILE...] [--bracketed FILE] [--measured FILE]
    python scripts/profile_viscosity.py --times-only FILE [--tree DIR]

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
CELLS, LENGTH, RE, LAW = (100, 25, 25), 4.0, 10.0, (3.0, 0.5, 0.01)
KEYS = ("VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS Size")


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


def assemble_times(tree, law, repeats=3, reps=10):
    """ms per sns_bench_assemble call, ``repeats`` times, with the package of ``tree``."""
    sys.path.insert(0, tree)
    import torch  # noqa: F401
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    m = M.duct_mesh(CELLS, LENGTH)
    P = FlowProblem(m, B.duct_bcs(m), reynolds=RE)
    U, _ = P.stokes_solve()
    out = {}
    for name in (("off", "on") if law else ("off",)):
        if name == "on":
            P.set_viscosity_law(*LAW)
        P.bench_assemble(U, "ns", reps=3)                                  # warm-up
        out[name] = [P.bench_assemble(U, "ns", reps=reps) for _ in range(repeats)]
    P.close()
    return out, m.num_tets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viscosity_law.txt"))
    ap.add_argument("--sections", default="0AB")
    ap.add_argument("--parent", default=None, help="csrc directory of a checkout of the parent commit")
    ap.add_argument("--parent-times", default=None, nargs="+", help="one file per run of --times-only on the parent")
    ap.add_argument("--bracketed", default=None, help="--times-only run of THIS tree made between the parent's runs")
    ap.add_argument("--measured", default=None)
    ap.add_argument("--times-only", default=None)
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.times_only:
        t, nt = assemble_times(args.tree, law=False)
        json.dump(dict(off=t["off"], tets=nt), open(args.times_only, "w"))
        print(t)
        return
    fh = open(args.out, "w")

    def emit(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    if "0" in args.sections:
        emit("Viscosity law (sns_set_viscosity_law): resource usage and measurements")
        emit("=" * 78)
        new = resource_usage(os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc"))
        emit("0  Resource usage of csrc/sns_kernels.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
        emit("   template arguments: k_element / k_fused_* <form, corrected convection, time term, viscosity law>, k_residual_tet without the form")
        emit(f"   {'kernel':52s} {'VGPRs':>5s} {'AGPRs':>5s} {'scratch':>7s} {'occ':>3s} {'LDS':>6s}")
        bad = []
        for k, v in new.items():
            if not re.search(r", true>$", k) or "k_element_viscosity" in k:
                continue
            off = re.sub(r", true>$", ", false>", k)
            for name in (off, k):
                r = new[name]
                emit(f"   {name:52s} {r.get('VGPRs', 0):5d} {r.get('AGPRs', 0):5d} {r.get('ScratchSize', 0):7d} {r.get('Occupancy', 0):3d} {r.get('LDS Size', 0):6d}")
            if v.get("ScratchSize", 0) > 0 and new[off].get("ScratchSize", 0) == 0:
                bad.append(k)
        for k in ("k_element_viscosity<false>", "k_element_viscosity<true>"):
            r = new[k]
            emit(f"   {k:52s} {r.get('VGPRs', 0):5d} {r.get('AGPRs', 0):5d} {r.get('ScratchSize', 0):7d} {r.get('Occupancy', 0):3d} {r.get('LDS Size', 0):6d}")
        emit(f"   law-on instantiations with scratch where the counterpart has none: {len(bad)} {bad if bad else ''}")
        if args.parent:
            old = resource_usage(args.parent)
            same = diff = 0
            for k, v in old.items():
                kk = re.sub(r">$", ", false>", k) if re.match(r"k_(element|fused_\w+|residual_tet)<", k) else k
                if new.get(kk) == v:
                    same += 1
                else:
                    diff += 1
                    emit(f"   DIFFERS {k}: parent {v} this tree {new.get(kk)}")
            emit(f"   kernels of the parent's sns_kernels.hip: {same + diff}; identical VGPR / AGPR / scratch / occupancy / LDS figures in this "
                 f"tree (law-off instantiation where there is one): {same}; different: {diff}")
        else:
            emit("   law-off figures against the parent commit: unmeasured (no --parent checkout given)")
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
            emit("A  sns_bench_assemble on the (100, 25, 25) duct, law off / law on / parent: unmeasured (no GPU)")
        else:
            t, nt = assemble_times(ROOT, law=True)
            off, on = np.array(t["off"]), np.array(t["on"])
            emit(f"A  {nt} tets, ms per sns_bench_assemble call (Jacobian + residual, fused path, state = the Stokes solution; three repeats of 10 calls)")
            emit(f"   law off  {off.tolist()}  median {np.median(off):.4f}")
            emit(f"   law on   {on.tolist()}  median {np.median(on):.4f}   (Carreau lambda {LAW[0]} n {LAW[1]} ratio {LAW[2]})")
            emit(f"   law on / law off: {np.median(on) / np.median(off):.3f} (medians); spread law off {off.min():.4f} .. {off.max():.4f}, law on {on.min():.4f} .. {on.max():.4f}")
            if args.parent_times:
                runs = [json.load(open(f))["off"] for f in args.parent_times]
                p = np.array([t for r in runs for t in r])
                # the comparison with the parent uses this tree's law-off run that sits BETWEEN the parent's runs where there is
                # one (the per-process medians drift by a few % over a session, more than the spread inside one process)
                cmp_off = np.array(json.load(open(args.bracketed))["off"]) if args.bracketed else off
                if args.bracketed:
                    emit(f"   law off, process between the parent's runs  {cmp_off.tolist()}  median {np.median(cmp_off):.4f}")
                inside = p.min() <= np.median(cmp_off) <= p.max()
                emit(f"   parent commit, same session, one process per list (in the order given, this tree's run in between)  {runs}  "
                     f"spread {p.min():.4f} .. {p.max():.4f}")
                emit(f"   law-off median inside the parent's spread: {'yes' if inside else 'NO'}; law off / parent (medians) {np.median(cmp_off) / np.median(p):.4f}")
            else:
                emit("   law off against the parent commit: unmeasured (no --parent-times given)")
    if "B" in args.sections:
        if not gpu:
            emit("B  Newton / BiCGStab iteration counts, Newtonian against law-on: unmeasured (no GPU)")
        else:
            sys.path.insert(0, ROOT)
            from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
            from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
            m = M.duct_mesh(CELLS, LENGTH)
            P = FlowProblem(m, B.duct_bcs(m), reynolds=RE)
            U, sres = P.stokes_solve()
            emit(f"B  the same duct, Re {RE}, default options, Newton from the Stokes solution ({sres.its} BiCGStab iterations)")
            _, r = P.newton_solve(U.clone())
            emit(f"   Newtonian: SNES reason {r.reason}, {r.its} Newton iterations, {r.ksp_its} BiCGStab iterations in all")
            P.set_viscosity_law(*LAW)
            w, r = P.newton_solve(U.clone())
            nu, _ = P.element_viscosity(w)
            emit(f"   law on (lambda {LAW[0]} n {LAW[1]} ratio {LAW[2]}): SNES reason {r.reason}, {r.its} Newton iterations, {r.ksp_its} BiCGStab iterations "
                 f"in all; nu_e / nu0 between {float(nu.min()) * RE:.4f} and {float(nu.max()) * RE:.4f}")
            emit(f"   The AMG hierarchy (aggregation, smoother damping) has NOT been tuned for a viscosity contrast of 1/r = {1.0 / LAW[2]:g}.")
            P.close()
    fh.close()


if __name__ == "__main__":
    main()
