"""Shape gradient (sns_residual_shape_gradient, csrc/sns_shape.hip): the records of profiles/shape_gradient.txt.

  0  resource usage (hipcc -Rpass-analysis=kernel-resource-usage for gfx950; no GPU needed): every kernel of every HIP unit of
     this tree against the same compile of a parent checkout (--parent DIR, the csrc directory of the parent commit; without
     it only this tree's new kernels are listed), and the new kernels' registers / scratch / LDS
  A  on the headline mesh of bench.py (300 x 75 x 75 cells, Re 200, state = the Stokes solution): the time of one
     sns_residual_shape_gradient call beside the time of one sns_residual call, measured in the same run (wall clock around
     `reps` synchronous calls after a warm-up, median of 5 rounds, the two alternated), and their ratio
  B  kernel against oracle on the connected test meshes, and the oracle against itself on the same cells in a second
     cyclic vertex order (the oracle's own rounding)

    python scripts/profile_shape.py [--out FILE] [--sections 0AB] [--parent DIR] [--cells 300,75,75]

Sections A and B need a GPU; without one they are written as "unmeasured".
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
CSRC = os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc")
KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size")


def resource_usage(csrc):
    """{unit: {demangled kernel: {key: value}}} of every .hip unit under ``csrc``."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    from concurrent.futures import ThreadPoolExecutor

    def one(src):
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
               "-I" + os.path.join(csrc, "..", "..", "include"), "-I" + csrc, "-Wno-unused-result", "-c", src, "-o", os.devnull,
               "-Rpass-analysis=kernel-resource-usage"]
        err = subprocess.run(cmd, capture_output=True, text=True).stderr
        names = re.findall(r"Function Name: (\S+)", err)
        dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n") if names else []
        rows, cur, i = {}, None, 0
        for ln in err.splitlines():
            if "Function Name:" in ln:
                cur = dem[i]
                i += 1
                rows[cur] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
            if m and cur and m.group(1).strip() in KEYS:
                rows[cur][m.group(1).strip()] = int(m.group(2))
        return os.path.basename(src), rows

    with ThreadPoolExecutor(8) as ex:
        return dict(ex.map(one, sorted(glob.glob(os.path.join(csrc, "*.hip")))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_gradient.txt"))
    ap.add_argument("--sections", default="0AB")
    ap.add_argument("--parent", default=None, help="csrc directory of a checkout of the parent commit")
    ap.add_argument("--cells", default="300,75,75")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    fh = open(args.out, "w")

    def emit(s=""):
        print(s, flush=True)
        fh.write(s + "\n")
        fh.flush()

    emit("Shape gradient (sns_residual_shape_gradient): resource usage and measurements")
    emit("=" * 78)
    if "0" in args.sections:
        new = resource_usage(CSRC)
        emit("0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed)")
        if args.parent:
            old = resource_usage(args.parent)
            n_same = n_diff = 0
            for unit, rows in old.items():
                for k, v in rows.items():
                    if new.get(unit, {}).get(k) == v:
                        n_same += 1
                    else:
                        n_diff += 1
                        emit(f"   DIFFERS {unit} {k}: parent {v} this tree {new.get(unit, {}).get(k)}")
            emit(f"   kernels present in the parent and in this tree: {n_same + n_diff}; identical VGPR / AGPR / SGPR / scratch / occupancy / "
                 f"LDS figures: {n_same}; different: {n_diff}")
        emit("   new kernels (csrc/sns_shape.hip); template arguments of k_shape_tet: <corrected convection, time term>")
        for k, v in new["sns_shape.hip"].items():
            emit(f"   {re.sub(r'[(].*', '', k):40s} {v}")
        emit(f"   scratch of the new kernels: {max(v.get('ScratchSize', 0) for v in new['sns_shape.hip'].values())} bytes/lane")
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    if "A" in args.sections:
        if not gpu:
            emit("A  time of one sns_residual_shape_gradient call beside one sns_residual call on the headline mesh: unmeasured (no GPU)")
            emit("   sns_residual: unmeasured   sns_residual_shape_gradient: unmeasured   ratio: unmeasured")
        else:
            from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
            from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
            m = M.duct_mesh(tuple(int(c) for c in args.cells.split(",")), 4.0)
            P = FlowProblem(m, B.duct_bcs(m), reynolds=200.0)
            U, _ = P.stokes_solve()
            lam = torch.randn_like(U)
            F = P.zeros()

            def t_of(fn):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / args.reps * 1e3

            tr, ts = [], []
            for _ in range(5):
                tr.append(t_of(lambda: P.residual(U, "ns", out=F)))
                ts.append(t_of(lambda: P.residual_shape_gradient(U, lam)))
            tr, ts = np.array(tr), np.array(ts)
            emit(f"A  {m.num_tets} tets, ms per call (wall clock, {args.reps} synchronous calls after a warm-up, median of 5 alternated rounds)")
            emit(f"   sns_residual {np.median(tr):.3f} ({tr.min():.3f} .. {tr.max():.3f})   sns_residual_shape_gradient {np.median(ts):.3f} "
                 f"({ts.min():.3f} .. {ts.max():.3f})   ratio {np.median(ts) / np.median(tr):.3f}")
            P.close()
    if "B" in args.sections:
        if not gpu:
            emit("B  kernel against oracle, oracle against itself in a second vertex order: unmeasured (no GPU)")
        else:
            import shape_oracle as SO
            import torch
            from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
            from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
            m = M.duct_mesh((4, 3, 3), 2.0, jitter=0.2)
            rng = np.random.default_rng(24)
            w, lam = rng.standard_normal(m.num_dofs), rng.standard_normal(m.num_dofs)
            P = FlowProblem(m, B.duct_bcs(m), reynolds=25.0)
            got = P.residual_shape_gradient(torch.from_numpy(w).cuda(), torch.from_numpy(lam).cuda()).cpu().numpy()
            P.close()
            ref = SO.gradient_3d(m.points, m.tets, w, lam, 25.0)
            ref2 = SO.gradient_3d(m.points, np.ascontiguousarray(m.tets[:, [1, 2, 0, 3]]), w, lam, 25.0)
            s = np.abs(ref).max()
            emit(f"B  jittered duct (4, 3, 3): |kernel - oracle|max / |oracle|max {np.abs(got - ref).max() / s:.2e}; oracle in a second "
                 f"cyclic vertex order against itself {np.abs(ref2 - ref).max() / s:.2e}")
    fh.close()


if __name__ == "__main__":
    main()
