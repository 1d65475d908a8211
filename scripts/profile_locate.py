"""Device point location (sns_locate_points) and P1 evaluation (sns_eval_p1) against the host's interpolate.locate_points:
the nodes of a duct mesh twice as fine located on a duct mesh, three sizes.

  build   sns_locate_points with ONE query point: bounds, bucket grid (count / scan / fill / sort) and the scratch memory
  locate  the same call with all query points, minus `build`
  eval    sns_eval_p1, ncomp = 4 (the [ux, uy, uz, p] records of a solution)
Device times: host clock around calls that end in a stream synchronise, median of 5 after a warm-up; the mesh and the
points are already on the device.  The host column is one call of locate_points on the same arrays; it is skipped above
1 M source tets (1.3 M tets x 1.7 M points would take about a minute and several GB of temporaries there).

    python scripts/profile_locate.py [--out profiles/locate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = [((60, 15, 15), (120, 30, 30)), ((120, 30, 30), (240, 60, 60)), ((150, 38, 38), (300, 75, 75))]
HOST_MAX_TETS = 1_000_000


def _median(f, reps=5):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import interpolate as IP, mesh as M
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; times in ms (device: median of 5), host: interpolate.locate_points, one call",
             f"{'source tets':>12} {'query pts':>10} {'build':>8} {'locate':>8} {'eval4':>7} {'device':>8} {'host':>9} "
             f"{'speed-up':>8}  same tets / max |lambda diff|"]
    print(lines[0], "\n" + lines[1], flush=True)
    IP.locate_points(M.duct_mesh((4, 2, 2)), np.zeros((1, 3)), device=dev)
    for cs, cf in PAIRS:
        src, fine = M.duct_mesh(cs), M.duct_mesh(cf)
        dm = IP._DeviceMesh(src, dev)
        q = IP._dev_array(fine.points, dev)
        vals = torch.randn((src.num_nodes, 4), dtype=torch.float64, device=dev)
        IP.locate_points_device(dm, q, 1e-6)
        t_build, _ = _median(lambda: IP.locate_points_device(dm, q[:1], 1e-6))
        t_all, (tet, lam, nmiss) = _median(lambda: IP.locate_points_device(dm, q, 1e-6))
        t_eval, _ = _median(lambda: IP.eval_p1_device(dm, vals, tet, lam))
        if src.num_tets <= HOST_MAX_TETS:
            t0 = time.perf_counter()
            th, lh = IP.locate_points(src, fine.points)
            t_host = time.perf_counter() - t0
            td = tet.cpu().numpy()
            same = f"{(td == th).mean():.6f} / {np.abs(lam.cpu().numpy() - lh).max():.1e}"
            host, sp = f"{1e3 * t_host:9.0f}", f"{t_host / t_all:7.0f}x"
        else:
            host, sp, same = f"{'skipped':>9}", f"{'-':>8}", f"(host skipped above {HOST_MAX_TETS} tets)"
        ln = (f"{src.num_tets:>12} {fine.num_nodes:>10} {1e3 * t_build:8.2f} {1e3 * (t_all - t_build):8.2f} {1e3 * t_eval:7.2f} "
              f"{1e3 * t_all:8.2f} {host} {sp}  {same}; missed {nmiss}")
        print(ln, flush=True)
        lines.append(ln)
        del dm, q, vals, tet, lam
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
