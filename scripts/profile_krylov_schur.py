"""Writes profiles/krylov_schur.txt: the cost record of the thick-restarted stability analysis (k_basis_rotate, sns_basis_rotate,
sns_stability_arnoldi_extend, solver.linear_stability(max_restarts > 0)).

  0  per instance of k_basis_rotate, the VGPR / SGPR / scratch / LDS / occupancy figures of the gfx950 compile
     (scripts/profile_stability.py's reader); needs hipcc, no GPU
  1  bytes one restart moves through k_basis_rotate as a function of (m, ndof), and the memory of the basis at m = 64 against
     m = 16 on the bench mesh and on the meshes the README names; arithmetic, no GPU
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets): ms of one sns_basis_rotate at (n_in, n_out) = (17, 9), (33, 17),
     (65, 33) -- warm-up, device-event timing, median and range of the repeats -- beside the bytes it moves
  B  there, linear_stability(n_modes=6, m=16, max_restarts=20) against linear_stability(m=64): wall time, Krylov iterations,
     restarts, converged modes, and what one restart's re-assembly and set-up cost (the handle's timers)
Without a GPU sections A and B say "not measured".

    python scripts/profile_krylov_schur.py [--cells 300 75 75] [--repeats 20] [--skip-duct]
"""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "profiles", "krylov_schur.txt")

# (name, nodes): the bench mesh (bench.py's default duct) and the meshes the README advertises
MESHES = (("300 x 75 x 75 duct, 10.1 M tets", 301 * 76 * 76), ("81 M tets, about", 13_900_000), ("192 M tets, about", 33_200_000))


def _progress(what):
    print(f"[profile_krylov_schur] {what}", file=sys.stderr, flush=True)


def rotate_bytes(n_in, ndof):
    """k_basis_rotate reads n_in columns and writes n_in columns (n_out outputs, n_in - n_out zeroed) of ndof doubles."""
    return 2 * n_in * ndof * 8


def _event_ms(fn, repeats):
    import torch
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
    return statistics.median(ts), min(ts), max(ts)


def measure_duct(cells, repeats):
    import numpy as np
    import torch
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    m = M.duct_mesh(tuple(cells), 4.0)
    P = S.FlowProblem(m, B.duct_bcs(m).flatten(), reynolds=100.0)
    _progress("duct problem built")
    U, _ = P.stokes_solve()
    w, rn = P.newton_solve(U.clone())
    _progress("Newton done")
    A_sec = [f"   duct {cells[0]} x {cells[1]} x {cells[2]}, {m.num_nodes} nodes, {m.num_tets} tets, ndof {m.num_dofs}; state: Newton from the "
             f"Stokes solution at Re 100, {rn.its} iterations, reason {rn.reason}",
             f"   3 warm-up calls, device events around each call (host copy of Q, launch, stream sync), median (min .. max) of {repeats}"]
    rng = np.random.default_rng(0)
    for n_in, n_out in ((17, 9), (33, 17), (65, 33)):
        V = torch.from_numpy(rng.standard_normal((n_in, 8))).cuda().repeat_interleave((m.num_dofs + 7) // 8, dim=1)[:, :m.num_dofs].contiguous()
        Q, _ = np.linalg.qr(rng.standard_normal((n_in, n_in)))
        Q = np.ascontiguousarray(Q[:, :n_out])
        ms = _event_ms(lambda: P.lib.sns_basis_rotate(P.h, n_in, n_out, Q.ctypes.data, V.data_ptr()), repeats)
        gb = rotate_bytes(n_in, m.num_dofs) / 1e9
        A_sec.append(f"   sns_basis_rotate ({n_in:2d}, {n_out:2d})  {ms[0]:9.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f}); {gb:.2f} GB moved: {gb / ms[0] * 1e3:.0f} GB/s")
        del V
    _progress("rotations timed")
    B_sec = []
    for kw in (dict(m=64), dict(m=16, max_restarts=20)):
        P.reset_timings()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = S.linear_stability(P, w, n_modes=6, shift=0.0, **kw)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        tm = P.timings()
        _progress(f"linear_stability {kw} done")
        B_sec.append(f"   {kw}: wall {sec:.2f} s; m_done {r.m_done}, reason {r.reason}, restarts {r.restarts}, {r.ksp_its} Krylov iterations; "
                     f"{int(r.converged.sum())} of {len(r.converged)} modes converged; basis {(kw['m'] + 1) * m.num_dofs * 8 / 1e9:.2f} GB; the handle's "
                     f"timers: Krylov {tm.krylov_ms / 1e3:.2f} s, assembly {tm.assemble_ms / 1e3:.2f} s, set-up {tm.pc_setup_ms / 1e3:.2f} s")
    P.close()
    return A_sec, B_sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-duct", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from profile_stability import resource_usage
    L = ["Thick-restarted (Krylov-Schur) stability analysis (sns_basis_rotate, sns_stability_arnoldi_extend, linear_stability(max_restarts > 0)): resource usage and cost",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    rows = [r for r in resource_usage() if "k_basis_rotate" in r["name"]]
    for r in rows:
        L.append("   %-40s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
    scratch = max(r.get("ScratchSize", 0) for r in rows)
    L.append(f"   scratch of k_basis_rotate: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: the row spills"))
    L.append("   LDS: dynamic, n_in x n_out doubles per block -- (17, 9) 1.2 KB, (33, 17) 4.5 KB, (65, 33) 17.2 KB, (65, 65) 33.8 KB at most -- "
             "so the static figure above is 0; the row of NMAX doubles is 2 NMAX VGPRs, every index a compile-time constant")
    import torch
    gpu = torch.cuda.is_available() and not a.skip_duct
    L.append("   its time: section A" if gpu else "   its time is NOT MEASURED until this script runs on hardware (section A)")
    L.append("1  Bytes and memory -- arithmetic, not measured")
    L.append("   one restart: k_basis_rotate reads (m + 1) ndof 8 B and writes as many (k + 1 outputs, m - k zeroed columns): 16 (m + 1) ndof B, "
             "once between m - keep inner solves")
    for name, nodes in MESHES:
        ndof = 4 * nodes
        L.append(f"   {name} ({nodes / 1e6:.1f} M nodes, ndof {ndof / 1e6:.1f} M): basis per side {65 * ndof * 8 / 1e9:6.2f} GB at m = 64, "
                 f"{17 * ndof * 8 / 1e9:6.2f} GB at m = 16 (x {65 / 17:.2f} less); one restart moves {rotate_bytes(17, ndof) / 1e9:.2f} GB at m = 16, "
                 f"{rotate_bytes(65, ndof) / 1e9:.2f} GB at m = 64")
    L.append("   per restart the entry point also re-assembles J + shift B and sets the hierarchy up again (stateless per call): about "
             "7.6 + 5 ms against about 125 ms per inner solve on the 10 M-tet duct by the README's figures -- " +
             ("for this path: the assembly and set-up timers of section B over restarts + 1 calls" if gpu else "not measured for this path"))
    if gpu:
        A_sec, B_sec = measure_duct(a.cells, a.repeats)
        L.append(f"A  MEASURED on {torch.cuda.get_device_name(0)}: one sns_basis_rotate")
        L += A_sec
        L.append("B  MEASURED there: linear_stability(n_modes=6, shift=0, ksp_rtol=1e-10), one run each, host timer around the call")
        L += B_sec
    else:
        why = " (no GPU where this file was written)" if not torch.cuda.is_available() else " (skipped)"
        L.append("A  one sns_basis_rotate at the 300 x 75 x 75 duct: not measured" + why)
        L.append("B  linear_stability(m=16, max_restarts=20) against linear_stability(m=64) there: not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
