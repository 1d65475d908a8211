"""Writes profiles/resolvent.txt: the cost record of the resolvent analysis (k_energy_pass, k_forcing_scale; sns_energy_apply,
sns_lumped_volumes, sns_resolvent_lanczos; solver.resolvent_analysis).

  0  per kernel of the feature, the VGPR / SGPR / scratch / LDS / occupancy figures of the gfx950 compile
     (scripts/profile_hessian.py's reader); needs hipcc, no GPU
  1  bytes of one energy pass; arithmetic
  A  on an MI355X, at the 300 x 75 x 75 duct (10.1 M tets): ms of one sns_energy_apply (parts = 1 and 2) and one sns_lumped_volumes
     beside one sns_mass_apply -- warm-up, device-event timing, median and range of the repeats
  B  there, ONE step of the process composed from the public entry points in the order sns_resolvent_lanczos runs it, split into
     forward solve / adjoint solve / the two flips with their set-ups / the rest (S, the two pair mass passes as two single passes
     each, the energy pass), host clock around calls that end in a stream synchronise; the flips' share of the step
  C  there, solver.resolvent_analysis(n_modes=3, m=24) in total: wall time, inner iterations, gains
Without a GPU sections A to C say "not measured".

    python scripts/profile_resolvent.py [--cells 300 75 75] [--repeats 20] [--omega 1.0] [--m 24] [--steps 3] [--skip-analysis]
                                        [--resources-from FILE]
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
OUT = os.path.join(ROOT, "profiles", "resolvent.txt")
KERNELS = (("sns_resolvent.hip", "k_energy_pass"), ("sns_resolvent.hip", "k_forcing_scale"), ("sns_resolvent.hip", "k_velocity_mask"))


def _progress(what):
    print(f"[profile_resolvent] {what}", file=sys.stderr, flush=True)


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


def _fmt(ms):
    return f"{ms[0]:8.3f} ms ({ms[1]:.3f} .. {ms[2]:.3f})"


def time_passes(P, w, repeats):
    import torch
    x = torch.cos(0.3 * torch.arange(P.ndof, dtype=torch.float64, device=P.device))
    xp = torch.cat([x, torch.sin(0.7 * torch.arange(P.ndof, dtype=torch.float64, device=P.device))]).contiguous()
    y, yp = P.zeros(), torch.empty_like(xp)
    lib, h = P.lib, P.h
    ptr = lambda v: v.data_ptr()

    def energy(parts):
        assert lib.sns_energy_apply(h, None, parts, ptr(xp if parts == 2 else x), ptr(yp if parts == 2 else y)) == 0

    def lumped():
        assert lib.sns_lumped_volumes(h, ptr(y)) == 0

    def mass():
        assert lib.sns_mass_apply(h, ptr(w), ptr(x), ptr(y)) == 0

    e1, e2, lm, ms = (_event_ms(lambda: energy(1), repeats), _event_ms(lambda: energy(2), repeats), _event_ms(lumped, repeats),
                      _event_ms(mass, repeats))
    return [f"   sns_energy_apply, parts = 1                 {_fmt(e1)}",
            f"   sns_energy_apply, parts = 2                 {_fmt(e2)}",
            f"   sns_lumped_volumes                          {_fmt(lm)}",
            f"   sns_mass_apply (the pass it is built like)  {_fmt(ms)}"]


def time_step(P, S, w, omega, steps):
    """`steps` steps of the process by hand from the public entry points; the split of the last ones (the first warms up)."""
    import torch

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def cmass(v, transpose=False):
        op = P.mass_apply_transpose if transpose else P.mass_apply
        return torch.complex(op(w, v.real.contiguous()).clone(), op(w, v.imag.contiguous()).clone())

    ml = P.lumped_volumes()
    free = ~torch.from_numpy(P.bc_mask.astype(bool)).to(P.device) & (ml > 0.0)
    s = torch.where(free, 1.0 / torch.sqrt(torch.where(free, ml, torch.ones_like(ml))), torch.zeros_like(ml))
    v = (s > 0.0) * torch.cos(1.0 + 0.37 * torch.arange(P.ndof, dtype=torch.float64, device=P.device))
    v = torch.complex(v / v.norm(), torch.zeros_like(v))
    P.jacobian(w)
    P.pc_setup()
    rows = []
    for step in range(steps):
        b, t_rest = clocked(lambda: cmass(s * v))
        (q, kf), t_fwd = clocked(lambda: P.shifted_solve(w, 1j * omega, b))
        r, t_e = clocked(lambda: P.energy_apply(q))
        _, t_flip1 = clocked(lambda: (P.transpose_operator(), P.pc_setup()))
        (y, ka), t_adj = clocked(lambda: P.shifted_solve(w, -1j * omega, r, transpose=True))
        _, t_flip2 = clocked(lambda: (P.transpose_operator(), P.pc_setup()))
        u, t_rest2 = clocked(lambda: s * cmass(y, transpose=True))
        gain2 = float(torch.vdot(v, u).real)
        v = u / u.norm()
        rows.append((t_fwd, t_adj, t_flip1 + t_flip2, t_rest + t_e + t_rest2, kf.its, ka.its, kf.reason, ka.reason, gain2))
        _progress(f"step {step} done")
    L = ["   step: forward solve s (its, reason) | adjoint solve s (its, reason) | two flips + set-ups s | rest s | flips' share | v^H T v"]
    for k, (tf, ta, tfl, tr, kf, ka, rf, ra, g2) in enumerate(rows):
        tot = tf + ta + tfl + tr
        L.append(f"   {k}: {tf:7.3f} ({kf}, {rf}) | {ta:7.3f} ({ka}, {ra}) | {tfl:7.3f} | {tr:7.3f} | {100.0 * tfl / tot:5.1f} % of {tot:.3f} s | {g2:.6e}"
                 + ("   (first step: warm-up, the transpose's partner table is built here)" if k == 0 else ""))
    return L


def time_analysis(P, S, w, omega, m):
    import torch
    P.reset_timings()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = S.resolvent_analysis(P, w, omega, n_modes=3, m=m)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    return [f"   wall {sec:.2f} s; m_done {r.m_done}, reason {r.reason}, {r.ksp_its} inner iterations over {2 * r.m_done + len(r.gains)} solves; gains "
            f"{', '.join(f'{g:.6e}' for g in r.gains)}; estimates / sigma_1^2 {', '.join(f'{e / max(r.gains[0] ** 2, 1e-300):.1e}' for e in r.residuals)}; "
            f"converged {r.converged.tolist()}; the handle's Krylov timer {P.timings().krylov_ms / 1e3:.2f} s"]


def measure(a):
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B
    from stabilized_navier_stokes_flow_fenicsx_amd import mesh as M
    from stabilized_navier_stokes_flow_fenicsx_amd import solver as S
    msh = M.duct_mesh(tuple(a.cells), 4.0)
    P = S.FlowProblem(msh, B.duct_bcs(msh).flatten(), reynolds=100.0, gmres_restart=30)
    U, _ = P.stokes_solve()
    w, rn = P.newton_solve(U.clone())
    _progress("duct: Newton done")
    head = [f"   duct {a.cells[0]} x {a.cells[1]} x {a.cells[2]}, {msh.num_nodes} nodes, {msh.num_tets} tets, ndof {msh.num_dofs}; state: Newton from the "
            f"Stokes solution at Re 100, {rn.its} iterations, reason {rn.reason}; gmres_restart 30; omega {a.omega}"]
    A_sec = head + [f"   3 warm-up calls, device events around each call, median (min .. max) of {a.repeats}"] + time_passes(P, w, a.repeats)
    _progress("passes done")
    P.set_options(ksp_rtol=1e-10)
    B_sec = time_step(P, S, w, a.omega, a.steps)
    P.set_options(ksp_rtol=1e-8)
    C_sec = None if a.skip_analysis else time_analysis(P, S, w, a.omega, a.m)
    P.close()
    return A_sec, B_sec, C_sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[300, 75, 75])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--omega", type=float, default=1.0)
    ap.add_argument("--m", type=int, default=24)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-analysis", action="store_true")
    ap.add_argument("--resources-from", default=None, help="an earlier record whose section 0 is kept instead of compiling")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from profile_hessian import resource_usage
    L = ["Resolvent analysis (sns_energy_apply, sns_lumped_volumes, sns_resolvent_lanczos; solver.resolvent_analysis): resource usage and cost",
         "=" * 98,
         "0  Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no GPU needed) -- from the compile, not measured"]
    if a.resources_from and os.path.exists(a.resources_from):
        old = open(a.resources_from).read().splitlines()
        start = next(i for i, ln in enumerate(old) if ln.startswith("0  "))
        L += old[start + 1:next(i for i, ln in enumerate(old) if ln.startswith("1  "))]
    else:
        scratch = 0
        for unit in sorted({u for u, _ in KERNELS}):
            for r in resource_usage(unit):
                if any(u == unit and k in r["name"] for u, k in KERNELS):
                    L.append("   %-52s %s" % (r["name"], {k: v for k, v in r.items() if k != "name"}))
                    scratch = max(scratch, r.get("ScratchSize", 0))
        L.append(f"   scratch over the kernels of the feature: {scratch} bytes/lane" + ("" if scratch == 0 else "   NON-ZERO: a kernel spills"))
    L.append("1  Bytes -- arithmetic, not measured")
    L.append("   one energy pass reads per (node, cell) pair the cell's 4 node ids, 12 coordinates, 4 mask words and 12 velocity entries per part "
             "(through the caches: a node is shared by some 24 cells) and writes 4 doubles per node and part; it reads neither w nor the operator")
    import torch
    gpu = torch.cuda.is_available()
    if gpu:
        A_sec, B_sec, C_sec = measure(a)
        name = torch.cuda.get_device_name(0)
        L.append(f"A  MEASURED on {name}: the energy pass alone")
        L += A_sec
        L.append(f"B  MEASURED there: {a.steps} steps of the process composed from the public entry points (ksp_rtol 1e-10), host clock around calls "
                 "that end in a stream synchronise; sns_resolvent_lanczos runs the same solves, flips and set-ups, and pair passes where this "
                 "composition runs two single passes")
        L += B_sec
        if C_sec is None:
            L.append(f"C  solver.resolvent_analysis(n_modes=3, m={a.m}) in total: not measured (skipped)")
        else:
            L.append(f"C  MEASURED there: solver.resolvent_analysis(n_modes=3, m={a.m}, omega={a.omega}, ksp_rtol=1e-10), one run, host timer around the call")
            L += C_sec
    else:
        why = " (no GPU where this file was written)"
        L.append("A  one sns_energy_apply (parts = 1, 2) and one sns_lumped_volumes beside sns_mass_apply at the 300 x 75 x 75 duct: not measured" + why)
        L.append("B  one step of the process split into forward solve / adjoint solve / the two flips with their set-ups / the rest, and the "
                 "flips' share of the step: not measured" + why)
        L.append("C  solver.resolvent_analysis(n_modes=3, m=24) there in total: not measured" + why)
    L.append("D  bench.py's headline line against the parent commit: not measured here (the benchmark's path -- Newton, BiCGStab, the V-cycle -- "
             "runs no code of this feature)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
