#!/usr/bin/env python
"""Headline benchmark: Newton iterations of the stabilised P1-P1 Navier-Stokes solve
on the 10.1 M-tet square duct (BASELINE.json configs[4], the configuration the metric
is quoted on; it fits one MI355X), Re = 200.

A "step" is ONE Newton iteration of a real Newton sequence started from the Stokes
solution: fused Jacobian+residual assembly (HIP), AMG setup, BiCGStab solve to rtol 1e-8
(the reference's KSP tolerance, NavierStokesChannelFlow.py:283), bt line-search residual.
When the sequence converges (||F|| < 1e-8, :281) it restarts from the Stokes solution.
metric = M-DOF/s = N_dof / (t_assemble + t_solve) per Newton iteration / 1e6  (SURVEY 8d).

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
A plain run does only what the headline needs: set-up, W + K Newton steps, the outputs of --dump-outputs and the JSON line.
--full adds what takes runs of its own: the all-fp64 repetition of the timed steps (all_f64_preconditioner), the assembly
kernels timed alone (roofline.assembly_kernels), the CPU baseline of the same step (cpu_baseline) and, for N>1, the weak layout.
N>1: `python bench.py --gpus N` started as a plain command launches its own N ranks (one per GPU, torch.distributed.run
on 127.0.0.1), relays rank 0's JSON line and exits with the workers' return code; started under an external
torch.distributed.run (the driver's way) it runs as the rank it is given.  WORLD_SIZE != --gpus is an error.
The HEADLINE is what north_star states -- the SAME 10.1 M-tet duct element-partitioned into N x-slabs (strong
scaling; every rank meshes only its own slab), halo exchange and dot-product all-reduces on RCCL inside libsns.so.
With --full the weak layout (duct refined by N^(1/3) per direction, every GPU keeps a ~10.1 M-tet slab) is timed afterwards and
reported under "weak_scaling" in the same JSON line (--no-weak skips it).
--config 3 / 4 / 4u time the other full-size BASELINE configs as secondary lines; the default (5) is the headline.
--dry-run: the launch + partition + halo-plan + collective path WITHOUT any HIP call (gloo on the CPU): what the
CPU test-suite runs with --gpus 2.
Environment: SNS_NO_OVERLAP=1 = exchange-then-full-pass instead of the overlapped interior/boundary split (the
fallback if the overlapped RCCL path misbehaves on a new machine); SNS_WATCHDOG_S = seconds without progress after
which a rank exits non-zero (default 900; 0 = off).
"""
import argparse
import glob
import json
import os
import socket
import subprocess
import sys
import threading
import time


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=str, default="5", choices=["3", "4", "4b", "4u", "5"],
                    help="BASELINE config: 5 = 10.1 M-tet duct Re 200 (headline), 3 = 55^3 cavity Re 100, "
                         "4 = 240x60x60 channel Re 50 with the inlet profiles of the reference's Plus image "
                         "(--inlet analytic: the two-stream substitute of round 2), 4b = the same image on the BODY-FITTED nozzle "
                         "channel of nozzle_mesh.py (--cells = 1000 x channel_mesh_size, default 20 -> lc 0.020, 4.66 M tets), "
                         "4u = Delaunay channel (~5 M tets)")
    ap.add_argument("--inlet", type=str, default="image", choices=["image", "analytic"],
                    help="config 4: inlet data from tests/golden/inlet_PlusF_final.png (default) or analytic")
    ap.add_argument("--cells", type=str, default=None)
    ap.add_argument("--length", type=float, default=4.0, help="duct length")
    ap.add_argument("--re", type=float, default=None)
    ap.add_argument("--ksp", type=str, default="bicgstab")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run what takes runs of its own: the all-fp64 repetition of the timed steps, "
                         "the assembly kernels timed alone, the CPU baseline and (N>1) the weak layout")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--cpu-maxit", type=int, default=1500,
                    help="iteration bound of the CPU baseline's Krylov solve (the 10.1 M-tet headline workload stops by "
                         "its own criterion after ~740 tfqmr iterations = ~100 s on 16 cores)")
    ap.add_argument("--no-f64-rerun", action="store_true", help="--full: skip the all-fp64 repetition of the timed steps")
    ap.add_argument("--budget", type=float, default=540.0,
                    help="N>1: wall-clock seconds the whole run of a rank may take (the driver gives the bench 600 s): the secondary legs "
                         "(peer-window transport, weak layout) share what is left of it after the headline -- each at most its own "
                         "--peer-timeout / --weak-timeout, and a leg that would start with less than 20 s left is skipped -- so the one "
                         "JSON line is out, and every rank has exited 0, inside the budget whatever the legs do")
    ap.add_argument("--no-weak", action="store_true", help="N>1, --full: skip the weak-scaling layout after the headline")
    ap.add_argument("--weak-timeout", type=float, default=300.0,
                    help="N>1: seconds the weak-scaling leg may take; after that the line is printed with "
                         "weak_scaling = {error: timeout} and every rank exits 0 (the headline is never lost to it)")
    ap.add_argument("--transport", type=str, default="rccl", choices=["rccl", "peer"],
                    help="N>1: communicator of the HEADLINE run: rccl (default; the peer-window transport then runs as a second, "
                         "guarded leg) or peer (sns_peer_*: no RCCL in the data path; no second leg)")
    ap.add_argument("--shared-gpu", action="store_true",
                    help="REHEARSAL of --gpus N on a 1-GPU box: every rank uses cuda:0 and torch.distributed runs on gloo; needs "
                         "--transport peer (RCCL cannot put two ranks on one GPU).  The ranks compete for the one GPU: the line is "
                         "marked shared_gpu_rehearsal and its timings mean nothing")
    ap.add_argument("--no-peer", action="store_true",
                    help="N>1: skip the repetition of the timed steps over the peer-window transport (sns_peer_*)")
    ap.add_argument("--peer-timeout", type=float, default=300.0,
                    help="N>1: seconds the peer-transport leg may take (as --weak-timeout: the measured line is never lost to it)")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE",
                    help="extra sns_options field for experiments, e.g. --opt amg_agg_size=4")
    ap.add_argument("--strong", action="store_true", help="(default since round 2; kept for old command lines)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no HIP: launch, partition, halo plans and one all-reduce on gloo (CPU rehearsal of --gpus N)")
    ap.add_argument("--launch-timeout", type=float, default=3000.0,
                    help="self-launched runs: kill the workers and exit non-zero after this many seconds")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="--gpus 1: after the timed steps write what the last timed Newton step returned (the solution vector, its "
                         "residual norms and counts) as DIR/<name>.npy, at most 64 MB in all (a seeded sample of a larger vector)")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args, argv):
    """`python bench.py --gpus N` as a plain command: start N workers (one per GPU) BEFORE anything touches the GPU
    or imports torch in this process, relay their output, return their exit code.  Never exec()s."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    print(f"[bench] launching {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    killed = []
    err_tail = []

    def relay_stderr():                                # pass the workers' stderr through, keep its tail for the record
        for eline in proc.stderr:
            sys.stderr.write(eline)
            sys.stderr.flush()
            err_tail.append(eline)
            del err_tail[:-200]

    et = threading.Thread(target=relay_stderr, daemon=True)
    et.start()

    def reaper():
        if proc.poll() is None:
            killed.append(True)
            print(f"[bench] launch timeout after {args.launch_timeout:.0f} s: killing the workers", file=sys.stderr, flush=True)
            try:
                os.killpg(proc.pid, 9)                 # the session we created: our workers and nothing else
            except OSError:
                proc.kill()

    timer = threading.Timer(args.launch_timeout, reaper)
    timer.daemon = True
    timer.start()
    held = []
    for line in proc.stdout:                           # rank 0's JSON line (and anything else the workers print)
        if line.lstrip().startswith("{") and '"metric"' in line:
            held.append(line)                          # the result line goes out only if the launch as a whole succeeded
            continue
        sys.stdout.write(line)
        sys.stdout.flush()
    rc = proc.wait()
    timer.cancel()
    et.join(timeout=5.0)
    self_launch.last_stderr_tail = "".join(err_tail)
    got_json = bool(held)
    for line in held:
        (sys.stdout if rc == 0 and not killed else sys.stderr).write(line if rc == 0 and not killed else "[bench] result line of a FAILED launch (not reported): " + line)
    sys.stdout.flush()
    if killed:
        return 124
    if rc == 0 and not got_json:
        print("[bench] workers exited 0 without a result line", file=sys.stderr, flush=True)
        return 3
    return rc


class Watchdog:
    """A rank that makes no progress for SNS_WATCHDOG_S seconds exits non-zero (os._exit: no re-exec, no clean-up
    that could hang on a stuck collective); torch.distributed.run then tears the other ranks down."""

    def __init__(self, rank):
        self.limit = float(os.environ.get("SNS_WATCHDOG_S", "900"))
        self.rank = rank
        self.last = time.monotonic()
        self.what = "start"
        if self.limit > 0:
            t = threading.Thread(target=self._run, daemon=True)
            t.start()

    def tick(self, what):
        self.last = time.monotonic()
        self.what = what

    def _run(self):
        while True:
            time.sleep(min(5.0, max(0.05, self.limit / 4)))
            if time.monotonic() - self.last > self.limit:
                print(f"[bench] watchdog: rank {self.rank} made no progress for {self.limit:.0f} s after '{self.what}': "
                      "exiting 86", file=sys.stderr, flush=True)
                os._exit(86)


WATCHDOG = None
T_START = time.monotonic()                # (this rank's process: torch import, rendezvous and setup all count against --budget)


MIN_LEG_S = float(os.environ.get("SNS_BENCH_MIN_LEG_S", "20"))      # a secondary leg is not started with less than this left for it
LEG_RESERVE_S = float(os.environ.get("SNS_BENCH_RESERVE_S", "12"))   # kept back for printing the line and leaving


def leg_seconds(budget, cap, legs_left, now=None):
    """Deadline of the next secondary leg: an equal share of what is left of --budget (minus a reserve for printing the line
    and leaving) among the legs still to run, at most the leg's own cap; less than MIN_LEG_S left for it = skip (returns 0)."""
    left = budget - ((time.monotonic() if now is None else now) - T_START) - LEG_RESERVE_S
    share = left / max(1, legs_left)
    if share < MIN_LEG_S:
        return 0.0
    return min(cap, share)


def run_weak_leg_guarded(out, rank, seconds, leg, key="weak_scaling", what="weak-scaling"):
    """The weak-scaling leg (and, with key = "peer_transport", the peer-transport leg) must never cost the already-measured
    headline: `leg()` (which fills out[key]) runs
    in this thread under a deadline kept by a timer thread of this same process (no child, no re-exec).  If the leg has
    not returned after `seconds`, rank 0 prints THE line with weak_scaling = {"error": "timeout ..."} and every rank leaves
    with os._exit(0) -- no clean-up that could wait on a stuck collective; the ranks enter the leg behind a common barrier, so
    their deadlines expire together and the launcher sees N clean exits.  Returns normally when the leg finished in time."""
    lock = threading.Lock()
    state = {"over": False}

    def expire():
        with lock:
            if state["over"]:
                return
            state["over"] = True
            if rank == 0:
                out[key] = {"error": f"timeout: the {what} leg did not finish within {seconds:.0f} s (headline unaffected)"}
                print(json.dumps(out), flush=True)
            print(f"[bench] rank {rank}: {what} leg exceeded {seconds:.0f} s: leaving with the headline only",
                  file=sys.stderr, flush=True)
            os._exit(0)

    timer = threading.Timer(seconds, expire)
    timer.daemon = True
    timer.start()
    try:
        leg()
    finally:
        with lock:                                   # (an expiry in progress keeps the lock until os._exit)
            state["over"] = True
        timer.cancel()


if __name__ == "__main__":
    _ARGS = parse_args()
    if _ARGS.steps < 1 or _ARGS.warmup < 0:
        print("error: --steps must be >= 1 and --warmup >= 0", file=sys.stderr)
        sys.exit(2)
    if _ARGS.dump_outputs and (_ARGS.gpus > 1 or _ARGS.dry_run):
        print("error: --dump-outputs needs a run on one GPU (--gpus 1, no --dry-run)", file=sys.stderr)
        sys.exit(2)
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != max(1, _ARGS.gpus):
        print(f"error: --gpus {_ARGS.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']} (start `python bench.py --gpus N` as a "
              "plain command, or run it under torch.distributed.run with --nproc-per-node N)", file=sys.stderr)
        sys.exit(2)
    if _ARGS.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _t0 = time.monotonic()
        _rc = self_launch(_ARGS, sys.argv[1:])
        # One documented fallback: a first attempt that FAILED FAST (crash, not a hang: the launch
        # timeout and the 900-s watchdog are not retried) is repeated once with the halo exchange and the operator pass on
        # one stream (SNS_NO_OVERLAP=1: exchange, then one full pass -- the path the single-GPU tests compare the
        # two-stream choreography against, bitwise); the result line says so under "launch_fallback".
        if _rc not in (0, 124) and time.monotonic() - _t0 < 300.0 and not os.environ.get("SNS_NO_OVERLAP"):
            # the first attempt's exit code and stderr tail go on file, so that the crash is diagnosed from the record
            # instead of being buried under the second run's output; the line of the second run is marked DEGRADED
            _logdir = os.environ.get("SNS_BENCH_LOG_DIR") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpurun_out")
            _logf = os.path.join(_logdir, f"bench_first_attempt_rc{_rc}.log")
            try:
                os.makedirs(_logdir, exist_ok=True)
                with open(_logf, "w") as _fh:
                    _fh.write(f"# python bench.py {' '.join(sys.argv[1:])}: first attempt (overlapped halo) exited {_rc} after "
                              f"{time.monotonic() - _t0:.0f} s; stderr tail:\n" + getattr(self_launch, "last_stderr_tail", ""))
            except OSError:
                _logf = None
            print(f"[bench] first attempt exited {_rc} (stderr tail in {_logf}): one more attempt with SNS_NO_OVERLAP=1; its "
                  "line will carry degraded = true", file=sys.stderr, flush=True)
            os.environ["SNS_NO_OVERLAP"] = "1"
            os.environ["SNS_BENCH_FALLBACK"] = (f"SNS_NO_OVERLAP=1 after a first attempt that exited {_rc}"
                                                + (f" (record: {_logf})" if _logf else ""))
            _rc = self_launch(_ARGS, sys.argv[1:])
        sys.exit(_rc)

# the host driver only supports dmabuf IPC: RCCL / cross-process device memory need this before HIP initialises
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    # torch.distributed.run exports OMP_NUM_THREADS=1 to its workers; the host-side symbolic setup (BSR pattern,
    # gather lists: OpenMP in libsns.so) wants this rank's share of the cores.  Must happen before libgomp loads.
    _lw = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ["WORLD_SIZE"]))
    os.environ["OMP_NUM_THREADS"] = str(max(1, min(16, (os.cpu_count() or 8) // max(1, _lw))))

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def cpu_baseline(mesh, mask, g, U, Re, maxit=1500):
    """The oracle's C/OpenMP restatement ("port", oracle/c) timed on the host cores on THE SAME workload as the GPU
    line (same mesh, BCs, initial guess, tolerances): ONE Newton iteration at the Stokes solution U
    of the full mesh -- assemble J+F, solve J y = F to rtol 1e-8, line-search residual -- with the REFERENCE's linear
    algorithm: KSP tfqmr (NavierStokesChannelFlow.py:77,282-283) + PETSc's default preconditioner in parallel,
    block-Jacobi (one block per thread) with ILU(0) on each block.  The Krylov solve is bounded by `maxit`
    iterations so that a run cannot hang on it; the default bound (1500) is far beyond the ~740 iterations after which
    tfqmr stops BY ITS OWN CRITERION on the headline workload.  `ksp_reason` is that criterion's outcome as PETSc's tfqmr
    applies it (the quasi-residual bound tau*sqrt(m+1) <= rtol*||b||, KSPSolve_TFQMR); the bound is known to run ahead of
    the true residual, so ||b - A x|| / ||b|| of the returned iterate is stated next to it, and `ksp_reason_strict` is what
    the port reports when the TRUE residual must be within 10x of the tolerance as well."""
    from oracle import cport
    # one GPU's host share is 16 cores on the bench box; the reference's own runs use 6 ranks (run_all_images.sh:6)
    cport.set_num_threads(min(16, os.cpu_count() or 1, cport.num_threads()))
    nthr = cport.num_threads()
    print(f"[bench] cpu_baseline: {mesh.num_tets} tets on {nthr} threads", file=sys.stderr, flush=True)
    rp, ci = cport.pattern(mesh.num_nodes, mesh.tets)
    t0 = time.time()
    vals, F = cport.assemble("ns", mesh.points, mesh.tets, U, Re, mask, g, rp, ci)
    t1 = time.time()
    print(f"[bench] cpu_baseline: assembly {t1 - t0:.1f}s", file=sys.stderr, flush=True)
    y, its, reason_strict, rn = cport.solve(mesh.num_nodes, rp, ci, vals, F, method="tfqmr", pc="ilu0", rtol=1e-8, maxit=maxit)
    t2 = time.time()
    info = cport.last_solve_info()
    reason = 2 if info["petsc_criterion_met"] else reason_strict
    print(f"[bench] cpu_baseline: tfqmr {its} its reason {reason} in {t2 - t1:.1f}s", file=sys.stderr, flush=True)
    _, Fn = cport.assemble("ns", mesh.points, mesh.tets, U - y, Re, mask, g, rp, ci)      # line-search residual
    t3 = time.time()
    ndof = mesh.num_dofs
    f0, f1 = float(np.linalg.norm(F)), float(np.linalg.norm(Fn))
    converged = None
    ref_file = os.path.join(ROOT, "profiles", "r3_cpu_baseline_converged.json")
    if os.path.exists(ref_file):          # ONE run of this same leg with --cpu-maxit 12000, committed (not repeated per bench run)
        try:
            c = json.loads(open(ref_file).read().strip().split("\n")[-1])["cpu_baseline"]
            converged = {"file": "profiles/r3_cpu_baseline_converged.json", "seconds": round(c["t_asm_s"] + c["t_solve_s"] + c["t_residual_s"], 1),
                         "ksp_its": c["ksp_its"], "cores": c["cores"], "value": c["value"], "unit": "M-DOF/s",
                         "note": "same mesh, same leg, Krylov solve NOT bounded: tfqmr stops by its own criterion (PETSc's: the "
                                 "quasi-residual bound tau*sqrt(m+1) <= rtol*||b||) after 740 iterations / 94.5 s with a TRUE residual of "
                                 "3.9e-6 ||b|| (the bound is known to run ahead of the residual; PETSc would report CONVERGED_RTOL here, "
                                 "the port reports -3 because it checks the true residual); ||F|| 2.18e-01 -> 2.86e-03 after the step"}
        except Exception:                 # noqa: BLE001 -- an unreadable record only drops the key
            converged = None
    bound = (f" -- stopped by tfqmr's own criterion (quasi-residual bound {info['tested'] / f0:.1e} ||b||), TRUE residual "
             f"{rn / f0:.1e} ||b||" if reason > 0 else
             f" -- NOT converged within {maxit} iterations (||r||/||b|| {rn / f0:.1e}): upper bound")
    return {"value": round(ndof / (t3 - t0) / 1e6, 4), "unit": "M-DOF/s", "cores": nthr, "kind": "port",
            "t_asm_s": round(t1 - t0, 2), "t_solve_s": round(t2 - t1, 2), "t_residual_s": round(t3 - t2, 2),
            "ksp_its": its, "ksp_reason": reason, "ksp_reason_strict": reason_strict,
            "ksp_criterion": "PETSc tfqmr: quasi-residual bound tau*sqrt(m+1) <= rtol*||b|| (rtol 1e-8)",
            "quasi_residual_bound_rel": float(f"{info['tested'] / f0:.3e}"), "true_residual_rel": float(f"{rn / f0:.3e}"),
            "converged_reference": converged,
            "sample": f"the GPU line's own workload: 1 Newton iteration at the Stokes solution on {mesh.num_tets} tets / "
                      f"{ndof} dofs, Re={Re:g}: C/OpenMP assembly {t1 - t0:.2f}s + tfqmr/bjacobi({nthr})-ILU(0) "
                      f"{t2 - t1:.2f}s ({its} its, reason {reason}) + residual {t3 - t2:.2f}s; "
                      f"||F|| {f0:.2e} -> {f1:.2e}{bound}"}


def pmc_traffic(kernel_substr):
    """(bytes, source file names): per-launch HBM bytes of a kernel from the COMMITTED rocprofv3 --pmc CSVs
    (profiles/*pmc*counter_collection.csv; not measured in this run -- `traffic_source` in the line names the files),
    corrected as MI355X_MICROARCH.md prescribes: FETCH_SIZE is in KiB and reads half the bytes of a wide streaming
    read on gfx950 (x2); WRITE_SIZE (KiB) is exact.  (None, None) if no such profile is committed."""
    import csv
    fetch = write = None
    src = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc*counter_collection.csv"))):   # latest round wins
        tot = {"FETCH_SIZE": [0.0, 0], "WRITE_SIZE": [0.0, 0]}
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if kernel_substr in row.get("Kernel_Name", "") and row.get("Counter_Name") in tot:
                    tot[row["Counter_Name"]][0] += float(row["Counter_Value"])
                    tot[row["Counter_Name"]][1] += 1
        if tot["FETCH_SIZE"][1]:
            fetch = tot["FETCH_SIZE"][0] / tot["FETCH_SIZE"][1] * 1024.0 * 2.0
            src["fetch"] = os.path.basename(f)
        if tot["WRITE_SIZE"][1]:
            write = tot["WRITE_SIZE"][0] / tot["WRITE_SIZE"][1] * 1024.0
            src["write"] = os.path.basename(f)
    if fetch is None or write is None:
        return None, None
    return fetch + write, f"profiles/{src['fetch']} + profiles/{src['write']} (committed PMC passes, not this run)"


def host_problem(cfg, cells, length, inlet="image"):
    """(mesh, (mask, g), description) of configs 3 / 4 / 4u on the host (setup, not timed)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M
    if cfg == "3":                         # LidDrivenNavierStokesFlow.py extended to the unit cube
        mesh = M.cavity_mesh(cells[0])
        return mesh, B.cavity_bcs(mesh).flatten(), f"lid-driven unit cube, {cells[0]}^3 cells"
    if cfg == "4b":                        # NavierStokesChannelFlow.py on the geometry image2gmsh3D.py:164-486 builds: nozzle_mesh.py
        from stabilized_navier_stokes_flow_fenicsx_amd import nozzle_mesh as NM
        img = os.path.join(ROOT, "tests", "golden", "inlet_PlusF_final.png")
        lc = cells[0] / 1000.0
        mesh, bcs, _ = NM.channel_from_image_bodyfitted(img, 0.5, lc)
        secs = " / ".join(str(c["triangles"]) for c in mesh.meta.get("cross_sections", [{"triangles": mesh.meta["cross_section_triangles"]}]))
        return mesh, bcs, (f"channel 4x1x1 minus the nozzle wall of the reference's Plus image extruded over x in [0, 0.5] (body-fitted, "
                           f"channel_mesh_size {lc:g}: {mesh.meta['planes']} node planes; cross-sections of {secs} triangles: contour-conforming "
                           "up to 0.15 behind the lip, contour-free lattice, the lattice of twice the spacing in the far field), "
                           "inlet profiles from the image, flowrate ratio 0.5")
    if cfg == "4u":                        # the reference's production meshes are gmsh Delaunay (image2gmsh3D.py:445-486)
        mesh = M.delaunay_channel_mesh(cells[0], lattice="bcc")
        return (mesh, B.channel_bcs(mesh, *B.two_stream_profiles(0.5)).flatten(),
                f"two-stream channel 4x1x1 on an UNSTRUCTURED Delaunay mesh (body-centred lattice, h = 1/{cells[0]}), "
                "flowrate ratio 0.5")
    if inlet == "image":                   # NavierStokesChannelFlow.py:102-117,150-157 on the reference's own input image
        from stabilized_navier_stokes_flow_fenicsx_amd import inlet_image as II
        img = os.path.join(ROOT, "tests", "golden", "inlet_PlusF_final.png")
        mesh, bcs, _ = II.channel_from_image(img, 0.5, cells)
        return mesh, bcs, (f"channel 4x1x1, {cells[0]}x{cells[1]}x{cells[2]} cells, inlet profiles + nozzle walls from the "
                           "reference's Plus image (InletImages/PlusF_final.png, box-filtered copy), flowrate ratio 0.5")
    mesh = M.channel_mesh(cells)
    return (mesh, B.channel_bcs(mesh, *B.two_stream_profiles(0.5)).flatten(),
            f"two-stream channel 4x1x1, {cells[0]}x{cells[1]}x{cells[2]} cells, analytic inlet profiles, flowrate ratio 0.5")


def build_problem(cfg, cells, length, Re, world, rank, local_rank, opts, dist_on, inlet="image", group=None):
    """(P, n_dof_global, n_tets_global, description, host_inputs) of one BASELINE config on this rank.
    Config 5 (duct): x-slab element partition, every rank meshes only its own slab (partition.duct_slab_part).
    Configs 3 / 4 / 4u: the global mesh is built on every rank and RCB-partitioned (setup cost, not timed)."""
    from stabilized_navier_stokes_flow_fenicsx_amd import bcs as B, mesh as M, partition as PT
    from stabilized_navier_stokes_flow_fenicsx_amd.solver import FlowProblem
    dev = f"cuda:{local_rank}"
    host = None
    if cfg == "5":
        if dist_on:
            part = PT.duct_slab_part(cells, length, rank, world)
            P = FlowProblem.from_part(part, device=dev, group=group, **opts)
        else:
            mesh = M.duct_mesh(cells, length)
            bcs = B.duct_bcs(mesh).flatten()
            P = FlowProblem(mesh, bcs, device=dev, **opts)
            host = (mesh, bcs)
        nd = 4 * (cells[0] + 1) * (cells[1] + 1) * (cells[2] + 1)
        nt = 6 * cells[0] * cells[1] * cells[2]
        desc = f"duct [0,{length:g}]x[-.5,.5]^2, {cells[0]}x{cells[1]}x{cells[2]} cells"
    else:
        mesh, bcs, desc = host_problem(cfg, cells, length, inlet)
        P = (FlowProblem.distributed(mesh, bcs, device=dev, group=group, **opts) if dist_on
             else FlowProblem(mesh, bcs, device=dev, **opts))
        host = (mesh, bcs)
        nd, nt = mesh.num_dofs, mesh.num_tets
    return P, nd, nt, desc, host


def dry_run(args, cfg, cells, length, world, rank):
    """--dry-run: everything `--gpus N` does up to the first HIP call, on the CPU: rendezvous (gloo), this rank's
    partition, the halo plan checked against the neighbours' (one real exchange of node ids), the boundary-row split
    libsns.so derives from it, and one all-reduce.  Prints the same kind of JSON line (value null)."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from stabilized_navier_stokes_flow_fenicsx_amd import _lib, partition as PT
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    WATCHDOG.tick("rendezvous")
    if cfg == "5":
        part = PT.duct_slab_part(cells, length, rank, world)
        nt = 6 * cells[0] * cells[1] * cells[2]
    else:
        mesh, (mask, g), _ = host_problem(cfg, cells, length, args.inlet)
        part = PT.build_local_part(mesh, mask, g, PT.rcb_partition(mesh.points, world), rank, world)
        nt = mesh.num_tets
    WATCHDOG.tick("partition")
    # halo plan: send the GLOBAL ids of the nodes I send; what arrives must be the global ids of my ghost slots
    gid = torch.from_numpy(np.repeat(part.l2g.astype(np.float64), 4))
    gid[4 * part.n_owned:] = -1.0
    if world > 1:
        PT.halo_exchange_torch(part, gid)
    halo_ok = bool(np.array_equal(gid.numpy()[::4].astype(np.int64), part.l2g))
    rp, ci, _, _ = _lib.host_pattern(part.n_local, part.mesh.tets)
    bnd = _lib.host_boundary_rows(part.n_owned, rp, ci)
    t = torch.tensor([float(part.n_owned), float(len(bnd)), 1.0 if halo_ok else 0.0, float(len(part.send_idx))],
                     dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t)
    WATCHDOG.tick("collectives")
    if os.environ.get("SNS_DRYRUN_STALL_RANK") == str(rank):      # test hook: a rank that never comes back
        time.sleep(3600)
    if os.environ.get("SNS_DRYRUN_CRASH_WITH_OVERLAP") and not os.environ.get("SNS_NO_OVERLAP") and rank == world - 1:
        os._exit(7)                                               # test hook: a rank that dies unless the fallback is on
    out = {"metric": "M-DOF/s (assembly+solve) per Newton iteration", "value": None, "unit": "M-DOF/s", "n_gpus": world,
           "dry_run": True, "transport": "gloo (CPU rehearsal, no HIP)", "rccl_ranks": None, "steps": 0, "warmup": 0,
           "launch_fallback": os.environ.get("SNS_BENCH_FALLBACK"), "degraded": bool(os.environ.get("SNS_BENCH_FALLBACK")),
           "config": {"workload": f"BASELINE config {cfg}: {nt} tets, partition + halo plans + one all-reduce only",
                      "parallelism": f"element partition x{world}", "owned_nodes_total": int(t[0]),
                      "boundary_rows_total": int(t[1]), "halo_plans_consistent_ranks": int(t[2]),
                      "halo_send_nodes_total": int(t[3]), "neighbours_of_rank0": [int(x) for x in part.neighbors]}}
    ok = int(t[2]) == world
    if os.environ.get("SNS_DRYRUN_PEER_STALL") and ok:
        # test hook: the peer-transport leg never comes back -- its deadline comes out of --budget like in a real run
        out["peer_transport"] = None
        secs = leg_seconds(args.budget, args.peer_timeout, 2 if args.full else 1)
        if secs > 0:
            run_weak_leg_guarded(out, rank, secs, lambda: time.sleep(36000), key="peer_transport", what="peer-transport")
        else:
            out["peer_transport"] = {"skipped": "less than 20 s of --budget left"}
    if os.environ.get("SNS_DRYRUN_WEAK_STALL") and ok and args.full:
        # test hook: the deadline of the weak-scaling leg with real ranks -- a leg that never comes back (on every rank, as a
        # stuck collective would look) must still end in ONE line on rank 0's stdout and N clean exits
        out["weak_scaling"] = None
        secs = leg_seconds(args.budget, args.weak_timeout, 1)
        if secs > 0:
            run_weak_leg_guarded(out, rank, secs, lambda: time.sleep(36000))
        else:
            out["weak_scaling"] = {"skipped": "less than 20 s of --budget left"}
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0 if ok else 4


def _dist_allreduce(t, op=None):
    """all_reduce of a small device tensor on whatever backend carries torch.distributed here (gloo: through the host)"""
    import torch.distributed as dist
    kw = {} if op is None else {"op": op}
    if dist.get_backend() == "gloo":
        tc = t.cpu()
        dist.all_reduce(tc, **kw)
        t.copy_(tc)
    else:
        dist.all_reduce(t, **kw)


def halo_overlap_selfcheck(P, world):
    """First contact of the overlapped halo path with a real multi-rank RCCL communicator: one operator pass with the
    interior / boundary split on two streams against the same pass as exchange-then-full-pass (halo_overlap = 0).
    Both compute every row with the same arithmetic, so the results must agree BITWISE on every rank; if they do
    not, the run continues on the fallback and the line says so."""
    import torch
    import torch.distributed as dist
    x = torch.arange(P.ndof, dtype=torch.float64, device=P.device).remainder(11.0) - 5.0
    x[4 * P.n_owned:] = 0.0
    no = 4 * P.n_owned
    if os.environ.get("SNS_NO_OVERLAP"):
        return "SNS_NO_OVERLAP set: exchange-then-full-pass"
    P.set_options(halo_overlap=0)
    y0 = P.spmv(x.clone())[:no].clone()
    P.set_options(halo_overlap=1)
    y1 = P.spmv(x.clone())[:no].clone()
    bad = torch.tensor([0.0 if torch.equal(y0, y1) else 1.0], dtype=torch.float64, device=P.device)
    if world > 1:
        _dist_allreduce(bad)
    if float(bad) > 0:
        P.set_options(halo_overlap=0)
        return f"MISMATCH on {int(bad)} rank(s): overlapped halo disabled, exchange-then-full-pass used"
    return "overlapped interior/boundary split == exchange-then-full-pass, bitwise, on every rank"


def halo_windows_selfcheck(P, world):
    """The peer-window transport's counterpart of halo_overlap_selfcheck, the first contact of the level passes' read path with
    real links: one operator pass that reads the ghost entries straight from the receive window (halo_windows = 1: one put
    launch, the boundary waves wait for the neighbours' flags themselves) against the same pass after put + wait / unpack into
    the vector's ghost tail (halo_windows = 0).  Every row is computed with the same arithmetic in the same order, so the
    results must agree BITWISE on every rank; if they do not, the run continues on the unpack path and the line says so."""
    import torch
    x = torch.arange(P.ndof, dtype=torch.float64, device=P.device).remainder(11.0) - 5.0
    x[4 * P.n_owned:] = 0.0
    no = 4 * P.n_owned
    P.set_options(halo_windows=0)
    y0 = P.spmv(x.clone())[:no].clone()
    P.set_options(halo_windows=1)
    y1 = P.spmv(x.clone())[:no].clone()
    bad = torch.tensor([0.0 if torch.equal(y0, y1) else 1.0], dtype=torch.float64, device=P.device)
    if world > 1:
        _dist_allreduce(bad)
    if float(bad) > 0:
        P.set_options(halo_windows=0, amg_exact_sweeps=0)
        return f"MISMATCH on {int(bad)} rank(s): window reads disabled, put + unpack used"
    return "ghost entries read straight from the receive window == put + unpack into the ghost tail, bitwise, on every rank"


def timed_newton_steps(P, U, steps, warmup, world):
    """W untimed + K timed Newton iterations of a real sequence from the Stokes solution U (restarted when it has
    converged); barrier + synchronize on both sides, MAX over ranks.  Returns (ms_per_step, log, w to go on from, (w, result)
    of the last timed step)."""
    import torch
    import torch.distributed as dist

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    state = {"w": U.clone(), "seq": 0, "last": None}
    log = []

    def step():
        w, r = P.newton_solve(state["w"])
        state["w"] = w
        state["last"] = (w, r)                                          # (w stays this step's result after a restart)
        state["seq"] += 1
        log.append((r.fnorms[-1] if r.fnorms else float("nan"), r.ksp_its, r.reason))
        if r.reason == 2 or r.reason == 3 or state["seq"] >= 30:       # sequence converged: start over
            state["w"] = U.clone()
            state["seq"] = 0

    for _ in range(warmup):
        step()
        if WATCHDOG:
            WATCHDOG.tick("warm-up step")
    P.reset_timings()
    P.time_kernels(True)
    log.clear()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        if WATCHDOG:
            WATCHDOG.tick("timed step")                # a time stamp only: nothing inside the timed region waits on it
    barrier()
    dt = time.perf_counter() - t0
    P.time_kernels(False)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        _dist_allreduce(t, dist.ReduceOp.MAX)
        dt = float(t)
    return dt / max(1, steps) * 1e3, log, state["w"], state["last"]


DUMP_BYTES = 64_000_000                                # --dump-outputs: all files together


def dump_outputs(dirname, w, r):
    """What a caller of the timed path (FlowProblem.newton_solve) received in the last timed step, as DIR/<name>.npy:
    w.npy = the solution vector (float64; if it alone would exceed the budget, a sample at fixed, seeded indices, whose
    positions go to w_index.npy), fnorms.npy = the step's residual norms, newton.npy = [its, reason, ksp_its]."""
    os.makedirs(dirname, exist_ok=True)
    import numpy as np
    small = {"fnorms": np.asarray(r.fnorms, dtype=np.float64),
             "newton": np.asarray([r.its, r.reason, r.ksp_its], dtype=np.float64)}
    wh = w.detach().cpu().numpy().astype(np.float64, copy=False)
    room = DUMP_BYTES - sum(a.nbytes for a in small.values()) - 4 * 128          # (128 B: an .npy header)
    arrays = dict(small)
    if wh.nbytes <= room:
        arrays["w"] = wh
    else:
        k = room // 16                                 # value + index, both float64
        idx = np.sort(np.random.default_rng(0).choice(wh.size, size=k, replace=False))
        arrays["w"], arrays["w_index"] = wh[idx], idx.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    print(f"[bench] outputs of the last timed step in {dirname}: " + ", ".join(f"{n}.npy {a.shape}" for n, a in arrays.items()),
          file=sys.stderr, flush=True)


def leg_record(P, U, sres, args, cfg, world, n_dof_global, f64_rerun=True, dump_dir=None):
    """The W + K timed Newton steps on handle P and every key of the line that belongs to THAT run of them: value, step time,
    transport, Newton log, phases, counters, the live roofline of the fine-level passes (HIP events around every launch) and
    the all-f64 repetition.  One record per transport leg: the line never mixes keys of two runs.  dump_dir: write
    the last timed step's outputs there (dump_outputs).  The assembly timed alone and the all-f64 repetition run with --full only."""
    comm = P.comm_info()
    ms_per_step, log, w, last = timed_newton_steps(P, U, args.steps, args.warmup, world)
    if dump_dir:
        dump_outputs(dump_dir, *last)
    value = n_dof_global / (ms_per_step * 1e-3) / 1e6
    tm = P.timings()
    kt = P.kernel_times()
    s = P.sizes()
    ctr = P.counters()
    # K1 (Jacobian + residual assembly) timed on its own after the timed region: HIP events around 5 passes
    asm_ms = P.bench_assemble(w, "ns", 5) if args.full else None
    asm_bytes = 2480.0 * s["n_tets"]                   # 2480 B/tet
    # the same K steps once more with EVERY array in fp64 (no fp32 copies inside the preconditioner), reported
    # beside the headline so that the effect of the mixed-precision preconditioner is on record
    all_f64 = None
    fmt0 = int(P.options.amg_f32_matrix)
    if fmt0 and f64_rerun and args.full and not args.no_f64_rerun:
        P.set_options(amg_f32_matrix=0)
        ms64, log64, _, _ = timed_newton_steps(P, U, args.steps, args.warmup, world)
        all_f64 = {"value": round(n_dof_global / (ms64 * 1e-3) / 1e6, 3), "unit": "M-DOF/s", "ms_per_step": round(ms64, 3),
                   "ksp_its": [b for _, b, _ in log64]}
        P.set_options(amg_f32_matrix=fmt0)
    # The fine-level matrix passes of a BiCGStab iteration: y = Ax and y = Ax + <r^, y> on the fp64 operator, and per
    # V-cycle (two per iteration) the residual on the preconditioner's matrix copy plus -- since round 3 -- the fused
    # coarse-grid correction + post-smoothing sweep over M = A P (0.37x the blocks of A) in place of a full Jacobi sweep.
    # Algorithmic bytes per launch:
    #   per nonzero block: values + 4 B column index -- 128 B fp64 operator, 64 B fp32 copy, 32 B fp16 copy
    #   per block row:     4 rowptr + 32 per vector touched (x, b, y, dot weight) + D^-1 (Jacobi: 128 B fp64, 64 B as the
    #                      fp32 copy the low-precision sweeps read) + 16 row scales (fp16)
    fmt = int(P.options.amg_f32_matrix)
    lp = {0: ("k_spmv<{m}, 1, 1, 0>", 132.0, 0.0), 1: ("k_spmv_lp<{m}, 1, 0, 1, 1>", 68.0, 0.0), 2: ("k_spmv_lp<{m}, 1, 0, 2, 1>", 36.0, 16.0)}[fmt]
    nb, nr = float(s["nnzb"]), float(s["n_owned"])
    nm = float(ctr["ap_blocks"])                     # blocks of M = A P (fine rows x coarse columns)
    kinfo = {
        # fused coarse-grid correction + first post-smoothing sweep: M's blocks + per row rowptr 4, r1 32, x1 32, agg 4,
        # P xc 32, free mask 4, D^-1 (fp32) 64, y 32, row scales (fp16)
        "post_m": (f"k_post_lp<{fmt}, 1>", lp[1] * nm + (4 + 32 * 4 + 4 + 4 + 64 + lp[2]) * nr,
                   "AMG fine level: coarse-grid correction + post-smoothing sweep in one pass over M = A P"),
        "jacobi": (lp[0].format(m=2), lp[1] * nb + (4 + 32 * 3 + (128 if fmt == 0 else 64) + lp[2]) * nr,
                   "AMG fine-level block-Jacobi sweep (a full pass over A: only where the fused sweep is off)"),
        "b_minus_ax": (lp[0].format(m=1), lp[1] * nb + (4 + 32 * 3 + lp[2]) * nr, "AMG fine-level residual r = b - Ax"),
        "ax": ("k_spmv<0, 1, 1, 0>", 132.0 * nb + (4 + 32 * 2) * nr, "Krylov operator y = Ax (fp64)"),
        "ax_dot": ("k_spmv<3, 1, 1, 0>", 132.0 * nb + (4 + 32 * 3) * nr, "Krylov operator y = Ax + <r^, y> (fp64)"),
    }
    per_kernel = {}
    for key, (kname_k, bytes_k, what) in kinfo.items():
        ms_k, calls_k = kt[key]
        if calls_k > 0:
            avg = ms_k / calls_k
            ach = bytes_k / (avg * 1e-3) / 1e9
            per_kernel[key] = {"kernel": kname_k, "what": what, "avg_launch_ms": round(avg, 5), "launches": int(calls_k),
                               "total_ms": round(ms_k, 2), "algorithmic_bytes_per_launch": bytes_k,
                               "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBS, 4),
                               # (profiles older than r2e carry the low-precision kernel without its last template argument)
                               "traffic": None, "traffic_source": None}
            if cfg == "5":
                per_kernel[key]["traffic"], per_kernel[key]["traffic_source"] = pmc_traffic(
                    kname_k[:kname_k.rindex(",")] if kname_k.startswith("k_spmv_lp") else kname_k)
    roofline = None
    if per_kernel:
        dom = max(per_kernel, key=lambda k_: per_kernel[k_]["total_ms"])       # dominant = largest total time, live
        d = per_kernel[dom]
        fam_bytes = sum(v["algorithmic_bytes_per_launch"] * v["launches"] for v in per_kernel.values())
        fam_ms = sum(v["total_ms"] for v in per_kernel.values())
        roofline = {"bound": "hbm", "achieved": d["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": d["frac"],
                    "traffic": d["traffic"], "traffic_source": d["traffic_source"], "kernel": d["kernel"], "what": d["what"],
                    "avg_launch_ms": d["avg_launch_ms"], "launches": d["launches"],
                    "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"],
                    "selection": "the fine-level SpMV kernel with the largest total time inside the timed region "
                                 "(HIP events around every launch); the four are within a few % of each other",
                    "fine_level_spmv_kernels": per_kernel,
                    # every algorithmic byte of the fine-level matrix passes of the timed region over the WHOLE step time:
                    # what the step as a whole reaches of the HBM roofline (the rest of the step is latency-bound work
                    # below the fine level, vector kernels, assembly and setup, whose bytes are not counted here)
                    "step_frac": round(fam_bytes / (ms_per_step * args.steps * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "step_frac_note": "sum of the algorithmic bytes of all fine-level matrix passes in the timed region / "
                                      "(steps x ms_per_step) / 8 TB/s",
                    "fine_level_spmv_family": {"share_of_step": round(fam_ms / (ms_per_step * args.steps), 3),
                                               "achieved": round(fam_bytes / (fam_ms * 1e-3) / 1e9, 1),
                                               "frac": round(fam_bytes / (fam_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                    "assembly_kernels": {"avg_ms": round(asm_ms, 4), "algorithmic_bytes": asm_bytes,
                                         "achieved": round(asm_bytes / (asm_ms * 1e-3) / 1e9, 1),
                                         "frac": round(asm_bytes / (asm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                         "note": "nominal: SURVEY 8d's 2480 B/tet over the kernel time; the scratch-free "
                                                 "kernels never move the 2 KiB/tet element matrix (PMC traffic 0.25-0.37x "
                                                 "of that) -- their honest bound is the fp64-VALU figure below",
                                         "path": "scratch-free (k_fused_offdiag + k_fused_diag)"
                                                 if P.options.assembly_fused else "staged (k_element + gathers)",
                                         # secondary: executed fp64 VALU flops of the scratch-free path,
                                         # counted from the gfx950 ISA: 300 fmac + 82 fma + 244 mul + 97 add per
                                         # block contribution = 1105 flop, 16 contributions per tet
                                         "fp64_vector": ({"executed_flops_per_tet": 17680,
                                                          "achieved_tflops": round(17680.0 * s["n_tets"] / (asm_ms * 1e-3) / 1e12, 2),
                                                          "peak_tflops": 78.6,
                                                          "frac": round(17680.0 * s["n_tets"] / (asm_ms * 1e-3) / 1e12 / 78.6, 4)}
                                                         if P.options.assembly_fused else None)}
                                        if asm_ms is not None else None}
    return {"value": round(value, 3), "ms_per_step": round(ms_per_step, 3), "transport": comm["transport"], "rccl_ranks": comm["rccl_ranks"],
            "log": log, "phase_ms_per_step": {"assemble": round(tm.assemble_ms / args.steps, 3),
                                              "pc_setup": round(tm.pc_setup_ms / args.steps, 3),
                                              "krylov": round(tm.krylov_ms / args.steps, 3)},
            "krylov_loop_last_solve": {"host_syncs": ctr["host_syncs"], "allreduces": ctr["allreduces"],
                                       "halo_exchanges": ctr["exchanges"], "its": log[-1][1] if log else None},
            "amg_levels": tm.amg_levels, "stokes_its": sres.its, "roofline": roofline, "all_f64_preconditioner": all_f64,
            "precision_fmt": fmt}


def leg_summary(rec):
    """the short form of a leg's record (the leg that is NOT the headline)"""
    return {"value": rec["value"], "unit": "M-DOF/s", "ms_per_step": rec["ms_per_step"], "transport": rec["transport"],
            "ksp_its": [b for _, b, _ in rec["log"]], "stokes_its": rec["stokes_its"], "phase_ms_per_step": rec["phase_ms_per_step"],
            "krylov_loop_last_solve": rec["krylov_loop_last_solve"],
            "fine_level_family_frac": (rec["roofline"] or {}).get("fine_level_spmv_family", {}).get("frac")}


def same_sequence(log_a, log_b):
    """the same Newton sequence on two transports: same SNES reasons, Krylov iterations within 3, |F| within 0.1 % (the
    transports sum the all-reduce contributions in different orders: last-bit differences only)"""
    return bool(len(log_a) == len(log_b) and all(
        c1 == c2 and abs(b1 - b2) <= 3 and abs(a1 - a2) <= 1e-3 * max(abs(a2), 1e-300)
        for (a1, b1, c1), (a2, b2, c2) in zip(log_a, log_b)))


def main():
    global WATCHDOG
    args = parse_args()

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, args.gpus):                              # (also checked before torch was imported)
        print(f"error: --gpus {args.gpus} but WORLD_SIZE {world}", file=sys.stderr)
        return 2
    WATCHDOG = Watchdog(rank)
    cfg = args.config
    default_cells = {"5": "300,75,75", "4": "240,60,60", "4b": "20", "4u": "47", "3": "55,55,55"}[cfg]
    cells = tuple(int(c) for c in (args.cells or default_cells).split(","))
    length = args.length
    if args.dry_run:
        return dry_run(args, cfg, cells, length, world, rank)
    if args.shared_gpu:
        if args.transport != "peer":
            print("error: --shared-gpu needs --transport peer (RCCL cannot put two ranks on one GPU)", file=sys.stderr)
            return 2
        local_rank = 0                                           # every rank on the box's one GPU (rehearsal)
    torch.cuda.set_device(local_rank)
    force_dist = bool(os.environ.get("SNS_FORCE_DIST"))          # rehearse the partitioned path with one rank
    dist_on = world > 1 or force_dist
    peers = None
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29561")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.shared_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        if args.transport == "peer":
            from stabilized_navier_stokes_flow_fenicsx_amd.solver import PeerGroup
            peers = PeerGroup(device=f"cuda:{local_rank}")

    Re = args.re if args.re is not None else {"5": 200.0, "4": 50.0, "4b": 50.0, "4u": 50.0, "3": 100.0}[cfg]
    opts = dict(reynolds=Re, ksp_type=args.ksp, pc_type="amg", snes_max_it=1)
    for kv in args.opt:
        k, v = kv.split("=", 1)
        opts[k] = float(v) if ("." in v or "e" in v.lower()) else int(v)

    # ---- headline: the SAME mesh on N GPUs (strong scaling; N = 1 is the mesh on one GPU) ----------------------
    P, n_dof_global, n_tets_global, desc, host = build_problem(cfg, cells, length, Re, world, rank, local_rank, opts, dist_on,
                                                               args.inlet, group=peers)
    WATCHDOG.tick("setup")
    comm = P.comm_info()
    if dist_on and world > 1 and peers is None and comm["rccl_ranks"] != world:
        print(f"error: RCCL communicator has {comm['rccl_ranks']} ranks, expected {world}", file=sys.stderr)
        return 5
    U, sres = P.stokes_solve()                       # initial guess, as the reference does (:519-523)
    if sres.reason <= 0:
        raise RuntimeError(f"Stokes solve did not converge: {sres}")
    WATCHDOG.tick("stokes")
    halo_check = (halo_windows_selfcheck(P, world) if peers is not None else halo_overlap_selfcheck(P, world)) if dist_on else None
    WATCHDOG.tick("halo self-check")
    rec = leg_record(P, U, sres, args, cfg, world, n_dof_global, dump_dir=args.dump_outputs)

    def line_of(rec):
        """THE JSON line with every leg-specific key taken from ONE leg's record"""
        fmt = rec["precision_fmt"]
        return {
            "metric": "M-DOF/s (assembly+solve) per Newton iteration",
            "value": rec["value"], "unit": "M-DOF/s", "n_gpus": world, "rccl_ranks": rec["rccl_ranks"],
            "transport": rec["transport"], "halo_overlap_selfcheck": halo_check, "launch_fallback": os.environ.get("SNS_BENCH_FALLBACK"),
            # true = this number comes from the fallback launch (exchange-then-full-pass) after the production two-stream path
            # FAILED on this machine: a defect to diagnose from the record named in launch_fallback, not a headline to quote
            "degraded": bool(os.environ.get("SNS_BENCH_FALLBACK")),
            # true = N ranks shared ONE GPU (--shared-gpu: the launch / partition / peer-window path rehearsed on a 1-GPU box): not a measurement
            "shared_gpu_rehearsal": bool(args.shared_gpu),
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "precision_note": ("operator, residuals, Krylov recurrences and reductions in f64; the AMG preconditioner's "
                               "smoother/residual passes read a " + {1: "fp32", 2: "row-scaled fp16"}[fmt] + " copy of the level "
                               "matrices (vectors and arithmetic f64; same Krylov iteration counts); with --full the strict "
                               "all-f64 figure of the same steps is under all_f64_preconditioner") if fmt else "all f64",
            "config": {"workload": f"BASELINE config {cfg}: {desc} = {n_tets_global} tets, "
                                   f"{n_dof_global} dofs, Re={Re:g}, Newton iteration (assemble J+F, AMG setup, "
                                   f"{args.ksp} rtol 1e-8, bt line search)",
                       "parallelism": (f"element partition x{world} ({'x-slabs' if cfg == '5' else 'RCB'}), "
                                       f"{n_tets_global // world} tets per GPU" if world > 1 else "single GPU"),
                       "scaling_note": "strong: the one mesh split N ways (north_star: >= 6x at 8 GPUs on the 10 M-tet duct); "
                                       "with --full the weak layout is under weak_scaling",
                       "newton_log_fnorm_kspits_reason": [(float(f"{a:.3e}"), b, c) for a, b, c in rec["log"]],
                       "phase_ms_per_step": rec["phase_ms_per_step"],
                       "krylov_loop_last_solve": rec["krylov_loop_last_solve"],
                       "amg_levels": rec["amg_levels"], "stokes_its": rec["stokes_its"]},
            "roofline": rec["roofline"],
            "all_f64_preconditioner": rec["all_f64_preconditioner"],
            "peer_transport": None,
            "weak_scaling": None,
            "cpu_baseline": None,
        }

    out = line_of(rec)
    if rank == 0 and world > 1:
        # the measured headline goes out at once (stderr; the ONE line on stdout follows when the secondary legs are through or
        # out of time): whatever happens later, the record of the run holds it
        print("[bench] headline measured: " + json.dumps({k: out[k] for k in ("value", "unit", "n_gpus", "ms_per_step", "transport")}),
              file=sys.stderr, flush=True)
    U_host = (U.cpu().numpy() if (args.full and not args.no_cpu_baseline and rank == 0 and world == 1 and not dist_on
                                  and host is not None) else None)
    P.close()
    del P, U
    torch.cuda.empty_cache()

    # ---- N > 1: the same timed steps once more over the peer-window transport --------------------------------------
    # (sns_peer_*: halo exchange / all-reduce / all-gather as stores into the other ranks' IPC-mapped windows, no RCCL in the
    # data path -- made for the latency-bound strong split.  Same W + K steps, same barriers, same clock.  If this leg is the
    # faster one -- and ran the same Newton sequence, and its communicator passed sns_peer_check_links between the real ranks,
    # halo ring included, without which no PeerGroup exists -- the WHOLE line (value, phases, counters, roofline) is this leg's
    # and the RCCL leg moves under "rccl_transport"; otherwise this leg sits under "peer_transport".  The leg runs under a
    # deadline taken from --budget and every device-side wait inside it is bounded: a transport problem costs this key, not
    # the line.)
    WATCHDOG.tick("headline done")
    weak = cfg == "5" and dist_on and args.full and not args.no_weak
    legs_left = (1 if (dist_on and not args.no_peer and peers is None) else 0) + (1 if weak else 0)
    if dist_on and not args.no_peer and peers is None:
        box = {}

        def peer_leg():
            pg, Pp = None, None
            try:
                from stabilized_navier_stokes_flow_fenicsx_amd.solver import PeerGroup
                pg = PeerGroup(device=f"cuda:{local_rank}")
                Pp, _, _, _, _ = build_problem(cfg, cells, length, Re, world, rank, local_rank, opts, True, args.inlet, group=pg)
                Up, sp = Pp.stokes_solve()
                if sp.reason > 0:
                    wcheck = halo_windows_selfcheck(Pp, world)
                    box["rec"] = leg_record(Pp, Up, sp, args, cfg, world, n_dof_global, f64_rerun=False)
                    out["peer_transport"] = leg_summary(box["rec"])
                    out["peer_transport"]["halo_windows_selfcheck"] = wcheck
                    out["peer_transport"]["same_sequence_as_rccl_leg"] = same_sequence(box["rec"]["log"], rec["log"])
                else:
                    out["peer_transport"] = {"error": f"Stokes solve reason {sp.reason}"}
            except Exception as exc:          # noqa: BLE001 -- reported in the line
                out["peer_transport"] = {"error": f"{type(exc).__name__}: {exc}"}
                box.pop("rec", None)
            finally:
                # the windows go whatever happened (an exception above must not leave the other ranks in the close barrier
                # until the deadline takes the process); errors of the teardown itself only add to the record
                try:
                    if Pp is not None:
                        Pp.close()
                    if pg is not None:
                        pg.close()
                except Exception as exc:      # noqa: BLE001
                    out["peer_transport"] = dict(out.get("peer_transport") or {}, close_error=f"{type(exc).__name__}: {exc}")

        secs = leg_seconds(args.budget, args.peer_timeout, legs_left)
        legs_left -= 1
        if secs > 0:
            run_weak_leg_guarded(out, rank, secs, peer_leg, key="peer_transport", what="peer-transport")
        else:
            out["peer_transport"] = {"skipped": "less than 20 s of --budget left after the headline"}
        # the leg's verdict, agreed between the ranks (a rank whose leg failed must not go on with another line than the others):
        # every rank measured the same MAX-over-ranks time, so the comparison itself is the same everywhere
        ok_here = 1.0 if ("rec" in box and out["peer_transport"].get("same_sequence_as_rccl_leg")) else 0.0
        tok = torch.tensor([ok_here], dtype=torch.float64, device="cuda")
        if world > 1:
            _dist_allreduce(tok, dist.ReduceOp.MIN)
        if world > 1 and float(tok) > 0 and box["rec"]["value"] > rec["value"]:
            keep = {k: out[k] for k in ("peer_transport",)}
            rccl_line = leg_summary(rec)
            out = line_of(box["rec"])
            out["peer_transport"] = dict(keep["peer_transport"], note="this leg IS the headline: value, phases, counters and roofline above are its own")
            out["rccl_transport"] = rccl_line
            out["all_f64_preconditioner"] = rec["all_f64_preconditioner"]          # (measured on the RCCL leg only; says so)
            if out["all_f64_preconditioner"]:
                out["all_f64_preconditioner"] = dict(out["all_f64_preconditioner"], transport=rec["transport"])

    # ---- second key for N > 1: the weak layout (every GPU keeps the single-GPU share) --------------------------
    WATCHDOG.tick("peer leg done")
    if weak:
        sc = float(world) ** (1.0 / 3.0)
        wcells = tuple(int(round(c * sc)) for c in cells)

        def weak_leg():
            Pw = None
            try:                              # a failure of the second key must not cost the headline line ...
                if os.environ.get("SNS_BENCH_WEAK_STALL"):          # test hook: a leg that never comes back
                    time.sleep(36000)
                Pw, nd_w, nt_w, desc_w, _ = build_problem("5", wcells, length, Re, world, rank, local_rank, opts, True, group=peers)
                Uw, sw = Pw.stokes_solve()
                if sw.reason > 0:
                    ms_w, log_w, _, _ = timed_newton_steps(Pw, Uw, args.steps, args.warmup, world)
                    out["weak_scaling"] = {"value": round(nd_w / (ms_w * 1e-3) / 1e6, 3), "unit": "M-DOF/s",
                                           "ms_per_step": round(ms_w, 3), "scaling": "weak", "transport": Pw.comm_info()["transport"],
                                           "workload": f"{desc_w} = {nt_w} tets, {nd_w} dofs ({nt_w // world} tets per GPU)",
                                           "ksp_its": [b for _, b, _ in log_w], "stokes_its": sw.its}
                else:
                    out["weak_scaling"] = {"error": f"Stokes solve reason {sw.reason}"}
            except Exception as exc:          # noqa: BLE001 -- reported in the line
                out["weak_scaling"] = {"error": f"{type(exc).__name__}: {exc}"}
            finally:
                if Pw is not None:
                    Pw.close()

        # ... and neither must a hang: a deadline per rank (the ranks leave the headline's last collective together)
        secs = leg_seconds(args.budget, args.weak_timeout, legs_left)
        if secs > 0:
            run_weak_leg_guarded(out, rank, secs, weak_leg)
        else:
            out["weak_scaling"] = {"skipped": "less than 20 s of --budget left"}

    if rank == 0:
        if U_host is not None:
            mesh, (mask, g) = host
            WATCHDOG.limit = 0 if WATCHDOG.limit <= 0 else max(WATCHDOG.limit, 3600.0)      # a long host-only leg
            WATCHDOG.tick("cpu baseline")
            out["cpu_baseline"] = cpu_baseline(mesh, mask, g, U_host, Re, maxit=args.cpu_maxit)
        print(json.dumps(out), flush=True)
    if peers is not None:
        peers.close()
    if dist_on:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
