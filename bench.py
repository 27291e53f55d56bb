#!/usr/bin/env python3
"""Benchmark of the hot path: Arnoldi steps (time-stepper matvec + orthogonalisation) on MI355X.

    python bench.py --gpus N --steps K --warmup W [--case cfg2|cfg3] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps, writes the outputs of the last timed step (--dump-outputs) and prints
the record: the headline figure and nothing else.  `--full` adds everything else the record can carry: the continuation
to k_dim = 128 and the leading Ritz pair, the byte accounting and the kernel rooflines, the CPU baseline, the Fortran-host
leg, and at N > 1 the same steps on one GPU and the short sharded run of cfg3 (`--extras` and `--ref-logfile` imply it).
A plain run at N > 1 over RCCL still does, before its timed steps, what picks the configuration it times: the RCCL pre-flight
(tests/mp_rccl_worker.py in fresh processes, see supervise) and the comparison of the three sharded step modes.

The workload is the SAME at every N (default: BASELINE configs[1], the configuration the metric is quoted on): Re=50
cylinder, lx1=8, E=1996, direct Arnoldi, k_dim=128.  One "step" = one Arnoldi step = nsteps(=183) linearised Navier-Stokes
time steps + one two-pass projection against the current Krylov basis.  W warm-up steps, EXACTLY K timed steps
(`value` = K / time).  At N = 1 the factorisation is then continued to k_dim = 128 so that `wall_time_kdim_s` (sum of the
per-step wall times of Arnoldi steps 1..128, warm-up included) and a converged `leading_ritz` are always in the record.

N > 1: ONE eigenproblem, elements sharded over the N ranks (one process per GPU), dssum / Schwarz halos and reductions on
RCCL over xGMI, the same operator as at N = 1 (projection space included): "strong" scaling of the
headline configuration.  `--case cfg3` selects BASELINE configs[2] instead (2x2-refined mesh, E=7984, lx1=12) at ANY N,
N = 1 included, so that a series `--case cfg3 --gpus 1,2,4` is one curve too; the default N > 1 record also carries a short
sharded run of cfg3 next to the same steps on one GPU (`config3_sharded`).  The sharded step is first tried as ONE captured
hipGraph per step class (RCCL calls inside the graph); if that attempt fails or stalls, the run is repeated with eager
launches in FRESH processes.  A sharded run that fails both ways prints an error record (`value` null) and exits non-zero:
there is no silent fallback to another workload.  `python bench.py --gpus N` spawns its own N ranks (before anything touches
the GPU); under torch.distributed.run every launcher rank supervises one worker process.  `--replicas` runs N independent
copies of the N = 1 workload instead ("weak").
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

K_DIM = 128
WATCHDOG_S = 2400          # N > 1 only: the whole run
PROBE_S = 420              # N > 1 only: communicator set-up + the two-step probe map of the sharded path


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed Arnoldi steps (default 128 at N=1 on cfg2, 2 on cfg4, 8 otherwise)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-steps", type=int, default=8, help="--case cfg5: time steps per (truncated) map")
    ap.add_argument("--case", choices=["cfg2", "cfg3", "cfg4", "cfg5"], default="cfg2", help="workload: BASELINE configs[1] (default, the metric's configuration), configs[2] at any N, or configs[3] (backward-facing step extruded to E = 50 100 hexahedra, adjoint) on one GPU")
    ap.add_argument("--lx1", type=int, default=None)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kdim", action="store_true", help="do not continue the factorisation to k_dim = 128 after the timed steps")
    ap.add_argument("--extras", action="store_true", help="N=1: AFTER the record is printed, run the optional diagnostics (step-time budget from back-to-back kernel timings, the same build at earlier rounds' solver settings) and write them to --extras-out; never part of the record")
    ap.add_argument("--extras-out", default=os.path.join(ROOT, "gpurun_out", "bench_extras.json"))
    ap.add_argument("--no-fortran-host", action="store_true", help="N=1: skip the timing leg of the flang-built host loop (host/arnoldi_host) over the same library")
    ap.add_argument("--optional-budget-s", type=float, default=420.0, help="N=1: wall-clock bound of everything after the timed steps; when it runs out the record is printed with what is there")
    ap.add_argument("--no-cfg3-probe", action="store_true", help="N>1: skip the short sharded run of cfg3 next to the headline workload")
    ap.add_argument("--replicas", action="store_true", help="N>1: N independent replicas of the N=1 workload instead of one sharded eigenproblem")
    ap.add_argument("--whole-mesh-setup", action="store_true", help="N>1: every rank builds the whole-mesh context and cuts its shard from it (default: rank-local set-up, whole-mesh in the retry attempt)")
    ap.add_argument("--shard-graph", type=int, default=-1, help="N>1: 1 = captured step graphs only, 0 = eager only, -1 = graphs first, eager retry in fresh processes")
    from nekstab_amd.settings import PRODUCTION, PRODUCTION_OPTIONS      # the settings tests/test_spectrum_pin_gpu.py pins
    ap.add_argument("--tol-helm", type=float, default=PRODUCTION["tol_helm"])
    ap.add_argument("--tol-pres", type=float, default=PRODUCTION["tol_pres"])
    ap.add_argument("--min-pres", type=int, default=PRODUCTION_OPTIONS["min_pres_iter"], help="minimum GMRES iterations per pressure solve")
    ap.add_argument("--pres-cap", type=int, default=0, help="upper bound of GMRES iterations per pressure solve in time steps >= 4 (0 = none)")
    ap.add_argument("--nproj", type=int, default=PRODUCTION["nproj"], help="pressure projection space (residualProj)")
    ap.add_argument("--fused", type=int, default=-1, help="persistent velocity solve: 1 / 0 / -1 = library default")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline (0 = all host cores)")
    ap.add_argument("--cpu-baseline-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-preflight", action="store_true", help="N>1 over RCCL: skip the two-form RCCL check (tests/mp_rccl_worker.py in fresh processes) in front of the timed run")
    ap.add_argument("--ref-logfile", default=None, help="a logfile of a nekStab run of the same case (its 'Time per iteration' lines, core/krylov_decomposition.f:92-98, and Nek5000's step lines): the record gains `reference_logfile` with the reference's own matvecs/s")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run every optional section of the record (k_dim continuation, Ritz pair, byte accounting, rooflines, CPU baseline, Fortran host, one-GPU comparison and cfg3 run at N>1); a plain run times the steps and prints the headline only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed in its last step as DIR/<name>.npy (float64, at most 64 MB in all: larger outputs as a fixed, seeded sample of elements): the Hessenberg matrix and the new Krylov vector (krylov_*; cfg5: the map's output, map_*); a sharded run (N>1) writes the Hessenberg matrix only, as no rank holds the whole vector, so its outputs compare with an N=1 run's hessenberg.npy alone")
    a = ap.parse_args()
    if a.extras or a.ref_logfile:
        a.full = True
    return a


METRIC = "Arnoldi matvecs/sec + wall-time to k_dim=128 eigenpairs, cylinder Re=50"


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


NO_GPU_EXIT = 7            # a worker found no GPU: nothing a second attempt could change (unique: the supervisor stops on it)
STALL_EXIT = 5             # a worker's watchdog fired (stalled exchange / a rank waiting for one that failed): the next attempt runs
FAIL_EXIT = 4              # a worker failed and every rank agreed on it (all_ok)
C3_PROBE_S = 600           # N > 1 only: the short sharded run of cfg3 behind the headline workload


def supervise(a):
    """N > 1.  This process never touches the GPU: it starts worker processes (NSK_BENCH_WORKER=1) and waits.
    Without a launcher it starts all N ranks; under torch.distributed.run (RANK / WORLD_SIZE in the environment) it starts
    the ONE worker of its rank.  Attempts: captured step graphs first, then -- in fresh processes, on a fresh rendezvous
    port -- eager launches.  Every rank's supervisor sees the same outcome (the workers agree on success through an
    all-reduce before any of them prints), so all supervisors move to the next attempt together."""
    under_launcher = "WORLD_SIZE" in os.environ
    world = int(os.environ["WORLD_SIZE"]) if under_launcher else a.gpus
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks" % (a.gpus, world))
    ranks = [int(os.environ["RANK"])] if under_launcher else list(range(world))
    base_port = int(os.environ.get("MASTER_PORT", "0")) if under_launcher else _free_port()
    modes = [1, 0] if a.shard_graph < 0 else [a.shard_graph]
    if a.replicas:
        modes = [0]
    # ---- pre-flight: before the timed run, FRESH child processes run the two-GPU RCCL check of the test
    # suite (tests/mp_rccl_worker.py: a sharded map with the all-reduce inside the halo messages' RCCL group, then with separate
    # calls, and nsk_orth across the ranks, each against the single-rank result).  The grouped form had never executed between
    # two GPUs when this was written: if it fails (wrong numbers, an error, a stall) and the separate calls pass, the timed run
    # takes rccl_fuse = 0 and the record says so.
    preflight = None
    ngpu = 0
    wants_preflight = not a.replicas and not a.no_preflight and os.environ.get("NSK_DIST_BACKEND", "nccl") == "nccl"
    if wants_preflight:                                     # (dry runs over gloo never count the devices)
        try:
            import torch
            ngpu = torch.cuda.device_count()
        except Exception:                                   # noqa: BLE001
            pass
    if wants_preflight and ngpu >= world:
        preflight = rccl_preflight(world, ranks, under_launcher, base_port)
        print("bench.py supervisor: RCCL pre-flight: %s" % json.dumps(preflight), file=sys.stderr, flush=True)
    rc = 1
    for att, mode in enumerate(modes):
        procs = []
        for r in ranks:
            env = dict(os.environ, NSK_BENCH_WORKER="1", NSK_BENCH_PREFLIGHT=json.dumps(preflight) if preflight else "", NSK_BENCH_SHARD_GRAPH=str(mode), NSK_BENCH_ATTEMPT=str(att), RANK=str(r),
                       LOCAL_RANK=os.environ.get("LOCAL_RANK", str(r)) if under_launcher else str(r), WORLD_SIZE=str(world),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(base_port + (23 + att if under_launcher else att)),
                       HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            env.pop("TORCHELASTIC_USE_AGENT_STORE", None)       # the workers of an attempt rendezvous on their own store (fresh port)
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
        rc = 0
        for p in procs:
            rc = max(rc, abs(p.wait()))
        if rc == 0:
            return 0
        if rc == NO_GPU_EXIT:                                   # nothing a second attempt could change (a stall, STALL_EXIT, is what the retry is for)
            break
        print("bench.py supervisor: attempt %d (%s) failed with code %d%s" % (att, "captured step graphs" if mode else "eager launches", rc,
              ": retrying with eager launches in fresh processes" if att + 1 < len(modes) else ""), file=sys.stderr, flush=True)
    if 0 in ranks:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "matvecs/s", "n_gpus": world, "error": "the sharded run failed in every attempt (see stderr)"}), flush=True)
    return rc or 1


def rccl_preflight(world, ranks, under_launcher, base_port):
    """Run tests/mp_rccl_worker.py on `world` ranks (one GPU each) in fresh processes: grouped all-reduce + halos (rccl_fuse = 1),
    then separate calls (0).  Returns {"fuse1": ok / error, "fuse0": ..., "rccl_fuse": the form the timed run should take}."""
    worker = os.path.join(ROOT, "tests", "mp_rccl_worker.py")
    res = {}
    for k, fuse in enumerate(("1", "0")):
        procs = []
        for r in ranks:
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=os.environ.get("LOCAL_RANK", str(r)) if under_launcher else str(r), WORLD_SIZE=str(world),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(base_port + (47 + k if under_launcher else 11 + k)), NSK_PREFLIGHT_FUSE=fuse,
                       HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            env.pop("TORCHELASTIC_USE_AGENT_STORE", None)
            procs.append(subprocess.Popen([sys.executable, worker], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        ok, note = True, ""
        for p in procs:
            try:
                so, se = p.communicate(timeout=420)
            except subprocess.TimeoutExpired:
                p.kill(); so, se = p.communicate()
                ok, note = False, "stalled (420 s)"
                continue
            if p.returncode != 0:
                ok, note = False, (note or ("exit code %d: %s" % (p.returncode, (se or so)[-200:].replace("\n", " "))))
            for l in so.splitlines():
                if l.startswith("MPRCCL errors"):
                    note = l[len("MPRCCL errors"):].strip()
        res["fuse" + fuse] = {"ok": ok, "note": note}
        if ok and fuse == "1":
            break                                            # the grouped form works: nothing else to try
    res["rccl_fuse"] = 1 if res.get("fuse1", {}).get("ok") else 0
    if not res.get("fuse1", {}).get("ok") and not res.get("fuse0", {}).get("ok", False):
        res["warning"] = "the RCCL check failed with grouped AND separate all-reduces: the timed run is attempted anyway (its own retry and watchdog apply)"
    return res


def cpu_baseline(case, threads, tol, nproj, gpu_value, q_sample=None, lx1=None):
    """The CPU baseline in a CHILD process with the OpenMP environment a CPU run would use (libgomp reads it when it is loaded):
    threads bound to cores, close to each other, spinning between the (many, short) parallel regions -- measured on the GPU box's
    256-core host (profiles/r06_cpu_scaling_v0.txt: ms per time step at 8 / 16 / 32 / 64 threads): 32.6 / 30.6 / 30.0 / 44.8 with
    the passive, unbound settings rounds 2-5 timed, 18.7 / 12.7 / 13.0 / 35.2 with OMP_WAIT_POLICY=active OMP_PROC_BIND=close
    OMP_PLACES=cores.  The child never touches the GPU; the Krylov vector of the sample travels in a temporary .npz."""
    import tempfile
    import numpy as np
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "q.npz")
        if q_sample is not None:
            np.savez(f, *[np.asarray(x, dtype=np.float64) for x in q_sample])
        env = dict(os.environ, OMP_WAIT_POLICY="active", OMP_PROC_BIND="close", OMP_PLACES="cores", GOMP_SPINCOUNT="infinite")
        env.pop("OMP_NUM_THREADS", None)
        try:
            visible = len(os.sched_getaffinity(0))
        except AttributeError:
            visible = os.cpu_count() or 1
        spec = json.dumps({"visible": visible, "lx1": lx1 or case.lx1, "threads": threads, "tol": list(tol), "nproj": nproj, "gpu_value": gpu_value, "q": f if q_sample is not None else None})
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", spec], env=env, capture_output=True, text=True, timeout=900)
        sys.stderr.write(r.stderr[-4000:])
        line = [l for l in r.stdout.splitlines() if l.startswith("CPU_BASELINE ")]
        if r.returncode != 0 or not line:
            raise RuntimeError("CPU baseline child failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-300:]))
        out = json.loads(line[-1][len("CPU_BASELINE "):])
        out["openmp_environment"] = {k: env[k] for k in ("OMP_WAIT_POLICY", "OMP_PROC_BIND", "OMP_PLACES")}
        return out


def _cpu_baseline_child(spec):
    sp = json.loads(spec)
    import numpy as np
    case = build_case("cfg2", sp["lx1"] if sp["lx1"] != 8 else None)
    q = None
    if sp["q"]:
        z = np.load(sp["q"])
        q = tuple(z[k] for k in z.files)
    out = _cpu_baseline_impl(case, sp["threads"], tuple(sp["tol"]), sp["nproj"], sp["gpu_value"], q, visible=sp.get("visible"))
    print("CPU_BASELINE " + json.dumps(out), flush=True)


def _cpu_baseline_impl(case, threads, tol, nproj, gpu_value, q_sample=None, visible=None):
    """The CPU port of the same step (oracle/cpu_step.c: C + OpenMP, the same PCG / GMRES + Schwarz + coarse algorithms,
    tolerances AND pressure projection space as the GPU path) timed on the host cores of the GPU box.  Thread count: the
    fastest of {8, 16, 32, 64} (capped at the visible cores) on a short calibration.  Bounded samples (about 25 s of CPU work
    in all): as many time steps of ONE matvec as fit the bound, extrapolated to the nsteps of a matvec; the input is the Krylov vector
    the FIRST TIMED GPU step mapped (downloaded from the device: the same work as `value` measures; the noise seed itself needs
    1.7x the velocity iterations of a Krylov vector) --
    (a) with the projection space (like for like with `value`), (b) without it (what rounds 1-4 reported), (c) on 4 threads
    for BASELINE configs[0] (k_dim = 32 on 4 CPU ranks)."""
    import numpy as np
    from nekstab_amd import seed
    from oracle.cpu_port import CpuPort
    from oracle.linns import LinNS2D
    log = lambda *x: print("[bench cpu_baseline]", *x, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    o = LinNS2D(x=case.x, y=case.y, gid=case.gid, nglob=case.nglob, mask=case.mask, ub=case.ub, spng=case.spng, re=case.re,
                endtime=case.endtime, lxd=case.lxd, has_outflow=case.has_outflow, factorize_pressure=False)
    kw = dict(tol_helm=tol[0], tol_pres=tol[1], tol_relative=1, min_pres=tol[2])
    cp = CpuPort(o, case.meta["vert"], case.meta["nvert"], nproj=nproj, **kw)
    setup = time.perf_counter() - t0
    log("set-up %.1f s" % setup)
    if q_sample is not None:
        q0 = tuple(np.asarray(a, dtype=np.float64) for a in q_sample)
        what_vec = "the Krylov vector the first timed GPU step mapped (projection space empty at the start of the sample)"
    else:
        qx, qy = seed.add_noise(case)
        q0 = (qx, qy, np.zeros((case.nel, case.lx1 - 2, case.lx1 - 2)))
        what_vec = "noise-seed vector"
    if visible is None:                                     # (with OMP_PROC_BIND libgomp pins the main thread: the parent counts the cores)
        try:
            visible = len(os.sched_getaffinity(0))
        except AttributeError:
            visible = os.cpu_count() or 1
    # candidates in ascending order, at most 64 threads: this problem has 128 k points per field, and with one thread per
    # visible core of a 256-core host a time step takes 67 s instead of 35 ms (measured in round 2)
    cands = [threads] if threads else sorted({min(visible, 8), min(visible, 16), min(visible, 32), min(visible, 64)})
    best = None
    calib, floor = {}, {}
    for nt in cands:                                        # calibration: one time step, then three more unless it is already hopeless
        cp.set_threads(nt)
        cp.proj_reset()
        t0 = time.perf_counter(); cp.matvec(q0, nsteps=1); t = time.perf_counter() - t0
        if best is not None and t > 3.0 * best[1]:
            log("calibration: %d threads %.1f ms for the first time step: skipped" % (nt, 1e3 * t))
            continue
        t0 = time.perf_counter(); cp.matvec(q0, nsteps=4); t = (time.perf_counter() - t0) / 4
        log("calibration: %d threads %.1f ms per time step" % (nt, 1e3 * t))
        calib[str(nt)] = 1e3 * t
        try:                                                # the fork-join floor at this thread count: regions per time step x an empty region
            cp.regions(reset=True); cp.proj_reset(); cp.matvec(q0, nsteps=2); nreg = cp.regions() / 2.0
            er = cp.empty_region_us()
            floor[str(nt)] = {"parallel_regions_per_time_step": nreg, "empty_region_us": er, "fork_join_floor_ms_per_time_step": 1e-3 * nreg * er}
            log("             %d threads: %.0f parallel regions per time step x %.1f us per empty region = %.1f ms" % (nt, nreg, er, 1e-3 * nreg * er))
        except Exception as e:                              # noqa: BLE001
            floor[str(nt)] = {"error": repr(e)[:200]}
        if best is None or t < best[1]:
            best = (nt, t)

    def sample(port, nt, per_step_guess, bound):
        port.set_threads(nt)
        port.proj_reset()
        ns = int(min(port.nsteps, max(8, bound / max(per_step_guess, 1e-4))))
        t0 = time.perf_counter(); port.matvec(q0, nsteps=ns); dt_ = time.perf_counter() - t0
        t = dt_ / ns * port.nsteps
        what = ("one whole matvec (%d time steps)" % ns) if ns == port.nsteps else \
               "the first %d of the %d time steps of one matvec, extrapolated (bound %.0f s of CPU work)" % (ns, port.nsteps, bound)
        log("%d threads, nproj %d: %.2f s per matvec (%s), %.2f pressure iterations per step" % (nt, port.case.nproj, t, what, port.stats["pres_iters"] / port.stats["steps"]))
        return {"threads": nt, "s_per_matvec": t, "matvecs_per_s": 1.0 / t, "sample": what, "sample_seconds": dt_,
                "helm_iters_per_step": port.stats["helm_iters"] / port.stats["steps"], "pres_iters_per_step": port.stats["pres_iters"] / port.stats["steps"]}

    a = sample(cp, best[0], best[1], 12.0)
    cp0 = CpuPort(o, case.meta["vert"], case.meta["nvert"], nproj=0, **kw)
    b = sample(cp0, best[0], best[1], 6.0)
    n4 = min(4, visible)
    c4 = sample(cp, n4, best[1] * best[0] / n4, 6.0)
    return {"value": a["matvecs_per_s"], "unit": "matvecs/s", "cores": a["threads"], "cores_used": a["threads"], "cores_visible": visible, "kind": "port",
            "thread_calibration_ms_per_time_step": calib, "fork_join_floor": floor,
            "thread_scaling_note": "fastest thread count of the calibration; MEASURED reason why more threads do not pay (fork_join_floor): a time step of this case "
                                   "opens several hundred OpenMP parallel regions over 127 744 points (two Helmholtz components solved one after the other, modified "
                                   "Gram-Schmidt with two regions per basis vector); regions per time step x the measured cost of an EMPTY region at the same thread "
                                   "count is the floor no amount of cores removes, and it grows with the team; profiles/r06_cpu_scaling_v0.txt has the same table with and without binding",
            "sample": ("%s of the same case (lx1=%d, E=%d), " + what_vec + "; oracle/cpu_step.c (C + OpenMP: Jacobi-PCG, GMRES + restricted Schwarz + vertex coarse "
                       "solve, tolerances %g / %g and a %d-vector pressure projection space as the GPU run); the Krylov projection (0.2 %% of a GPU step) is not in the sample; "
                       "%d cores visible; set-up %.0f s excluded") % (a["sample"], case.lx1, case.nel, tol[0], tol[1], nproj, visible, setup),
            "gpu_over_cpu": gpu_value / a["matvecs_per_s"],
            "wall_time_kdim_s_projected": a["s_per_matvec"] * K_DIM,
            "iterations": {k: v for k, v in a.items() if k.endswith("per_step")},
            "without_projection_space": {"matvecs_per_s": b["matvecs_per_s"], "threads": b["threads"], "sample": b["sample"],
                                         "iterations": {k: v for k, v in b.items() if k.endswith("per_step")},
                                         "note": "the algorithm rounds 1-4 reported as cpu_baseline (their C port had no projection space)"},
            "config1_k32_4threads": {"matvecs_per_s": c4["matvecs_per_s"], "threads": c4["threads"],
                                     "wall_time_k32_s_projected": c4["s_per_matvec"] * 32, "sample": c4["sample"]}}


def parse_reference_logfile(path):
    """A true reference number, when somebody has one: the per-iteration timing a nekStab run prints (the only route to it here:
    Nek5000 is not vendored in the reference tree).  arnoldi_factorization writes, per Arnoldi step,
        ' iteration current and total:  <mstep> / <mend>'                                   (core/krylov_decomposition.f:75)
        ' Time per iteration/remaining:  0h  1min /  0h 14min'                              (core/krylov_decomposition.f:92-98)
    -- whole minutes, ROUNDED UP (ceiling) -- and Nek5000 writes one line per time step in between,
        'Step    100, t= 1.0000000E+00, DT= 1.0000000E-02, C=  0.494 2.2841E+00 2.1910E-02'     (elapsed seconds, seconds of the step)
    When the step lines are there, an iteration's wall time is the sum of its steps' seconds (exact); otherwise the minute lines
    give an upper bound of the time = a lower bound of matvecs/s.  Returns a dict for the record."""
    import re
    it_re = re.compile(r"iteration current and total:\s*(\d+)\s*/\s*(\d+)")
    tm_re = re.compile(r"Time per iteration/remaining:\s*(\d+)h\s*(\d+)min")
    st_re = re.compile(r"^\s*Step\s+(\d+),\s*t=\s*([-+0-9.eEdD]+),\s*DT=\s*([-+0-9.eEdD]+),\s*C=\s*([-+0-9.eEdD]+)\s+([-+0-9.eEdD]+)\s+([-+0-9.eEdD]+)")
    iters, cur = [], None
    with open(path, errors="replace") as fh:
        for line in fh:
            m = it_re.search(line)
            if m:
                cur = {"mstep": int(m.group(1)), "mend": int(m.group(2)), "step_s": 0.0, "steps": 0, "minutes": None}
                iters.append(cur)
                continue
            if cur is None:
                continue
            m = st_re.match(line)
            if m and cur["minutes"] is None:
                cur["step_s"] += float(m.group(6).replace("D", "E").replace("d", "e")); cur["steps"] += 1
                continue
            m = tm_re.search(line)
            if m:
                cur["minutes"] = 60 * int(m.group(1)) + int(m.group(2))
    done = [i for i in iters if i["minutes"] is not None]
    if not done:
        return {"path": path, "error": "no completed Arnoldi iteration ('Time per iteration/remaining:' line) found"}
    out = {"path": path, "iterations": len(done), "k_dim": done[-1]["mend"], "time_steps_per_iteration": float(sum(i["steps"] for i in done)) / len(done)}
    if all(i["steps"] > 0 for i in done):
        t = sum(i["step_s"] for i in done) / len(done)
        out.update({"s_per_iteration": t, "matvecs_per_s": 1.0 / t, "resolution": "exact: the seconds Nek5000 prints per time step, summed over the steps of an Arnoldi iteration"})
    else:
        t = 60.0 * sum(i["minutes"] for i in done) / len(done)
        out.update({"s_per_iteration_upper_bound": t, "matvecs_per_s_lower_bound": (1.0 / t) if t > 0 else None,
                    "resolution": "whole minutes rounded up ('Time per iteration' lines only: core/krylov_decomposition.f:92-98): an upper bound of the time"})
    return out


def fortran_host_leg(case, seed_state, a, steps, py_value):
    """north_star: the outer Arnoldi loop stays in Fortran on the host.  host/arnoldi_host (flang; host/krylov_host.f90 over
    host/nekstab_hip_mod.f90) runs the same warm-up + timed Arnoldi steps on the same library in a child process and prints the
    reference's per-iteration timing line (core/krylov_decomposition.f:92-98) with the wall seconds of the step; this leg
    reports matvecs/s over the timed steps next to the Python host's."""
    import tempfile
    import numpy as np
    from nekstab_amd.casefile import write_case_bin
    exe = os.path.join(ROOT, "host", "arnoldi_host")
    if not os.path.exists(exe):
        return {"error": "host/arnoldi_host not built (flang absent when __graft_entry__.build() ran)"}
    kd = a.warmup + steps
    with tempfile.TemporaryDirectory() as td:
        cb = os.path.join(td, "case.bin")
        write_case_bin(cb, case, seed_state, settings={"tol_helm": a.tol_helm, "tol_pres": a.tol_pres, "min_pres_iter": a.min_pres, "nproj": a.nproj, "max_helm_iter": 100})
        t0 = time.perf_counter()
        r = subprocess.run([exe, cb, str(kd), td], capture_output=True, text=True, timeout=300)
        wall = time.perf_counter() - t0
    if r.returncode != 0:
        return {"error": "arnoldi_host exited with %d: %s" % (r.returncode, (r.stderr or r.stdout)[-300:])}
    ts = [float(l.split("step_wall_s=")[1]) for l in r.stdout.splitlines() if "step_wall_s=" in l]
    if len(ts) < kd:
        return {"error": "arnoldi_host printed %d of %d timing lines" % (len(ts), kd)}
    t = float(np.sum(ts[a.warmup:kd]))
    return {"matvecs_per_s": steps / t, "ms_per_step": 1e3 * t / steps, "steps": steps, "warmup": a.warmup, "vs_python_host": (steps / t) / py_value,
            "process_wall_s": wall, "host": "host/arnoldi_host (flang): arnoldi_factorization of host/krylov_host.f90 calling nsk_matvec / nsk_orth through iso_c_binding; "
                                            "per-step wall time from the reference's 'Time per iteration' line (core/krylov_decomposition.f:92-98)"}


def run_extras(a, case, full, seed_state, stats, step_s, out, extras):
    """--extras: diagnostics that are NOT part of the record (they run after it is printed)."""
    import numpy as np
    import torch
    from nekstab_amd import krylov
    from nekstab_amd.capi import NekStabHip
    qx, qy, zp = seed_state
    steps = out["steps"]
    # How much of a time step is kernel time at all ("latency-bound" as a number): the step's kernels timed back to back
    # with HIP events (every launch doing full work) x the launches the logged iteration counts imply, against the wall
    # time of a step.  The rest is kernel boundaries, launches that find their solve converged and host gaps.
    try:
        hit, pit = out["helm_iters_per_step"], out["pres_iters_per_step"]
        st = full.stats()
        kt = {kn: full.bench_kernel(kn, 100)["avg_us"] for kn in ("helm", "convect", "rhs", "pres_rhs", "proj_apply_e", "schwarz_uc3", "divgs_t", "pres_update", "vel_update_proj", "proj_update")}
        per = {"velocity solve (k_helm x (iterations + 1))": kt["helm"] * (hit + 1.0),
               "pressure iterations (k_schwarz_uc + k_divgs_t per iteration: round 6, two launches)": (kt["schwarz_uc3"] + kt["divgs_t"]) * pit,
               "once per step (convect, rhs, pres_rhs, proj_apply_e, pres_update, vel_update_proj, proj_update)":
                   kt["convect"] + kt["rhs"] + kt["pres_rhs"] + kt["proj_apply_e"] + kt["pres_update"] + kt["vel_update_proj"] + kt["proj_update"]}
        wall_us = 1e3 * out["ms_per_time_step"]
        extras["step_time_budget"] = {"wall_us_per_time_step": wall_us, "kernel_us": kt, "kernel_us_back_to_back": per, "busy_fraction": sum(per.values()) / wall_us,
                                      "budgeted_launches_per_step": {"helm": st["budget_helm"], "pres": st["budget_pres"]},
                                      "note": "kernel durations from nsk_bench_kernel (HIP events, back to back, full-work launches); busy_fraction = their sum / wall time of a step"}
    except Exception as e:                                  # noqa: BLE001
        extras["step_time_budget"] = {"error": repr(e)[:300]}

    # The same build at the inner-solver settings earlier records were quoted on: 24 timed Arnoldi steps each, after 4 warm-up steps.
    def rate(tol_helm, tol_pres, nproj, opts, tol_relative=1):
        hc = NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=tol_helm, tol_pres=tol_pres, tol_relative=tol_relative,
                        schwarz_layers=2, max_helm_iter=100, max_pres_iter=48, nproj=nproj)
        try:
            for k, v in opts.items():
                hc.set_option(k, v)
            Qc = hc.alloc(30)
            hc.upload(Qc[0], qx, qy, zp)
            hc.scal(Qc[0], 1.0 / hc.norm(Qc[0]))
            Hc = np.zeros((30, 29)); sc_ = {}
            krylov.arnoldi_factorization(hc, Qc, Hc, 1, 4, 0, stats=sc_)
            torch.cuda.synchronize(); t0c = time.perf_counter()
            krylov.arnoldi_factorization(hc, Qc, Hc, 5, 28, 0, stats=sc_)
            torch.cuda.synchronize(); dtc = time.perf_counter() - t0c
            stc = hc.stats()
        finally:
            hc.close()
        return {"matvecs_per_s": 24 / dtc, "helm_iters_per_step": stc["total_helm_iters"] / max(stc["total_steps"], 1),
                "pres_iters_per_step": stc["total_pres_iters"] / max(stc["total_steps"], 1), "capped_solves": stc["total_capped_solves"]}
    try:
        extras["same_build_other_settings"] = {
            "note": "Arnoldi steps 5-28 of the same case; NOT the headline: these settings do not hold the 5e-6 parity bound on the wake rows (DESIGN.md section 1)",
            "this_run_same_window": {"matvecs_per_s": 24.0 / float(np.sum(step_s[4:28])) if len(step_s) >= 28 else None, "settings": "production (as `value`)"},
            "round1_bench_settings": dict(rate(1e-9, 3e-1, 8, {"min_pres_iter": 2, "pres_cap": 4}), settings="1e-9 / 3e-1, 2-4 GMRES iterations, 8 projection vectors (BENCH_r01: 15.2 matvecs/s)"),
            "round2_initial_settings": dict(rate(1e-11, 1e-1, 16, {"min_pres_iter": 2}), settings="1e-11 / 1e-1, at least 2 GMRES iterations, 16 projection vectors (9.78 matvecs/s at the start of round 2)"),
            "production_without_projection_space": dict(rate(a.tol_helm, a.tol_pres, 0, {"min_pres_iter": a.min_pres}), settings="production tolerances, NO projection space"),
            "nek5000_own_solver_semantics": dict(rate(1e-9, 1e-7, 20, {"helm_guess": 0, "min_pres_iter": 1}, tol_relative=0),
                                                 settings="the reference's 1cyl.par:27-35 taken literally: ABSOLUTE residual tolerances 1e-9 (velocity) / 1e-7 (pressure) in Nek5000's norms, zero initial guess, "
                                                          ">= 1 GMRES iteration, 20 projection vectors -- on unit-norm Krylov vectors these stop after ~1 pressure iteration per step; the wake rows of the spectrum move by up to 1.3e-3 at these settings (profiles/r06_wake_rows.json): not parity settings"),
            "production_three_launch_iteration": dict(rate(a.tol_helm, a.tol_pres, a.nproj, {"min_pres_iter": a.min_pres, "fuse2": 0}), settings="production settings with option fuse2 = 0: the pressure GMRES iteration as the three launches of rounds 3-5 (k_update_coarse, k_schwarz, k_divgs)"),
            "production_two_launch_iteration": dict(rate(a.tol_helm, a.tol_pres, a.nproj, {"min_pres_iter": a.min_pres}), settings="production settings (as `value`: k_schwarz_uc + k_divgs_t), same window, for the A/B with the line above"),
        }
    except Exception as e:                                  # noqa: BLE001
        extras["same_build_other_settings"] = {"error": repr(e)[:300]}


KERNEL_FAMILIES = {"2d": ("nsk_kernels.hpp", "nsk_persist.hpp", "nsk_dev.hpp", "nsk_basis.hpp", "nsk_crtrig.hpp"),
                   "3d": ("nsk3_kernels.hpp", "nsk3_mfma.hpp", "nsk3_mfma_ops.hpp", "nsk_dev.hpp")}


def family_hashes():
    """sha256 of the kernel SOURCES of the quadrilateral and of the hexahedral kernel set (the headers the kernels live in): what the
    HBM-side bytes of a launch depend on.  A PMC table stays valid for a kernel family whose sources did not change, even when the
    library was rebuilt for a host-side change or for the other family (its full source hash then differs)."""
    import hashlib
    out = {}
    for fam, files in KERNEL_FAMILIES.items():
        h = hashlib.sha256()
        for f in files:
            with open(os.path.join(ROOT, "nekstab_amd", "csrc", f), "rb") as fh:
                h.update(fh.read())
        out[fam] = h.hexdigest()
    return out


def pmc_traffic(kernel_key):
    """HBM-side bytes per launch of the dominant kernel from the committed PMC passes (scripts/profile_r06.sh ->
    profiles/rNN_pmc_traffic.json): used only when the file was produced by THIS build of the library (full source hash) or, for
    a table that records them, by a build with the same sources of the kernel's FAMILY (family_hashes)."""
    import glob
    stamp = os.path.join(ROOT, "nekstab_amd", "lib", "libnekstab_hip.so.srchash")
    if not os.path.exists(stamp):
        return None, "no PMC pass of this build"
    mine = open(stamp).read().strip()
    fam = "3d" if kernel_key.startswith("k3::") else "2d"
    famh = family_hashes()[fam]
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
        tab = json.load(open(path))
        if tab.get("srchash") != mine and (tab.get("family_hash") or {}).get(fam) != famh:
            continue
        rec = tab.get("kernels", {}).get(kernel_key)
        if not rec:
            return None, "kernel not in the PMC table of " + os.path.basename(path)
        same = "this build" if tab.get("srchash") == mine else "a build with the same %s kernel sources" % ("hexahedral" if fam == "3d" else "quadrilateral")
        return rec["bytes_per_launch"], "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of %s (2 x FETCH_SIZE + WRITE_SIZE, gfx950 correction): profiles/%s" % (same, os.path.basename(path))
    return None, "the committed PMC tables (profiles/r*_pmc_traffic.json) are from other builds of the library"


DUMP_BYTES = 64 << 20


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy (float64) per output of the timed path's last step.  When they exceed 64 MB together,
    every array whose first axis is the element index keeps the same fixed, seeded sample of elements (sorted), so two builds
    are compared output for output."""
    import numpy as np
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_BYTES:
        nel = max(v.shape[0] for v in arrays.values())
        big = sum(v.nbytes for v in arrays.values() if v.shape[0] == nel)
        keep = int(nel * (DUMP_BYTES - (1 << 16) - (total - big)) / big)       # (64 kB for the .npy headers)
        rows = np.sort(np.random.default_rng(20240611).choice(nel, size=keep, replace=False))
        arrays = {k: (v[rows] if v.shape[0] == nel else v) for k, v in arrays.items()}
    os.makedirs(dirname, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), np.ascontiguousarray(v))
    print("[bench] outputs of the last timed step: %s in %s" % (", ".join("%s %s" % (k, v.shape) for k, v in arrays.items()), dirname), file=sys.stderr, flush=True)


def vector_outputs(ctx, v, prefix, hexa):
    """The fields of one state vector on the host: {prefix_u, prefix_v, [prefix_w,] prefix_p}."""
    f = ctx.download3(v) if hexa else ctx.download(v)
    names = ("u", "v", "w", "p") if hexa else ("u", "v", "p")
    return {prefix + "_" + n: a for n, a in zip(names, f)}


def build_case(name, lx1_override=None):
    from nekstab_amd import mesh
    if name == "cfg4":
        # BASELINE configs[3]: the reference's backward-facing step (examples/back_fstep, Re = 500) extruded over 30 periodic
        # spanwise layers: E = 50 100 hexahedra, lx1 = 8, 25.65 M points per field, state vector 702 MB; adjoint Arnoldi
        from nekstab_amd import mesh3d
        nz = int(os.environ.get("NSK_BENCH_CFG4_LAYERS", "30"))      # (tests run a thin slab)
        c2 = mesh.load_case_npz(os.path.join(ROOT, "tests", "golden", "backstep_case.npz"), lx1_override or 8, re=500.0, endtime=1.0, xlspg=5.0, xrspg=10.0, spng_str=2.0)
        c3 = mesh3d.extrude_case(c2, nz, 0.2 * nz, periodic=True)
        c3.meta["c2"] = c2
        c3.meta["nz"] = nz
        return c3
    lx1 = lx1_override or (12 if name == "cfg3" else 8)
    case = mesh.load_case_npz(os.path.join(ROOT, "tests", "golden", "cylinder_case.npz"), lx1)
    if name == "cfg3":
        case = mesh.refine_case_2x2(case)                  # E = 7984 (BASELINE configs[2])
    return case


def run_cfg5(a):
    """--case cfg5: BASELINE configs[4]'s SIZE -- a lid-driven cube of 46 x 46 x 47 = 99 452 hexahedra with cav.box's wall clustering, lx1 = 10:
    99.5 M points per field, state vector 2.8 GB, ~175 GB of device memory on one GPU.  The line times `--steps` TRUNCATED maps of
    `--map-steps` time steps each after `--warmup` of them (a time step takes a second; the reference's case, T = 1 at its CFL, would be
    ~700 of them per map), reports ms_per_time_step, projects `value` = 1 / (ms_per_time_step x the steps of a whole map of THIS
    case's T) and carries the kernel roofline of k3::k_helm_p<10> (HIP events, full-work launches) with this build's PMC traffic.  An auxiliary line (the metric's configuration is configs[1]: the default run)."""
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    from nekstab_amd import mesh3d, roofline
    from nekstab_amd.capi import NekStabHip
    steps = a.steps if a.steps is not None else 2
    warm = a.warmup if a.warmup != 2 else 1
    stretch = lambda xi: 0.5 * (1.0 - np.cos(np.pi * xi))
    t0 = time.perf_counter()
    c = mesh3d.box_case_3d(46, 46, 47, 10, lengths=(1.0, 1.0, 1.0), re=1000.0, endtime=0.02, stretch=stretch)
    sx, sy, sz = np.sin(np.pi * c.x), np.sin(np.pi * c.y), np.sin(np.pi * c.z)
    c.ub[0] = sx ** 2 * np.sin(2 * np.pi * c.y) * sz ** 2 * c.mask
    c.ub[1] = -np.sin(2 * np.pi * c.x) * sy ** 2 * sz ** 2 * c.mask
    del sx, sy, sz
    nproj = 8
    h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], tol_helm=1e-9, tol_pres=1e-2, tol_relative=1, max_helm_iter=400, max_pres_iter=192, nproj=nproj)
    setup_s = time.perf_counter() - t0
    nfull = h.nsteps
    q, f = h.alloc(2)
    w = 1e-2 * np.sin(2 * np.pi * c.x) * np.sin(3 * np.pi * c.y) * np.sin(2 * np.pi * c.z) * c.mask      # a smooth three-dimensional perturbation
    h.upload3(q, c.ub[0] + w, c.ub[1] - w, w, np.zeros(h.npres))
    del w
    h.set_nsteps(a.map_steps)
    for _ in range(warm):
        h.matvec(f, q, 0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        h.matvec(f, q, 0)
    h.norm(f); torch.cuda.synchronize(); elapsed = time.perf_counter() - t0
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, vector_outputs(h, f, "map", True))
    st = h.stats()
    ms_ts = 1e3 * elapsed / (steps * a.map_steps)
    za = int(st.get("zero_arrays", 0))
    out = {"metric": METRIC, "value": 1.0 / (1e-3 * ms_ts * nfull), "unit": "matvecs/s", "n_gpus": 1, "steps": steps, "warmup": warm,
           "ms_per_step": 1e3 * elapsed / steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
           "data": "synthetic: a smooth three-dimensional perturbation of an analytic vortex on the box mesh (the reference's lid_driven case needs its 3-D base flow, which is not in the tree)",
           "value_note": "PROJECTED: 1 / (ms_per_time_step x %d time steps of a whole map); the timed maps are truncated to %d time steps" % (nfull, a.map_steps),
           "config": {"workload": "lid-driven cube at BASELINE configs[4]'s size: E=%d hexahedra (46 x 46 x 47, cav.box wall clustering), lx1=10, lxd=15, %d time steps per map (full map: %d); state vector %.2f GB"
                                  % (c.nel, a.map_steps, nfull, 8e-9 * h.nstate),
                      "tolerances": "Helmholtz 1e-9, pressure 1e-2 relative, projection space %d, host-read convergence flags" % nproj, "parallelism": "1 GPU"},
           "setup_s": setup_s, "ms_per_time_step": ms_ts, "helm_iters_per_step": st["helm_iters"] / max(st["steps"], 1), "pres_iters_per_step": st["pres_iters"] / max(st["steps"], 1),
           "zero_arrays": za}
    if not a.full:
        print(json.dumps(out), flush=True)
        h.close()
        return 0
    rule, distinct = roofline.helm_launch_bytes(nel=c.nel, lx1=10, ndim=3, zero_arrays=za)
    kr = h.bench_kernel("helm", 10)
    traffic, tnote = pmc_traffic("k3::helm<10>")
    out.update({
           "roofline": {"bound": "hbm", "kernel": "k3::k_helm_p<10> (one CG iteration of the three components: resident workgroups, the next element's vectors by LDS-DMA; 64-69 % of the kernel time of a time step: profiles/r06_cfg5_trace_summary.txt)", "achieved": distinct / kr["avg_us"] / 1e3, "peak": 8000.0, "unit": "GB/s",
                        "frac": distinct / kr["avg_us"] / 1e3 / 8000.0, "traffic": traffic, "traffic_source": tnote, "avg_launch_us": kr["avg_us"], "algorithmic_bytes_per_launch": distinct,
                        "survey_rule": {"algorithmic_bytes_per_launch": rule, "frac": rule / kr["avg_us"] / 1e3 / 8000.0},
                        "note": "every distinct array of the launch ONCE (the figure to quote); SURVEY 8(d)'s per-component rule counts the arrays the three components share three times: `survey_rule`, not a bandwidth"},
           "cpu_baseline": None, "cpu_baseline_note": "the C / OpenMP port covers quadrilaterals: the default record (configs[1]) carries the CPU baseline"})
    kt = {}
    for kn in ("divgs", "schwarz", "convect_mfma", "helm_wg"):
        try:
            kt[kn] = h.bench_kernel(kn, 10)["avg_us"]
        except Exception as e:                              # noqa: BLE001
            kt[kn] = repr(e)[:100]
    out["kernel_us"] = dict(kt, helm=kr["avg_us"])
    print(json.dumps(out), flush=True)
    h.close()
    return 0


def main():
    a = parse()
    if a.cpu_baseline_child:
        return _cpu_baseline_child(a.cpu_baseline_child)
    if a.case == "cfg5":
        if a.gpus > 1:
            raise SystemExit("bench.py --case cfg5: one GPU")
        return run_cfg5(a)
    if a.gpus > 1 and os.environ.get("NSK_BENCH_WORKER") != "1":
        raise SystemExit(supervise(a))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks" % (a.gpus, world))
    backend = os.environ.get("NSK_DIST_BACKEND", "nccl")   # "gloo": dry run of the N>1 protocol with all ranks on one GPU (host-staged halos)
    shard_graph = int(os.environ.get("NSK_BENCH_SHARD_GRAPH", "0"))
    if world > 1 and backend == "nccl":
        os.environ["HIP_VISIBLE_DEVICES"] = str(local)     # before anything touches the GPU
    if world > 1 and os.environ.get("NSK_BENCH_TEST_STALL") == os.environ.get("NSK_BENCH_ATTEMPT", "0"):
        # test hook (tests/test_host_cpu.py): this attempt's workers behave like a run whose first exchange never completes
        import threading
        threading.Timer(1.0, lambda: (print("bench.py rank %d: forced stall (test hook): giving up" % rank, file=sys.stderr, flush=True), os._exit(STALL_EXIT))).start()
        time.sleep(3600)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench.py needs a GPU: the hot path has no CPU fallback", file=sys.stderr, flush=True)
        raise SystemExit(NO_GPU_EXIT)
    dist = None
    if world > 1:
        # watchdog: a multi-rank run that stalls (an exchange that never completes) must not hang the caller for ever.  A
        # THREAD, not SIGALRM: a rank stuck inside a C call (hipStreamSynchronize behind a lost message) never runs a
        # Python signal handler, but ctypes releases the GIL, so a timer thread still fires.
        import threading

        def _stalled(what, limit):
            print("bench.py rank %d: %s: no result after %d s: giving up" % (rank, what, limit), file=sys.stderr, flush=True)
            os._exit(STALL_EXIT)
        wd = threading.Timer(WATCHDOG_S, _stalled, ("multi-rank run", WATCHDOG_S))
        wd.daemon = True
        wd.start()
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
        else:
            dist.init_process_group(backend)
    from nekstab_amd import krylov, roofline, seed
    from nekstab_amd.capi import NekStabHip

    sharded = world > 1 and not a.replicas
    headline = (a.case == "cfg2" and world == 1)
    hexa = a.case == "cfg4"
    if hexa and world > 1:
        raise SystemExit("bench.py --case cfg4: one GPU (the sharded hexahedral path is exercised by tests/test_fullsize_gpu.py and scripts/local_setup_cfg4.py)")
    steps = a.steps if a.steps is not None else (K_DIM if headline else (2 if hexa else 8))
    if hexa and a.warmup == 2:
        a.warmup = 1                                       # a matvec of this case is 315 time steps of ~60 ms
    case = build_case(a.case, a.lx1)
    cfg_index = {"cfg2": 1, "cfg3": 2, "cfg4": 3}[a.case]
    amode = 1 if hexa else 0                               # configs[3] is an ADJOINT Arnoldi run

    def make_context(cs):
        if hexa:                                           # the settings of scripts/run_cfg4_arnoldi.py
            return NekStabHip(cs, cs.meta["vert"], cs.meta["nvert"], tol_helm=1e-10, tol_pres=1e-2, tol_relative=1, max_helm_iter=150, max_pres_iter=96, nproj=a.nproj)
        # shards carry the parent's projection space (nsk_shard_create), so the sharded operator is the single-rank one
        hh = NekStabHip(cs, cs.meta["vert"], cs.meta["nvert"], tol_helm=a.tol_helm, tol_pres=a.tol_pres, tol_relative=1,
                        schwarz_layers=2, max_helm_iter=100 if cs.lx1 <= 8 else 250, max_pres_iter=48 if cs.lx1 <= 8 else 144, nproj=a.nproj)
        if a.min_pres > 0:
            hh.set_option("min_pres_iter", a.min_pres)
        return hh

    # Sharded runs: RANK-LOCAL set-up in the first attempt (every rank sets up its own elements + two rings and the ranks
    # exchange the volume, the CFL maximum and their coarse rows: sharded.LocalParent); the retry attempt cuts the shards from
    # a whole-mesh context on every rank, as rounds 1-2 did.  Rank 0 builds the whole-mesh context AFTER the sharded run, for
    # the one-GPU number of the same steps.
    local_setup = sharded and not a.whole_mesh_setup and int(os.environ.get("NSK_BENCH_ATTEMPT", "0")) == 0
    parts = {}

    def make_parent(cs):
        from nekstab_amd.sharded import LocalParent, partition_rcb
        parts[id(cs)] = partition_rcb(cs, world)
        if not local_setup:
            return make_context(cs)
        lp = LocalParent(cs, parts[id(cs)], rank, tol_helm=a.tol_helm, tol_pres=a.tol_pres, tol_relative=1, schwarz_layers=2, max_helm_iter=100,
                         max_pres_iter=48, nproj=a.nproj)
        lp.finish_dist(dist)
        if a.min_pres > 0:
            lp.set_option("min_pres_iter", a.min_pres)
        return lp

    t0 = time.perf_counter()
    full = make_parent(case) if sharded else make_context(case)
    setup_s = time.perf_counter() - t0
    print("[bench] rank %d: context ready in %.1f s (%d of E=%d elements, lx1=%d)" % (rank, setup_s, full.nel, case.nel, case.lx1), file=sys.stderr, flush=True)
    if a.pres_cap > 0 and not sharded:
        full.set_option("pres_cap", a.pres_cap)
    if a.fused >= 0:
        full.set_option("fused", a.fused)
    if hexa:
        # seed: the reference's committed optimal perturbation of the 2-D step (examples/back_fstep/transient_growth), extruded,
        # plus a spanwise-periodic w component: a three-dimensional vector whose inner solves behave like a Krylov vector's
        from nekstab_amd import mesh, mesh3d
        c2, nz = case.meta["c2"], case.meta["nz"]
        tg = np.load(os.path.join(ROOT, "tests", "golden", "backstep_tg.npz"))
        u2 = mesh.interp_field_2d(tg["pRe_u"].astype(np.float64), case.lx1) * c2.mask
        qx, qy = mesh3d.extrude_field(u2[0], nz), mesh3d.extrude_field(u2[1], nz)
        qz = 1e-1 * np.sin(2 * np.pi * case.z / (0.2 * nz)) * case.mask * np.abs(qx)
        zp = np.zeros(full.npres)
    else:
        qx, qy = seed.add_noise(case)
        zp = np.zeros((case.nel, case.lx1 - 2, case.lx1 - 2))

    def upload_seed(ctx, v):
        if hexa:
            ctx.upload3(v, qx, qy, qz, zp)
        else:
            ctx.upload(v, qx, qy, zp)

    def make_shard(parent, cs):
        from nekstab_amd.sharded import ShardRank
        dev = "cuda" if backend == "nccl" else "cpu"
        idt = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0 and backend == "nccl":
            idt = torch.tensor(list(ShardRank.new_unique_id(parent.lib)), dtype=torch.uint8, device=dev)
        dist.broadcast(idt, 0)
        sh = ShardRank(parent, cs, rank, world, bytes(idt.cpu().tolist()) if backend == "nccl" else None, parts[id(cs)])
        if backend != "nccl":
            from nekstab_amd.sharded import attach_host_transport
            attach_host_transport(sh, dist)
            if os.environ.get("NSK_BENCH_HALO_OVERLAP") == "1":     # dry run: interior workgroups run while gloo moves the halos
                sh.set_option("halo_overlap", 1)
        else:
            sh.set_option("shard_graph", 0)                # eager until the first exchanges have run (RCCL sets its peer connections up lazily: not inside a capture)
            pf = os.environ.get("NSK_BENCH_PREFLIGHT")
            if pf and json.loads(pf).get("rccl_fuse") == 0:
                sh.set_option("rccl_fuse", 0)              # the pre-flight check of this run found the grouped all-reduce wanting (supervise())
            if int(os.environ.get("NSK_BENCH_ATTEMPT", "0")) > 0:
                sh.set_option("rccl_fuse", 0)              # the retry attempt: the all-reduces as calls of their own (the grouped form has not run on hardware before this node)
        return sh

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def all_ok(ok, err):
        """Every rank learns whether ALL ranks got here in good shape; a failure anywhere ends every worker non-zero (the
        supervisors then start the next attempt together)."""
        flag = torch.tensor([1.0 if ok else 0.0], device="cuda" if backend == "nccl" else "cpu")
        try:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        except Exception as e:                              # noqa: BLE001
            err = err or repr(e)[:400]
            flag = torch.zeros(1)
        if float(flag.item()) == 0.0:
            print("bench.py rank %d: SHARDED RUN FAILED (%s; shard_graph = %d)" % (rank, err or "another rank failed", shard_graph), file=sys.stderr, flush=True)
            os._exit(FAIL_EXIT)

    def agree(ok):
        """True when EVERY rank reports ok (a failed all-reduce counts as a failure); nobody exits."""
        flag = torch.tensor([1.0 if ok else 0.0], device="cuda" if backend == "nccl" else "cpu")
        try:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            return float(flag.item()) != 0.0
        except Exception:                                   # noqa: BLE001
            return False

    h = full
    if sharded:
        # first execution of the RCCL halo path on this node: a two-step probe map under its own, shorter, watchdog
        pw = threading.Timer(PROBE_S, _stalled, ("sharded probe map (first execution of the RCCL halo path)", PROBE_S))
        pw.daemon = True
        pw.start()
        err = None
        shard_mode = {}
        try:
            h = make_shard(full, case)
            probe = h.alloc(2)
            h.upload(probe[0], qx, qy, zp)
            h.scal(probe[0], 1.0 / h.norm(probe[0]))
            ns = h.nsteps
            h.set_nsteps(2)
            h.matvec(probe[1], probe[0], 0)                 # eager: every peer connection and the all-reduce ring exist after this
            if (shard_graph == 1 and backend == "nccl") or os.environ.get("NSK_BENCH_FORCE_MODE_PROBE") == "1":      # (the override: dry runs exercise this code)
                # Two ways to run the sharded step over RCCL, and no hardware to have measured them on before this run: (a) one
                # captured graph per step class with the RCCL calls inside (no host work per step, but every BUDGETED iteration
                # pays its exchange and all-reduce); (b) eager launches with the convergence flags read on the host (half to a
                # third of the collectives, a stream synchronisation per solve).  Time 24 time steps each way, keep the faster.
                h.set_nsteps(int(os.environ.get("NSK_BENCH_PROBE_STEPS", "24")))      # (dry runs over gloo shorten it)
                times = {}
                # (c): (b) + the boundary workgroups' halo in flight while the interior workgroups run.  The captured graphs come LAST and
                # with SETTLED launch budgets (the largest iteration counts the host-checked maps just saw, + 3): at the start-up
                # budgets (100 / 48 launches per solve, each with its collectives) the comparison would be against a state the
                # timed factorisation leaves after its first maps.
                MODES = {"hostcheck": (0, 1, 0), "hostcheck_overlap": (0, 1, 1), "graph": (1, 0, 0)}
                seen = {"helm": 0, "pres": 0}
                for name, (gr, hcq, ovl) in MODES.items():
                    h.set_option("shard_graph", gr)
                    h.set_option("shard_hostcheck", hcq)
                    h.set_option("halo_overlap", ovl)
                    if name == "graph":
                        h.set_option("budget_helm", seen["helm"] + 3)
                        h.set_option("budget_pres", seen["pres"] + 3)
                    h.matvec(probe[1], probe[0], 0)         # (captures / settles)
                    if name != "graph":
                        stq = h.stats()
                        seen["helm"] = max(seen["helm"], int(stq["max_helm_iter"])); seen["pres"] = max(seen["pres"], int(stq["max_pres_iter"]))
                    barrier(); tq = time.perf_counter()
                    h.matvec(probe[1], probe[0], 0)
                    barrier(); tq = time.perf_counter() - tq
                    tt = torch.tensor([tq], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
                    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                    times[name] = float(tt.item())
                shard_mode.update(times, picked=min(times, key=times.get))
                gr, hcq, ovl = MODES[shard_mode["picked"]]
                h.set_option("shard_graph", gr)
                h.set_option("shard_hostcheck", hcq)
                h.set_option("halo_overlap", ovl)
            h.set_nsteps(ns)
            h.free(probe)
        except Exception as e:                              # noqa: BLE001
            err = repr(e)[:400]
        all_ok(err is None, err)
        pw.cancel()
    if os.environ.get("NSK_BENCH_MAP_STEPS"):              # dry runs (tests): shorter maps; the record says so in config.workload through h.nsteps
        h.set_nsteps(int(os.environ["NSK_BENCH_MAP_STEPS"]))
        if sharded and rank == 0 and not local_setup:
            full.set_nsteps(int(os.environ["NSK_BENCH_MAP_STEPS"]))
    ktot = max(a.warmup + steps, K_DIM if (headline and a.full and not a.no_kdim) else 0)
    Q = h.alloc(ktot + 1)
    upload_seed(h, Q[0])
    h.scal(Q[0], 1.0 / h.norm(Q[0]))
    H = np.zeros((ktot + 1, ktot))
    stats = {}
    # warm-up steps: also settle the adaptive launch budgets / graph captures
    krylov.arnoldi_factorization(h, Q, H, 1, a.warmup, amode, stats=stats)
    barrier()
    t0 = time.perf_counter()
    krylov.arnoldi_factorization(h, Q, H, a.warmup + 1, a.warmup + steps, amode, stats=stats)
    barrier()
    elapsed = time.perf_counter() - t0
    print("[bench] rank %d: %d timed Arnoldi steps in %.2f s" % (rank, steps, elapsed), file=sys.stderr, flush=True)
    if dist is not None:
        t = torch.tensor([elapsed], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    kdone = a.warmup + steps
    if a.dump_outputs and rank == 0:
        # the factorisation so far and the basis vector the last timed step appended (sharded: the Hessenberg matrix only)
        dumped = {"hessenberg": H[:kdone + 1, :kdone]}
        if not sharded:
            dumped.update(vector_outputs(h, Q[kdone], "krylov", hexa))
        dump_outputs(a.dump_outputs, dumped)
    kdim_case = 256 if hexa else K_DIM
    par = "1 GPU"
    if world > 1:
        par = ("element-sharded x%d (%s, one eigenproblem, %s)" % (world, "RCCL halos" if backend == "nccl" else "host-staged halos over %s: protocol dry run" % backend,
               "step graphs" if (shard_graph == 1 and backend == "nccl" and shard_mode.get("picked") == "graph") else ("eager launches, host-read convergence flags" + (", halo / interior overlap" if shard_mode.get("picked") == "hostcheck_overlap" else "")))) if sharded else "replicas x%d" % world
    # ---- THE RECORD.  Complete from here on: value = the K timed steps.  Everything below adds fields to it, each section
    # inside its own try / except (a failed section leaves {"error": ...} in its field), and the N = 1 run keeps a watchdog
    # that prints the record as it stands if the optional work outlives --optional-budget-s.  BENCH_r04 was lost because an
    # optional diagnostic raised before the single print at the end of this function.
    out = {
        "metric": METRIC,
        "value": (world if (world > 1 and not sharded) else 1) * steps / elapsed, "unit": "matvecs/s", "n_gpus": world, "steps": steps, "warmup": a.warmup,
        "ms_per_step": 1e3 * elapsed / steps, "higher_is_better": True, "scaling": "strong" if sharded else "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic seed vector (the reference's add_noise) on the reference's committed mesh and base flow (fixtures under tests/golden)",
        "config": {"workload": ("backward-facing step Re=500 extruded over %d periodic layers, adjoint Arnoldi (BASELINE configs[3]): E=%d hexahedra, lx1=%d, lxd=%d, nsteps=%d/matvec, k_dim=256; state vector %.0f MB"
                                % (case.meta["nz"], case.nel, case.lx1, case.lxd, h.nsteps, 8e-6 * h.nstate)) if hexa else
                               "cylinder Re=50 direct Arnoldi (BASELINE configs[%d]): E=%d, lx1=%d, lxd=%d, nsteps=%d/matvec, k_dim=%d"
                               % (cfg_index, case.nel, case.lx1, case.lxd, h.nsteps, K_DIM),
                   "base_flow": "reference BF_bfs0.f00001 (committed fixture) extruded, w = 0; seed = the reference's optimal perturbation pRe extruded + a spanwise-periodic w" if hexa
                                else "reference BF_1cyl0.f00001 (committed fixture), seed = add_noise",
                   "tolerances": ("Helmholtz |b-Hu|<=1e-10|b|, pressure |g-E dp|<=1e-2|g| (time steps 1-3 of a map: x0.01), projection space %d, host-read convergence flags: DESIGN.md section 8" % a.nproj) if hexa else
                                 "Helmholtz |b-Hu|<=%g|b|, pressure |g-E dp|<=%g|g| with at least %d GMRES iterations per solve%s (time steps 1-3 of a map: pressure tolerance x0.01), projection space %d: DESIGN.md section 1"
                                 % (a.tol_helm, a.tol_pres, a.min_pres, (" and at most %d after time step 3" % a.pres_cap) if a.pres_cap else "", a.nproj),
                   "parallelism": par,
                   "host_loop": "Python over ctypes (nekstab_amd/krylov.py); the flang-built loop over the same C-ABI is timed in `fortran_host`"},
        "setup_s": setup_s,
        "matvec_s_mean": float(np.mean(stats["matvec_s"][a.warmup:a.warmup + steps])), "orth_s_mean": float(np.mean(stats["orth_s"][a.warmup:a.warmup + steps])),
    }
    import threading as _th
    _plock = _th.Lock()
    _printed = {"done": False}

    def emit():
        """print THE one JSON line, once.  The watchdog thread may call this while the main thread is adding a field: serialise
        first (retrying while the dictionary changes), and only a printed line counts as done."""
        with _plock:
            if _printed["done"] or rank != 0:
                return
            line = None
            for _ in range(50):
                try:
                    line = json.dumps(dict(out))
                    break
                except RuntimeError:                           # dictionary changed size during iteration
                    time.sleep(0.02)
            if line is None:                                    # the record proper (scalars and the small dictionaries of the timed region)
                line = json.dumps({k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data") if k in out})
            print(line, flush=True)
            _printed["done"] = True

    def guarded(field, fn):
        """run an optional section; its failure is a field of the record, never the end of the run"""
        t_sec = time.perf_counter()
        try:
            if field in os.environ.get("NSK_BENCH_TEST_FAIL", "").split(","):      # test hook (tests/test_bench_driver_gpu.py)
                raise RuntimeError("forced failure of section %s (test hook)" % field)
            fn()
        except Exception as e:                                  # noqa: BLE001
            out[field] = {"error": repr(e)[:300]}
            print("[bench] section %s failed: %r" % (field, e), file=sys.stderr, flush=True)
        print("[bench] section %s: %.1f s" % (field, time.perf_counter() - t_sec), file=sys.stderr, flush=True)

    if a.ref_logfile:
        def sec_reflog():
            r = parse_reference_logfile(a.ref_logfile)
            ref = r.get("matvecs_per_s") or r.get("matvecs_per_s_lower_bound")
            if ref:
                r["gpu_over_reference"] = out["value"] / ref
            out["reference_logfile"] = r
        guarded("reference_logfile", sec_reflog)

    opt_wd = None
    if world == 1 and a.full:
        def _optional_overrun():
            out["optional_sections_cut"] = "the sections after the timed steps outlived --optional-budget-s = %g s: the record is printed as it stood" % a.optional_budget_s
            emit()
            os._exit(0)
        opt_wd = _th.Timer(a.optional_budget_s, _optional_overrun)
        opt_wd.daemon = True
        opt_wd.start()

    # ---- wall time to k_dim Ritz pairs: continue the SAME factorisation (not part of `value`)
    def sec_kdim():
        nonlocal kdone
        if kdone < ktot:
            krylov.arnoldi_factorization(h, Q, H, kdone + 1, ktot, amode, stats=stats)
            kdone = ktot
    if a.full:
        guarded("wall_time_kdim_s", sec_kdim)
    kdone = len(stats["matvec_s"])                          # (what was completed, also after a failure half way)
    step_s = np.array(stats["matvec_s"][:kdone]) + np.array(stats["orth_s"][:kdone])
    wall_kdim = float(step_s[:K_DIM].sum()) if kdone >= K_DIM else None
    if not isinstance(out.get("wall_time_kdim_s"), dict):
        out["wall_time_kdim_s"] = wall_kdim
    if wall_kdim is None:
        out["wall_time_kdim_note"] = "only %d of the %d Arnoldi steps were run (--steps / --no-kdim / no --full); per-step time x %d = %.1f s projected" % (kdone, kdim_case, kdim_case, kdim_case * elapsed / steps)

    def sec_ritz():
        kk = min(kdone, K_DIM) if kdone >= K_DIM else kdone
        vals, vecs = krylov.eig_sorted(H[:kk, :kk])
        # The reference's only lx1 = 8 table is the adjoint one (same spectrum up to discretisation): Spectre_Ha.dat row 1 = 0.7386891 -+ 0.6972319i;
        # the CPU oracle's converged direct spectrum at lx1 = 8 is in tests/golden/cylinder_oracle_spectra.npz (Hd8)
        ritz = {"k": kk, "re": float(vals[0].real), "im": float(abs(vals[0].imag)), "residual": float(abs(H[kk, kk - 1] * vecs[kk - 1, 0]))}
        if not hexa:
            ritz["reference_Spectre_Ha_lx1_8"] = [0.7386891, 0.6972319]
            ritz["parity"] = ("rows pinned to the REFERENCE's tables at 5e-6 (tests/test_spectrum_pin_gpu.py, k = 200 at these settings): every converged row of "
                              "Spectre_Ha.dat (adjoint, lx1 = 8) and rows 1, 4 of Spectre_Hd.dat (direct, lx1 = 6); the wake rows 5-23 of Spectre_Hd.dat sit 1.2e-5 .. 4.6e-5 "
                              "from the table and are pinned to the ORACLE only (1e-8 HIP vs oracle): DESIGN.md section 1")
        out["leading_ritz"] = ritz
    if a.full:
        guarded("leading_ritz", sec_ritz)

    if not sharded and a.full:
        st = {}

        def sec_bytes():
            st.update(full.stats())
            tsteps = max(st["total_steps"], 1)
            out.update({"helm_iters_per_step": st["total_helm_iters"] / tsteps, "pres_iters_per_step": st["total_pres_iters"] / tsteps,
                        "map_retries": st["retries"], "graph_recaptures": st["recaptures"], "graph_recapture_s": st["recapture_seconds"],
                        "capped_solves": st["total_capped_solves"], "worst_cap_ratio": st["total_worst_cap_ratio"],
                        "launch_budgets": {"per_time_step": {"maps": st["step_budget_maps"], "helm_launches_per_step": st["step_budget_helm_mean"], "pres_iterations_per_step": st["step_budget_pres_mean"]},
                                           "persistent_tail_maps": st["tail_maps"],
                                           "last_step_class": {"helm": st["budget_helm"], "pres": st["budget_pres"]},
                                           "note": "launches per time step in the captured graphs: budgets = largest count of the step and its neighbours over the last 8 maps + head-room, a launch beyond a solve's own count returning on a device flag; persistent_tail_maps > 0: one persistent launch per solve behind them runs whatever a solve still needs, so no budget overflows and no map is redone (default where the grid is resident: safety net, head-room 1 / 0; option tail = 1: the numbers are HEADS = median counts and the tail does the rest; nsk_persist.hpp)"}})
            # ---- SURVEY 8(d) accounting: algorithmic bytes per matvec from the logged iteration counts
            geom = dict(nel=case.nel, lx1=case.lx1, ndim=2, nvert=int(case.meta["nvert"]), coarse_lda=(lambda nv: ((nv + 767) // 768) * 768 if ((nv + 767) // 768) * 768 <= 3072 else ((nv + 255) // 256) * 256)(int(case.meta["nvert"])),
                        patch_stride=(((case.lx1 - 2 + 4) ** 2 + 3) // 4) * 4, nproj=a.nproj,
                        fuse2=1 if (case.nel <= 4096 and os.environ.get("NSK_FUSE2", "1") != "0") else 0)      # (the two-launch pressure iteration: graph-replayed meshes)
            if hexa:
                geom = dict(nel=case.nel, lx1=case.lx1, ndim=3, nvert=int(case.meta["nvert"]), nproj=a.nproj, zero_arrays=int(full.stats().get("zero_arrays", 0)))
                out["zero_arrays"] = {"mask": geom["zero_arrays"], "note": "hexahedra: arrays that vanish on every node (bits 0-8 metric terms, 9-11 G factors 4-6, 12-23 base-flow constants of the convection kernel) are neither loaded nor counted in the algorithmic bytes; Nek5000 skips the same terms on its undeformed elements (hmholtz.f axhelm, ifdfrm)"}
            bpm, per = roofline.matvec_bytes(st, full.nsteps, **geom)
            st["_per"] = per
            out["geometry"] = geom
            jmean = a.warmup + (steps + 1) / 2.0
            bpm_k = roofline.krylov_bytes(full.nstate, jmean)
            e2e = (bpm + bpm_k) / (elapsed / steps) / 1e9
            out["bytes_per_matvec"] = {"time_stepper": bpm, "krylov_projection_mean": bpm_k, "per_time_step_by_kernel": per,
                                       "rule": "SURVEY 8(d): every distinct array once per kernel invocation, from the logged iteration counts (nekstab_amd/roofline.py)"}
            out["roofline_end_to_end"] = {"bound": "hbm", "achieved": e2e, "peak": 8000.0, "unit": "GB/s", "frac": e2e / 8000.0,
                                          "note": "algorithmic bytes of a whole Arnoldi step / its wall time"}
            out["ms_per_time_step"] = 1e3 * float(np.mean(stats["matvec_s"][a.warmup:a.warmup + steps])) / full.nsteps
            if hexa:
                out["pres_basis_index_sum_per_step"] = st["total_pres_jsum"] / tsteps
                out["coarse_bytes_per_solve"] = st["coarse_bytes_per_solve"]
                # the SURVEY rule counts the arrays the three components of a CG launch share once PER COMPONENT; with every distinct array once per launch:
                rule, distinct = roofline.helm_launch_bytes(nel=case.nel, lx1=case.lx1, ndim=3, zero_arrays=geom["zero_arrays"])
                hit = st["total_helm_iters"] / tsteps
                bpm_d = bpm - full.nsteps * (rule - distinct) * hit
                out["bytes_per_matvec"]["time_stepper_shared_arrays_once"] = bpm_d
                e2d = (bpm_d + bpm_k) / (elapsed / steps) / 1e9
                out["roofline_end_to_end"].update({"achieved_shared_arrays_once": e2d, "frac_shared_arrays_once": e2d / 8000.0})
        guarded("bytes_per_matvec", sec_bytes)

        # ---- dominant kernel, timed live with HIP events on the library's own stream.  nsk_bench_kernel runs on the live
        # solver state and marks it dirty: the next map of this context starts from a reset state (nsk.hip: reset_solver_state)
        def sec_roofline():
            P = full.nvel
            fused_on = False
            if a.fused > 0:
                try:
                    kern8 = full.bench_kernel("helm_fused", 200)
                    kern0 = full.bench_kernel("helm_fused0", 200)
                    fused_on = True
                except Exception:                               # noqa: BLE001
                    fused_on = False
            if fused_on:
                its = 8
                per = st["_per"]
                alg = per["K2 rhs"] + per["K4 pres_rhs"] + 148.0 * 2 * P * its
                achieved = alg / (kern8["avg_us"] * 1e-6) / 1e9
                traffic, tnote = pmc_traffic("k_helm_fused<%d>" % case.lx1)
                out["roofline"] = {"bound": "hbm", "kernel": "k_helm_fused<%d> (rhs + %d CG iterations of both components + pressure rhs in one persistent launch)" % (case.lx1, its),
                                   "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0, "traffic": traffic, "traffic_source": tnote,
                                   "avg_launch_us": kern8["avg_us"], "us_per_cg_iteration": (kern8["avg_us"] - kern0["avg_us"]) / its,
                                   "algorithmic_bytes_per_launch": alg}
            elif hexa:
                # live HIP-event timings of the hot hexahedral kernels on the state the last map left (every launch does full work)
                za = int(full.stats().get("zero_arrays", 0))
                rule, distinct = roofline.helm_launch_bytes(nel=case.nel, lx1=case.lx1, ndim=3, zero_arrays=za)
                P2, nel_, N_ = full.npres, case.nel, case.lx1
                one = roofline.per_step_bytes(nel=nel_, lx1=N_, ndim=3, nvert=int(case.meta["nvert"]), nproj=0, helm_iters=0.0, pres_iters=1.0, pres_jsum=0.0, coarse_bytes=0.0, zero_arrays=za)
                kb = {"helm": rule, "divgs": one["K7 divgs (x n_pres)"], "schwarz": one["K6 schwarz (x n_pres)"] - nel_ * 8 * 12.0}
                for jq in (8, 24):
                    kb["gs_dots%d" % jq] = 8.0 * P2 * (jq + 2)
                    kb["gs_lag%d" % jq] = 8.0 * P2 * (jq + 3) + 64.0 * nel_        # (no pending correction in this timing: one store)
                ktab = {}
                for kn, byts in kb.items():
                    kr = full.bench_kernel(kn, 20)
                    ktab[kn] = {"avg_us": kr["avg_us"], "algorithmic_bytes": byts, "GBps": byts / kr["avg_us"] / 1e3, "frac": byts / kr["avg_us"] / 1e3 / 8000.0}
                ktab["helm"]["algorithmic_bytes_shared_arrays_once"] = distinct
                ktab["helm"]["frac_shared_arrays_once"] = distinct / ktab["helm"]["avg_us"] / 1e3 / 8000.0
                for kn in ktab:
                    tr, _ = pmc_traffic("k3::" + kn)
                    ktab[kn]["traffic"] = tr
                out["kernels"] = ktab
                traffic, tnote = pmc_traffic("k3::helm")
                out["roofline"] = {"bound": "hbm", "kernel": "k3::k_helm<%d> (one CG iteration of the three components; the largest share of the kernel time: profiles/r06_cfg4_kernel_table.md, r05_cfg4_trace_summary.txt)" % case.lx1,
                                   "achieved": distinct / ktab["helm"]["avg_us"] / 1e3, "peak": 8000.0, "unit": "GB/s", "frac": ktab["helm"]["frac_shared_arrays_once"], "traffic": traffic, "traffic_source": tnote,
                                   "avg_launch_us": ktab["helm"]["avg_us"], "algorithmic_bytes_per_launch": distinct,
                                   "survey_rule": {"algorithmic_bytes_per_launch": rule, "frac": ktab["helm"]["frac"]},
                                   "note": "every distinct array of the launch ONCE (the figure to quote).  SURVEY 8(d)'s per-component rule (172 B per point and COMPONENT, less 8 B for every G factor that vanishes on the whole mesh: zero_arrays) counts the arrays the three components share three times: `survey_rule`, not a bandwidth"}
            else:
                kern = full.bench_kernel("helm", 200)
                alg = 148.0 * 2 * P
                achieved = alg / (kern["avg_us"] * 1e-6) / 1e9
                traffic, tnote = pmc_traffic("k_helm<%d>" % case.lx1)
                out["roofline"] = {"bound": "hbm", "kernel": "k_helm<%d>" % case.lx1, "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                                   "traffic": traffic, "traffic_source": tnote, "avg_launch_us": kern["avg_us"], "algorithmic_bytes_per_launch": alg,
                                   "note": "148 B per point and component (SURVEY 8(d): K3 + K4 + K5) x 2 components x %d points / the average of 200 back-to-back full-work launches (HIP events on the library's stream); the ~30 MB working set is Infinity-Cache resident" % P}
        guarded("roofline", sec_roofline)
        if isinstance(out.get("roofline"), dict) and "error" in out["roofline"]:
            out["roofline"].update({"bound": "hbm", "achieved": None, "peak": 8000.0, "unit": "GB/s", "frac": None, "traffic": None})
    elif sharded:
        st = h.stats()
        out.update({"helm_iters_per_step_last_map": st["helm_iters"] / max(st["steps"], 1), "pres_iters_per_step_last_map": st["pres_iters"] / max(st["steps"], 1),
                    "map_retries": st["retries"], "graph_recaptures": st["recaptures"]})
        out["roofline"] = {"bound": "hbm", "kernel": None, "achieved": None, "peak": 8000.0, "unit": "GB/s", "frac": None, "traffic": None,
                           "note": "sharded run: the step is a chain of small kernels and RCCL exchanges, no single dominant kernel measured (the N = 1 record has the kernel roofline)"}

        def one_gpu_same_steps(ctx, cs, nst):
            """the same Arnoldi steps (warm-up + timed) on ONE GPU: rank 0's full-mesh context, hipGraph path"""
            x, y = seed.add_noise(cs)
            Q1 = ctx.alloc(a.warmup + nst + 1)
            ctx.upload(Q1[0], x, y, np.zeros((cs.nel, cs.lx1 - 2, cs.lx1 - 2)))
            ctx.scal(Q1[0], 1.0 / ctx.norm(Q1[0]))
            H1 = np.zeros((a.warmup + nst + 1, a.warmup + nst)); s1 = {}
            krylov.arnoldi_factorization(ctx, Q1, H1, 1, a.warmup, 0, stats=s1)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            krylov.arnoldi_factorization(ctx, Q1, H1, a.warmup + 1, a.warmup + nst, 0, stats=s1)
            torch.cuda.synchronize(); t1 = time.perf_counter() - t1
            ctx.free(Q1)
            return nst / t1

        setup_local = {"rank_local": bool(local_setup), "seconds_rank0": setup_s, "elements_rank0": int(full.nel), "elements_mesh": int(case.nel)}
        if local_setup:
            h.close(); full.close()                              # (the shard and its sub-mesh context: done)
            if rank == 0 and a.full:
                t0 = time.perf_counter()
                full = make_context(case)
                setup_local["whole_mesh_seconds_rank0"] = time.perf_counter() - t0
        out["setup"] = setup_local
        if os.environ.get("NSK_BENCH_PREFLIGHT"):
            out["rccl_preflight"] = dict(json.loads(os.environ["NSK_BENCH_PREFLIGHT"]), note="tests/mp_rccl_worker.py in fresh processes before the timed run: a sharded map with the all-reduce inside the halo messages' RCCL group (fuse1) and, only if that fails, with separate calls (fuse0); `rccl_fuse` is the form this run used")
        out["shard_mode"] = dict(shard_mode, config=a.case, note="seconds for 24 sharded time steps with captured step graphs (RCCL calls inside) / with eager launches and host-read convergence flags / the same with the halo of the velocity solve overlapped with its interior work; the timed run uses the fastest") if shard_mode else \
            {"picked": "hostcheck" if backend != "nccl" or shard_graph == 0 else "graph", "note": "not compared in this attempt"}
        if rank == 0 and a.full:
            try:
                r1 = one_gpu_same_steps(full, case, steps)
                out["single_gpu_same_config"] = {"matvecs_per_s": r1, "sample": "the same %d + %d Arnoldi steps of the same case on rank 0's full-mesh context (hipGraph path), timed after the sharded run" % (a.warmup, steps),
                                                 "speedup_sharded": (steps / elapsed) / r1}
            except Exception as e:                              # noqa: BLE001
                out["single_gpu_same_config"] = {"error": repr(e)[:300]}
        dist.barrier()
        all_ok(True, None)                                 # nobody prints a record unless every rank got to the end of the headline workload
        emit()                                             # THE RECORD, before the optional sharded run of configs[2] (its result goes to stderr and --extras-out)
        extras = {}
        # ---- BASELINE configs[2] next to the headline workload: where element sharding is meant to pay (1.15 M points per field).
        # The headline record is PRINTED at this point; this section runs under its own watchdog (a stall ends the worker with
        # code 0), every rank catches its own exceptions and the ranks agree on the outcome before anyone goes on.
        if a.case == "cfg2" and not a.no_cfg3_probe and a.full:
            def _cfg3_stalled():
                print("bench.py rank %d: config3_sharded: no result after %d s: keeping the headline record" % (rank, C3_PROBE_S), file=sys.stderr, flush=True)
                if rank == 0:
                    print("[bench extras] " + json.dumps({"config3_sharded": {"error": "stalled: no result after %d s" % C3_PROBE_S}}), file=sys.stderr, flush=True)
                os._exit(0)
            c3w = threading.Timer(C3_PROBE_S, _cfg3_stalled)
            c3w.daemon = True
            c3w.start()
            rec3, err3, case3 = None, None, None
            try:
                if not local_setup:
                    h.close()
                    full.close()
                elif rank == 0:
                    full.close()
                h = full = None
                case3 = build_case("cfg3")
                t0 = time.perf_counter()
                full = make_parent(case3)
                setup3_s = time.perf_counter() - t0
                h = make_shard(full, case3)                # (a NEW communicator: ncclCommInitRank inside ShardRank; eager so far)
                x3, y3 = seed.add_noise(case3)
                z3 = np.zeros((case3.nel, case3.lx1 - 2, case3.lx1 - 2))
                n3 = 2
                Q3 = h.alloc(n3 + 2)
                h.upload(Q3[0], x3, y3, z3)
                h.scal(Q3[0], 1.0 / h.norm(Q3[0]))
                # peer connections are per communicator and RCCL sets them up lazily: the first exchanges of THIS communicator
                # run eagerly (a two-step map), as for the headline shard, before captured graphs may be switched on
                ns3 = h.nsteps
                h.set_nsteps(2)
                h.matvec(Q3[1], Q3[0], 0)
                h.set_nsteps(ns3)
                if shard_graph == 1 and backend == "nccl":     # the mode that was faster on the headline workload
                    h.set_option("shard_graph", 1 if shard_mode.get("picked") == "graph" else 0)
                    h.set_option("shard_hostcheck", 0 if shard_mode.get("picked") == "graph" else 1)
                    h.set_option("halo_overlap", 1 if shard_mode.get("picked") == "hostcheck_overlap" else 0)
                H3 = np.zeros((n3 + 2, n3 + 1)); s3 = {}
                krylov.arnoldi_factorization(h, Q3, H3, 1, 1, 0, stats=s3)
                barrier(); t3 = time.perf_counter()
                krylov.arnoldi_factorization(h, Q3, H3, 2, n3 + 1, 0, stats=s3)
                barrier(); t3 = time.perf_counter() - t3
                tt = torch.tensor([t3], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                rec3 = {"workload": "cylinder Re=50 direct Arnoldi (BASELINE configs[2]): E=%d, lx1=%d, nsteps=%d/matvec" % (case3.nel, case3.lx1, h.nsteps),
                        "matvecs_per_s": n3 / float(tt.item()), "steps": n3, "warmup": 1,
                        "setup": {"rank_local": bool(local_setup), "seconds_rank0": setup3_s, "elements_rank0": int(full.nel), "elements_mesh": int(case3.nel)}}
            except Exception as e:                              # noqa: BLE001
                err3 = repr(e)[:400]
                print("bench.py rank %d: config3_sharded failed: %s" % (rank, err3), file=sys.stderr, flush=True)
            if agree(err3 is None):
                try:
                    if local_setup:
                        h.close(); full.close()
                        h = full = None
                        if rank == 0:
                            t0 = time.perf_counter()
                            full = make_context(case3)
                            rec3["setup"]["whole_mesh_seconds_rank0"] = time.perf_counter() - t0
                    if rank == 0:
                        saved = a.warmup
                        a.warmup = 1
                        r13 = one_gpu_same_steps(full, case3, n3)
                        a.warmup = saved
                        rec3["single_gpu_same_config"] = {"matvecs_per_s": r13, "speedup_sharded": rec3["matvecs_per_s"] / r13}
                except Exception as e:                          # noqa: BLE001
                    rec3["single_gpu_same_config"] = {"error": repr(e)[:400]}
                extras["config3_sharded"] = rec3
                dist.barrier()
            else:
                extras["config3_sharded"] = {"error": err3 or "another rank failed"}
            c3w.cancel()
        if rank == 0 and extras:
            print("[bench extras] " + json.dumps(extras), file=sys.stderr, flush=True)
            try:
                os.makedirs(os.path.dirname(a.extras_out), exist_ok=True)
                with open(a.extras_out, "w") as fh:
                    json.dump(extras, fh, indent=1)
            except OSError:
                pass

    # ---- N = 1: the CPU baseline and the Fortran-host leg, then THE RECORD; the optional diagnostics run after it
    if world == 1:
        if headline and a.full and not a.no_cpu_baseline:
            def sec_cpu():
                qs = full.download(Q[a.warmup]) if not hexa else None      # the input of the first timed Arnoldi step
                out["cpu_baseline"] = cpu_baseline(case, a.cpu_threads, (a.tol_helm, a.tol_pres, a.min_pres), a.nproj, out["value"], qs)
            guarded("cpu_baseline", sec_cpu)
        if hexa and a.full:
            out["cpu_baseline"] = None
            out["cpu_baseline_note"] = "the C / OpenMP port of the step (oracle/cpu_step.c) covers quadrilaterals; the hexahedral oracle (oracle/linns3d.py) uses sparse direct solves and does not reach this size: the default record (BASELINE configs[1]) carries the CPU baseline"
        if headline and a.full and not a.no_fortran_host:
            def sec_fortran():
                out["fortran_host"] = fortran_host_leg(case, (qx, qy, zp), a, steps, out["value"])
            guarded("fortran_host", sec_fortran)
        emit()
        if opt_wd is not None:
            opt_wd.cancel()
        if a.extras and headline:
            extras = {}

            def sec_extras():
                run_extras(a, case, full, (qx, qy, zp), stats, step_s, out, extras)
            try:
                sec_extras()
            except Exception as e:                              # noqa: BLE001
                extras["error"] = repr(e)[:300]
            try:
                os.makedirs(os.path.dirname(a.extras_out), exist_ok=True)
                with open(a.extras_out, "w") as fh:
                    json.dump(extras, fh, indent=1)
            except OSError as e:
                print("[bench] extras not written: %r" % e, file=sys.stderr, flush=True)
            print("[bench extras] " + json.dumps(extras), file=sys.stderr, flush=True)
        full.close()
        return
    if not sharded:                                        # replicas (world > 1)
        emit()
    if sharded and h is not None:
        h.close()
    if full is not None:
        full.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
