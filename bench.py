#!/usr/bin/env python3
"""bench.py — headline benchmark: candidate-evals/s of Differential Evolution on
Rosenbrock-128D, fp64 (BASELINE.json metric; workload = configs[1], pop=65536 per GPU).

A "step" is one turn of the DE loop (best scan + stop tests + one generation of
mutation/crossover/evaluation/selection over the whole population) on synthetic
input: x0_i = 4.096, CR=0.9, F=0.8, strategy random, early stops disabled.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
A plain run sets up, warms up (2000 untimed steps, re-initialisation, W steps), times exactly K
steps and prints the line; --dump-outputs DIR writes what the last step left a caller as .npy
files. --full adds everything else the benchmark measures (kernel roofline, accepting regime,
north_star sizes, CPU baselines, other_configs, time_to_solution).
N > 1: one rank per GPU, weak scaling (every GPU owns 65536 agents). Either an external launcher
(torch.distributed.run) has set RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*, or — WORLD_SIZE unset —
this process starts the N ranks itself as fresh child processes before anything touches a GPU
(launch_ranks) and forwards rank 0's line. Rank 0 prints ONE JSON line.
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

D = 128
POP_PER_GPU = 65536
BYTES_PER_CANDIDATE = 5 * D * 8 + 16  # 4 row reads + 1 row write + score r/w
HBM_PEAK_GBS = 8000.0                  # MI355X_MICROARCH.md: 8.0 TB/s spec


def free_port():
    """A free rendezvous port on the loopback interface."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def spawn_ranks(n, argv, timeout=None):
    """Start n ranks of this script (fresh child processes, RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set) with the arguments argv and wait for them; returns (exit codes, the non-empty
    lines rank 0 wrote to stdout). A rank that died leaves its peers inside a collective: they
    get a grace period, then exactly the processes started here are ended; the same after
    `timeout` seconds."""
    port = free_port()
    import tempfile
    procs = []
    with tempfile.TemporaryFile(mode="w+") as out0:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv],
                                          env=env, stdout=out0 if r == 0 else sys.stderr,
                                          stderr=sys.stderr))
        started, failed_at = time.monotonic(), None
        while any(p.poll() is None for p in procs):
            if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
                failed_at = time.monotonic()
            if timeout is not None and failed_at is None and time.monotonic() - started > timeout:
                failed_at = time.monotonic() - 31.0
            if failed_at is not None and time.monotonic() - failed_at > 30.0:
                for p in procs:
                    if p.poll() is None:
                        p.kill()
            time.sleep(0.05)
        rcs = [p.returncode for p in procs]
        out0.seek(0)
        lines = [l for l in out0.read().splitlines() if l.strip()]
    return rcs, lines


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes
    of this one (which has not imported torch, let alone touched a GPU — never an exec), wait for
    them, forward rank 0's JSON line, exit non-zero if any rank failed.

    Under --full, the headline (DE) job at its default size is followed by a second N-rank job of
    the same script, BASELINE configs[4] as it is worded — the PSO swarm sharded over the N GPUs, 131 072
    particles x 256 each, one all-gather of the best record per iteration — whose summary rides in
    the headline line as `other_configs`; it can only add to the line, never cost it."""
    rcs, lines = spawn_ranks(args.gpus, sys.argv[1:])
    for l in lines[:-1]:
        print(l, file=sys.stderr)
    if any(rcs) or not lines:
        raise SystemExit(f"bench.py --gpus {args.gpus}: rank exit codes {rcs}")
    line = lines[-1]
    if (args.workload == "de" and args.full and args.pop_per_gpu == POP_PER_GPU
            and not args.no_other_configs and line.startswith("{")):
        entry = {"config": f"configs[4] PSO Accelerated, swarm sharded over {args.gpus} GPUs, "
                           "131072 x 256 per GPU"}
        try:
            prc, plines = spawn_ranks(args.gpus, ["--gpus", str(args.gpus), "--workload", "pso-accel",
                                                  "--steps", "100", "--warmup", "300",
                                                  "--no-cpu-baseline"], timeout=240.0)
            pj = [l for l in plines if l.startswith("{")]
            if any(prc) or not pj:
                raise RuntimeError(f"rank exit codes {prc}")
            d = json.loads(pj[-1])
            entry.update({k: d[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step",
                                            "scaling", "dtype")})
            entry["workload"] = d["config"]["workload"]
            entry["turn_driver"] = d["config"].get("turn_driver")
            entry["rccl_ranks"] = d["config"].get("rccl_ranks")
        except Exception as exc:
            entry["error"] = str(exc)[:300]
        try:
            out = json.loads(line)
            out["other_configs"] = [entry]
            line = json.dumps(out)
        except ValueError:
            pass
    print(line)


class Ranks:
    """This process's place in the job: one rank per GPU. world > 1 (or NLSG_BENCH_FORCE_DIST=1)
    opens a torch.distributed process group — RCCL; gloo under NLSG_BENCH_REHEARSAL=1 — which the
    sharded workloads use for their exchange and every workload uses for the barrier and the
    max-over-ranks of the timed region."""

    def __init__(self, args):
        import torch
        self.torch = torch
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        if self.world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={self.world}")
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (no CPU fallback)")
        self.local_rank = rehearsal_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(self.local_rank)
        self.device = torch.device("cuda", self.local_rank)
        # NLSG_BENCH_FORCE_DIST=1 exercises the sharded/RCCL path with a single rank (self-test)
        self.distributed = self.world > 1 or os.environ.get("NLSG_BENCH_FORCE_DIST") == "1"
        self.dist = None
        if self.distributed:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                # ranks cannot agree on a port by themselves: a launcher (or spawn_ranks) names it;
                # only the single-rank self-test may pick any free one
                if self.world > 1:
                    raise SystemExit("WORLD_SIZE > 1 needs MASTER_PORT (set by the launcher)")
                os.environ["MASTER_PORT"] = str(free_port())
            dist.init_process_group(**pg_args(self.rank, self.world, self.device))
            self.dist = dist

    def barrier(self):
        if self.distributed:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def max_over_ranks(self, value):
        if not self.distributed:
            return value
        t = self.torch.tensor([value], dtype=self.torch.float64,
                              device="cpu" if self.dist.get_backend() == "gloo" else self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def min_over_ranks(self, value):
        return -self.max_over_ranks(-value)

    def slice_seed(self, base):
        """Replica workloads (independent problems, no collective): rank r solves problems
        [r * batch, (r + 1) * batch) of a global batch of world * batch, drawn from its own
        stream so that no two ranks hold the same problem."""
        return (base + 7919 * self.rank) % 2**32

    def replicas(self):
        return (f"replicas x{self.world}: disjoint slices of {self.world} x batch independent "
                "problems, no data-path collective")

    def close(self):
        if self.distributed:
            self.dist.barrier()
            self.dist.destroy_process_group()


def cpu_baseline():
    """Reference DE (unmodified nlsolver.h, built into oracle/_ref) timed on this host's
    cores; falls back to the oracle port when the reference binary is absent."""
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    gens = 200
    if os.path.exists(drv):
        out = subprocess.check_output([drv, "bench-de", str(D), str(POP_PER_GPU), str(gens)],
                                      text=True)
        r = json.loads(out)
        return {"value": r["candidate_evals_per_s"], "unit": "candidate-evals/s", "cores": 1,
                "kind": "reference",
                "sample": f"reference DE<random> Rosenbrock-{D}D pop={POP_PER_GPU}, "
                          f"{gens} generations ({r['fcalls']} evals, {r['seconds']:.1f} s), "
                          "1 thread (library is single-threaded by design)"}
    from tests import _oracle as O
    lib = O.load()
    threads = os.cpu_count() or 1
    run = O.DESyncRun(lib, "rosenbrock", POP_PER_GPU, D, np.full(D, 4.096), eps=0.0,
                      max_iter=10**9, best_val_no_change=10**9)
    t0 = time.perf_counter()
    run.step(gens, threads=threads)
    dt = time.perf_counter() - t0
    return {"value": POP_PER_GPU * gens / dt, "unit": "candidate-evals/s", "cores": threads,
            "kind": "port",
            "sample": f"oracle sync DE Rosenbrock-{D}D pop={POP_PER_GPU}, {gens} generations, "
                      f"OpenMP {threads} threads"}


def host_threads():
    """Cores this process may really use: the affinity mask, capped by the cgroup CPU quota (a GPU
    box shows all host cores but grants a share of them) and by 16, the share of a one-GPU box."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 16))


def cpu_baseline_all_cores():
    """SURVEY §8(d)'s second CPU figure: the batched CPU restatement (oracle's synchronous DE, the
    algorithm the GPU runs) with OpenMP over agents on all of this host's cores."""
    from tests import _oracle as O
    lib = O.load()
    threads = host_threads()
    gens = 1500
    run = O.DESyncRun(lib, "rosenbrock", POP_PER_GPU, D, np.full(D, 4.096), eps=0.0,
                      max_iter=10**9, best_val_no_change=10**9)
    run.step(5, threads=threads)
    t0 = time.perf_counter()
    run.step(gens, threads=threads)
    dt = time.perf_counter() - t0
    return {"value": POP_PER_GPU * gens / dt, "unit": "candidate-evals/s", "cores": threads,
            "kind": "port",
            "sample": f"oracle synchronous DE (keyed draws) Rosenbrock-{D}D pop={POP_PER_GPU}, "
                      f"{gens} generations ({dt:.1f} s), OpenMP over agents, {threads} threads"}


CONSISTENCY_VIOLATIONS = []
MIN_TIMED_S = 0.050  # every timed region is repeated until it covers at least this much wall time


def check_kernel_within_step(kernel_ms, ms_per_step, what):
    """A line is self-consistent only if the dominant kernel fits into the step that contains it
    (3 % for timer noise between the two measurements). A violation is RECORDED — the line still
    prints, carrying `kernel_within_step: false`, and the script exits non-zero after it."""
    if os.environ.get("NLSG_BENCH_NO_CONSISTENCY_CHECK") == "1":
        return True  # counter-collection passes of the profiler stretch launches unevenly
    ok = kernel_ms <= 1.03 * ms_per_step
    if not ok:
        CONSISTENCY_VIOLATIONS.append(f"{what}: roofline.kernel_ms {kernel_ms:.4f} > ms_per_step "
                                      f"{ms_per_step:.4f}: the two describe different regimes")
    return ok


def timed_steps(ranks, stepper, steps, min_s=MIN_TIMED_S):
    """The contract's timed region — barrier + synchronize on both sides, max over ranks — around
    `steps` steps, REPEATED until the region covers min_s (a 20-step run of 47 us turns is
    0.9 ms: one clock ramp away from noise). Every rank repeats the same number of times (agreed
    on the slowest rank's first repetition). min_s = 0 times exactly `steps` steps.
    Returns (seconds, steps actually timed)."""
    ranks.barrier()
    t0 = time.perf_counter()
    stepper(steps)
    ranks.barrier()
    dt = ranks.max_over_ranks(time.perf_counter() - t0)
    total, done = dt, steps
    extra = int(np.ceil(min_s / max(dt, 1e-9))) - 1
    if extra > 0:
        ranks.barrier()
        t0 = time.perf_counter()
        stepper(steps * extra)
        ranks.barrier()
        total += ranks.max_over_ranks(time.perf_counter() - t0)
        done += steps * extra
    return total, done


DUMP_POP_ROWS = 16384        # population rows --dump-outputs writes: 16 MiB at D = 128
DUMP_SCORES_MAX = 1 << 22    # scores of every agent up to 32 MiB, the same row sample past it


def dump_rows(n):
    """The population rows --dump-outputs writes: all n, or a fixed seeded sample of DUMP_POP_ROWS
    of them in ascending order."""
    if n <= DUMP_POP_ROWS:
        return np.arange(n)
    return np.sort(np.random.default_rng(20240917).choice(n, DUMP_POP_ROWS, replace=False))


def dump_de_outputs(dirname, eng, st, population, scores):
    """--dump-outputs: what the timed path left a caller after its last step, as float64 .npy files
    (at most 16 + 32 MiB in all): the scores of every agent, the best agent, a status vector
    (best f, best index, iteration, function calls, std_err) and the population rows dump_rows
    picks. The same run arguments give the same inputs, so two builds can be compared file for
    file."""
    os.makedirs(dirname, exist_ok=True)
    n = len(scores)
    rows = dump_rows(n)
    best_x, best_f, best_index = eng.best()
    arrays = {"population_sample": population[rows],
              "scores": scores if n <= DUMP_SCORES_MAX else scores[rows],
              "best_x": best_x,
              "status": [best_f, best_index, st.iteration, st.function_calls_used, st.std_err]}
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.asarray(a, dtype=np.float64))


def ref_baseline(cmd, key, unit, sample):
    """Times the unmodified reference (oracle/_ref/ref_driver <cmd>) on this host, 1 thread."""
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    if not os.path.exists(drv):
        return None
    r = json.loads(subprocess.check_output([drv, *map(str, cmd)], text=True))
    return {"value": r[key], "unit": unit, "cores": 1, "kind": "reference",
            "sample": f"{sample} ({r['seconds']:.1f} s), 1 thread (library is single-threaded by design)"}


PMC_DIRS = ("profiles/r04", "profiles/r03", "profiles/r02", "profiles/r01")  # newest first


def pmc_traffic(pop_local):
    """HBM bytes per launch of de_generation_kernel from the committed rocprofv3 PMC passes
    (profiles/rNN/de_pmc_summary.json; separate FETCH_SIZE / WRITE_SIZE runs of this script),
    corrected as MI355X_MICROARCH.md prescribes: FETCH_SIZE counts half of wide coalesced
    reads on gfx950 (calibrated on de_scan_partial_kernel's known 8 B/agent), WRITE_SIZE exact;
    both in KiB. The figure is read from the committed profile, not measured in this run:
    `traffic_source` names the file. None when no profile exists for this population size."""
    tag = {65536: "c2b", 1048576: "nsb"}.get(pop_local)
    for d in PMC_DIRS:
        path = os.path.join(ROOT, d, "de_pmc_summary.json")
        if tag is None or not os.path.exists(path):
            continue
        prof = json.load(open(path)).get(tag, {})
        pick = lambda ctr: next((v["mean_KiB"] for k, v in prof.get(ctr, {}).items()
                                 if "de_generation_kernel" in k), None)
        fetch, write = pick("FETCH_SIZE"), pick("WRITE_SIZE")
        if fetch is not None and write is not None:
            return {"traffic": (2.0 * fetch + write) * 1024.0,
                    "traffic_source": f"{d}/de_pmc_summary.json[{tag}] (committed rocprofv3 --pmc "
                                      "passes of this script; not collected in this run)"}
    return {"traffic": None, "traffic_source": None}


def pmc_bytes(tag, kernels, default_sizes=True):
    """HBM bytes per launch summed over `kernels` (name fragments) from the committed PMC passes
    of `bench.py --workload <tag>` at its default size (profiles/rNN/pmc_summary.json, made by
    profiles/summarize_pmc.py): 2 x FETCH_SIZE + WRITE_SIZE KiB, the gfx950 correction of
    MI355X_MICROARCH.md. traffic None when not profiled or the run is not at the default size."""
    for d in PMC_DIRS:
        path = os.path.join(ROOT, d, "pmc_summary.json")
        if not default_sizes or not os.path.exists(path):
            continue
        prof = json.load(open(path)).get(tag, {})
        total = 0.0
        for frag in kernels:
            f = next((v["mean_KiB"] for k, v in prof.get("FETCH_SIZE", {}).items() if frag in k), None)
            w = next((v["mean_KiB"] for k, v in prof.get("WRITE_SIZE", {}).items() if frag in k), None)
            if f is None or w is None:
                total = None
                break
            total += (2.0 * f + w) * 1024.0
        if total is not None:
            return {"traffic": total,
                    "traffic_source": f"{d}/pmc_summary.json[{tag}] (committed rocprofv3 --pmc "
                                      "passes of this script; not collected in this run)"}
    return {"traffic": None, "traffic_source": None}


def main_bfgs(args):
    """BASELINE configs[2]: BFGS on the convex quadratic, dim=1024, batch=4096 independent
    starts on one GPU. One step = one BFGS iteration of every problem (stop tests, direction,
    More-Thuente search, rank-2 inverse-Hessian update). Replicas only across GPUs (problems
    are independent, no collective)."""
    import math

    import torch

    import nlsolver_amd
    n = 1024
    batch = 4096 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    local_rank = ranks.local_rank
    d = np.array([1.0 + 9.0 * i / (n - 1) for i in range(n)])
    b = np.array([math.sin(0.1 * i) for i in range(n)])
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    x0 = 1.0 + 0.5 * (rng.random((batch, n)) - 0.5)
    eng = nlsolver_amd.BFGSEngine(nlsolver_amd.QuadDiagRank1(d, b, 0.01), batch,
                                  max_iter=10**9, grad_eps=0.0, alpha=1.0, device=local_rank,
                                  **({"symmetric": True} if args.bfgs_symmetric else {}),
                                  **({"reference_order": True} if args.bfgs_reference_order else {}))
    # The line describes ONE regime: iterations in which every problem streams a dense H. Iteration
    # 0 runs on H = I (never materialised); towards convergence the reset guard (nlsolver.h:
    # 3253-3260) re-identities H problem by problem and the passes skip their reads. An untimed
    # pre-pass (it also wakes the device up) finds the window: `dense_upto` = the number of
    # leading iterations after which no problem has been reset or has stopped.
    eng.init(x0)
    eng.step(2)
    dense_upto = 2
    while dense_upto < 64 and eng.identity_count() == 0 and eng.unfinished() == batch:
        dense_upto += 1
        eng.step(1)
    dense_upto -= 1  # the iteration that produced the first reset is outside the window
    dense_upto = int(ranks.min_over_ranks(dense_upto))
    warm = max(1, min(args.warmup, 4))
    steps = max(1, min(args.steps, 40, dense_upto - warm))
    eng.init(x0)
    eng.step(warm)
    ranks.barrier()
    t0 = time.perf_counter()
    eng.step(steps)
    ranks.barrier()
    dt = ranks.max_over_ranks(time.perf_counter() - t0)
    dense_verified = eng.identity_count() == 0 and eng.unfinished() == batch
    # the two H passes alone (hipEvents inside the iteration), same window: iterations k0 .. k0+3
    k0 = max(1, min(8, dense_upto - 4))
    eng.init(x0)
    eng.step(k0)
    total_ms, hess_ms = eng.time_steps(4)
    hess_ms /= 4
    # what a whole run to the rounding floor averages (identity-H iterations included): reported
    # beside `value`, never as it
    eng.init(x0)
    eng.step(warm)
    ranks.barrier()
    t1 = time.perf_counter()
    eng.step(44)
    ranks.barrier()
    dt_run = ranks.max_over_ranks(time.perf_counter() - t1)
    open_ = eng.unfinished()
    # literal: read H (t = H y) + read & write H (update); symmetric: the upper blocks only
    bytes_per_iter = (eng.hessian_bytes_per_iteration() if args.bfgs_symmetric
                      else 3 * n * n * 8) * batch
    achieved = bytes_per_iter / (hess_ms * 1e-3) / 1e9
    within = check_kernel_within_step(hess_ms, dt / steps * 1e3, "bfgs")
    ref_order = None
    if not args.bfgs_symmetric and not args.bfgs_reference_order:
        # the same iterations in REFERENCE ORDER (what the drop-in classes run: every sum in the reference's
        # index order, its results bit for bit; H passes with a lane per row), reported beside `value`
        eng.close()
        eng = nlsolver_amd.BFGSEngine(nlsolver_amd.QuadDiagRank1(d, b, 0.01), batch, max_iter=10**9,
                                      grad_eps=0.0, alpha=1.0, device=local_rank, reference_order=True)
        eng.init(x0)
        eng.step(warm)
        ranks.barrier()
        t2 = time.perf_counter()
        eng.step(steps)
        ranks.barrier()
        dt_ref = ranks.max_over_ranks(time.perf_counter() - t2)
        eng.init(x0)
        eng.step(k0)
        _, hess_ref = eng.time_steps(4)
        ref_order = {"value": ranks.world * batch * steps / dt_ref, "ms_per_step": dt_ref / steps * 1e3,
                     "kernel": "bfgs_hy_seq_kernel + bfgs_denom_seq_kernel + bfgs_update_seq_kernel",
                     "kernel_ms": hess_ref / 4,
                     "achieved_GBs": bytes_per_iter / (hess_ref / 4 * 1e-3) / 1e9}
    if ranks.rank == 0:
        print(json.dumps({
            "kernel_within_step": within,
            "metric": "BFGS iterations x problems / s (quadratic dim=1024)",
            "value": ranks.world * batch * steps / dt, "unit": "iteration-problems/s",
            "n_gpus": ranks.world, "steps": steps,
            "warmup": warm, "ms_per_step": dt / steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BFGS + More-Thuente, convex quadratic dim={n}, batch={batch} "
                                   "independent starts per GPU (BASELINE configs[2]), "
                                   f"{'symmetric (upper blocks of H)' if args.bfgs_symmetric else 'literal'}"
                                   f" rank-2 update{', reference order' if args.bfgs_reference_order else ''}",
                       **({"reference_order": ref_order} if ref_order else {}),
                       "timed_iterations": f"{warm} .. {warm + steps - 1} of a fresh run: every problem "
                                           "streams a dense inverse Hessian",
                       "dense_h_iterations_available": dense_upto, "dense_h_verified": dense_verified,
                       "whole_run": {"value": ranks.world * batch * 44 / dt_run,
                                     "ms_per_step": dt_run / 44 * 1e3, "iterations": f"{warm} .. {warm + 43}",
                                     "note": "includes the iterations after the quadratic has converged, "
                                             "in which the reset guard keeps H = I and the passes "
                                             "skip their reads"},
                       "unfinished_problems": open_, "parallelism": ranks.replicas()},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS,
                         **pmc_bytes("bfgs_sym" if args.bfgs_symmetric else "bfgs",
                                     ["bfgs_sym_hy_kernel", "bfgs_sym_update_kernel"] if args.bfgs_symmetric
                                     else ["bfgs_hy_kernel", "bfgs_update_kernel"],
                                     batch == 4096 and not args.bfgs_reference_order),
                         "kernel": ("bfgs_sym_hy_kernel + bfgs_sym_update_kernel" if args.bfgs_symmetric
                                    else "bfgs_hy_seq_kernel + bfgs_denom_seq_kernel + bfgs_update_seq_kernel"
                                    if args.bfgs_reference_order
                                    else "bfgs_hy_kernel + bfgs_update_kernel"), "kernel_ms": hess_ms,
                         "algorithmic_bytes_per_launch": bytes_per_iter},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-bfgs", n, 24], "iterations_per_s", "iteration-problems/s",
                f"reference BFGS, same quadratic dim={n}, 24 starts x 50 iterations")})}))
    eng.close()
    ranks.close()


def main_bfgs_fd(args):
    """BFGS with the reference's DEFAULT gradient (fin_diff, nlsolver.h:1385-1413) on the device:
    Rosenbrock-128D, batch = 4096 independent starts, 20 iterations, in REFERENCE ORDER — what the
    drop-in classes run for this model (every sum in the reference's index order: its results bit for
    bit). One step = one BFGS iteration of every problem; each gradient is 4 n = 512 probes of 128
    terms, a probe per lane on the base point's shared prefix sums. The tree-order
    kernels (a probe per wave) are timed beside it as `tree_order`."""
    import nlsolver_amd
    n, iters = 128, 20
    batch = 4096 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    x0 = 0.8 + 0.4 * (rng.random((batch, n)) - 0.5)

    def run(reference_order):
        eng = nlsolver_amd.BFGSEngine("rosenbrock", batch, dim=n, max_iter=iters, grad_eps=0.0,
                                      alpha=1.0, device=ranks.local_rank, reference_order=reference_order)
        eng.init(x0)
        eng.step(2)
        reps, dt = 1, 0.0
        while True:  # whole solves until the timed region covers MIN_TIMED_S
            ranks.barrier()
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.init(x0)
                eng.step(iters + 1)  # the last turn only fires the stop test and evaluates f once
            ranks.barrier()
            dt = ranks.max_over_ranks(time.perf_counter() - t0)
            if dt >= MIN_TIMED_S:
                break
            reps = int(np.ceil(reps * MIN_TIMED_S / max(dt, 1e-6) * 1.1))
        x, st = eng.download()
        eng.close()
        assert all(s.done and s.iteration == iters for s in st)
        return dt / reps, st, reps

    dt_tree, _, _ = run(False)
    dt, st, reps = run(True)
    fcalls = sum(s.function_calls_used for s in st)
    if ranks.rank == 0:
        print(json.dumps({
            "metric": "BFGS iterations x problems / s (Rosenbrock-128D, finite-difference gradient)",
            "value": ranks.world * batch * iters / dt, "unit": "iteration-problems/s",
            "n_gpus": ranks.world, "steps": iters, "solves_timed": reps,
            "warmup": 2, "ms_per_step": dt / iters * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BFGS + More-Thuente, default fin_diff gradient, Rosenbrock-{n}D, "
                                   f"batch={batch} independent starts per GPU, reference order",
                       "objective_calls_per_s": ranks.world * fcalls / dt,
                       "tree_order": {"value": ranks.world * batch * iters / dt_tree,
                                      "ms_per_step": dt_tree / iters * 1e3},
                       "mean_final_f": float(np.mean([s.f_value for s in st])),
                       "parallelism": ranks.replicas()},
            "roofline": {"bound": "latency", "achieved": None, "peak": None, "unit": None,
                         "frac": None, "traffic": None, "kernel": "bfgs_search_kernel",
                         "kernel_ms": dt / iters * 1e3,
                         "note": "serial prefix and tail chains of the probes (a lane each) and the line "
                                 "search's dependent decisions; not roofline-graded"},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-bfgs-fd", n, 256, iters], "iterations_per_s", "iteration-problems/s",
                f"reference BFGS, default fin_diff gradient, Rosenbrock-{n}D, 256 starts x {iters} "
                "iterations")})}))
    ranks.close()


def timed_solves(ranks, eng, x0, reps):
    """The contract's bracket around an engine's own event-timed solves (inputs resident, the
    start points re-uploaded outside the events): barrier + synchronize on both sides, the
    slowest rank's milliseconds per solve."""
    ranks.barrier()
    ms = ranks.max_over_ranks(eng.time_solve(x0, reps) / reps)
    ranks.barrier()
    if ms * reps < MIN_TIMED_S * 1e3:  # too short a region: once more, long enough (same count on every rank)
        reps = int(np.ceil(MIN_TIMED_S * 1e3 / max(ms, 1e-6)))
        ms = ranks.max_over_ranks(eng.time_solve(x0, reps) / reps)
        ranks.barrier()
    ranks.solves_timed = reps
    return ms


def main_nmpso(args):
    """Batched Nelder-Mead / PSO hybrid: Rosenbrock-32D (97 particles per
    instance), 4096 independent instances, 100 iterations (eps = 0, no early stop). One step = one
    iteration of every instance: sort, simplex step on the best 33 particles, PSO move + evaluation
    of the other 64."""
    import nlsolver_amd
    n, iters = 32, 100
    batch = 4096 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    x0 = 0.5 + 1.0 * (rng.random((batch, n)) - 0.5)
    eng = nlsolver_amd.NMPSOEngine("rosenbrock", batch, n, max_iter=iters, eps=0.0,
                                   no_change_best_iter=2**62, device=ranks.local_rank,
                                   inst_lo=ranks.rank * batch)
    x, st = eng.minimize(x0)
    ms = timed_solves(ranks, eng, x0, 3)
    evals = sum(s.function_calls_used for s in st)
    assert all(s.iteration == iters for s in st)
    if ranks.rank == 0:
        print(json.dumps({
            "metric": "NelderMeadPSO objective evaluations x instances / s (Rosenbrock-32D)",
            "value": ranks.world * evals / (ms * 1e-3), "unit": "particle-evals/s",
            "n_gpus": ranks.world, "steps": iters,
            "warmup": iters, "ms_per_step": ms / iters, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"NelderMeadPSO, Rosenbrock-{n}D, batch={batch} independent "
                                   f"instances of {3 * n + 1} particles per GPU, {iters} iterations",
                       "iteration_instances_per_s": ranks.world * batch * iters / (ms * 1e-3),
                       "mean_best_f": float(np.mean([s.f_value for s in st])),
                       "parallelism": ranks.replicas()},
            "roofline": {"bound": "valu", "achieved": None, "peak": None, "unit": None,
                         "frac": None, "traffic": None, "kernel": "nmpso_solve_kernel", "kernel_ms": ms,
                         "note": "vector-issue bound (the PSO move's keyed draws) once enough instances "
                                 "per CU hide the simplex step's dependent decisions; not roofline-graded"},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-nmpso", n, 4096, iters], "evals_per_s", "particle-evals/s",
                f"reference NelderMeadPSO, Rosenbrock-{n}D, 4096 instances x {iters} iterations")})}))
    eng.close()
    ranks.close()


def main_sann(args):
    """Batched simulated annealing: Rosenbrock-128D, 16 384 independent chains, the
    reference's default temperature_iter = 10 and temperature_max = 10, 100 temperatures. One step
    = one temperature of every chain = 9 trial points (9 x 128 normal draws + one objective
    evaluation each), one wave per chain, nothing but registers between the first load and the
    last store."""
    import nlsolver_amd
    n, iters, t_iter = 128, 100, 10
    batch = 16384 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    x0 = 0.5 + 1.0 * (rng.random((batch, n)) - 0.5)
    eng = nlsolver_amd.SANNEngine("rosenbrock", batch, n, max_iter=iters, temperature_iter=t_iter,
                                  temperature_max=10.0, device=ranks.local_rank,
                                  chain_lo=ranks.rank * batch)
    x, st = eng.minimize(x0)
    ms = timed_solves(ranks, eng, x0, 3)
    trials = sum(s.function_calls_used for s in st)
    f0 = float(np.mean([((1 - r[:-1]) ** 2 + 100 * (r[1:] - r[:-1] ** 2) ** 2).sum() for r in x0[:256]]))
    if ranks.rank == 0:
        print(json.dumps({
            "metric": "SANN trial points x chains / s (Rosenbrock-128D)",
            "value": ranks.world * trials / (ms * 1e-3), "unit": "trial-points/s",
            "n_gpus": ranks.world, "steps": iters,
            "warmup": iters, "ms_per_step": ms / iters, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"SANN, Rosenbrock-{n}D, batch={batch} independent chains per GPU, "
                                   f"{iters} temperatures x {t_iter - 1} trial points",
                       "normal_draws_per_s": ranks.world * trials * n / (ms * 1e-3),
                       "mean_start_f": f0, "mean_best_f": float(np.mean([s.f_value for s in st])),
                       "parallelism": ranks.replicas()},
            "roofline": {"bound": "valu", "achieved": None, "peak": None, "unit": None, "frac": None,
                         "traffic": None, "kernel": "sann_anneal_kernel", "kernel_ms": ms,
                         "note": "register-resident chains: two counter draws, log, cos, sqrt per "
                                 "coordinate and trial on the fp64 VALU; not roofline-graded"},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-sann", n, 4096, iters, t_iter], "trials_per_s", "trial-points/s",
                f"reference SANN, Rosenbrock-{n}D, 4096 chains x {iters} temperatures x {t_iter - 1} "
                "trial points")})}))
    eng.close()
    ranks.close()


def main_lm_fd(args):
    """LevenbergMarquardt with the reference's DEFAULT functors (fin_diff + fin_diff_h,
    nlsolver.h:3494-3511) on the device: Rosenbrock-16D, batch = 8192 independent starts, 10
    iterations, in REFERENCE ORDER — what the drop-in classes run for this model (every sum in the
    reference's index order: its results bit for bit). One step = one LM iteration of every problem =
    1 + 4 n + 16 n^2 = 4161 objective evaluations per problem, a probe per lane on the base point's
    shared terms. The tree-order kernels (a probe per group of lanes) are timed beside
    it as `tree_order`."""
    import nlsolver_amd
    from nlsolver_amd._capi import LM_CHOLESKY, LM_CHOLESKY_REFERENCE_ORDER
    n, iters = 16, 10
    batch = 8192 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    x0 = 0.8 + 0.4 * (rng.random((batch, n)) - 0.5)
    with nlsolver_amd.lm.LMEngine("rosenbrock", batch=batch, n=n, lam=10.0, max_iter=iters, f_delta=0.0,
                                  device=ranks.local_rank, solver=LM_CHOLESKY) as tree_eng:
        tree_eng.minimize(x0.copy())
        ms_tree = timed_solves(ranks, tree_eng, x0, 5)
    eng = nlsolver_amd.lm.LMEngine("rosenbrock", batch=batch, n=n, lam=10.0, max_iter=iters,
                                   f_delta=0.0, device=ranks.local_rank, solver=LM_CHOLESKY_REFERENCE_ORDER)
    x, st, lam = eng.minimize(x0.copy())
    ms = timed_solves(ranks, eng, x0, 5)
    fcalls = sum(s.function_calls_used for s in st)
    assert all(s.iteration == iters for s in st)
    if ranks.rank == 0:
        print(json.dumps({
            "metric": "LM iterations x problems / s (Rosenbrock-16D, finite-difference gradient and Hessian)",
            "value": ranks.world * batch * iters / (ms * 1e-3), "unit": "iteration-problems/s",
            "n_gpus": ranks.world,
            "steps": iters, "warmup": iters, "ms_per_step": ms / iters, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"Levenberg-Marquardt, default fin_diff / fin_diff_h functors, "
                                   f"Rosenbrock-{n}D, batch={batch} independent starts per GPU, reference order",
                       "objective_calls_per_s": ranks.world * fcalls / (ms * 1e-3),
                       "tree_order": {"value": ranks.world * batch * iters / (ms_tree * 1e-3),
                                      "ms_per_step": ms_tree / iters},
                       "finite_final_f": int(np.sum(np.isfinite([s.f_value for s in st]))),
                       "parallelism": ranks.replicas()},
            "roofline": {"bound": "valu", "achieved": None, "peak": None, "unit": None,
                         "frac": None, "traffic": None, "kernel": "lm_fd_iter_kernel",
                         "kernel_ms": ms / (iters + 1),
                         "note": "fp64 VALU issue bound (the probes' chains, a lane each); "
                                 "not roofline-graded"},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-lm-fd", n, 16384, iters], "iterations_per_s", "iteration-problems/s",
                f"reference LevenbergMarquardt, default functors, Rosenbrock-{n}D, 16384 starts x "
                f"{iters} iterations")})}))
    eng.close()
    ranks.close()


def main_lm(args):
    """BASELINE configs[3]: Levenberg-Marquardt NLLS m=512, n=64, batch=8192 on one GPU
    (tanh regression, 20 iterations, lambda0 = 10, up = down = 10, f_delta = 0). One step = one
    LM iteration of every problem: residuals + J^T J (fp64 MFMA) + J^T r, damped solve, update.
    Cholesky solver (the reference class's own get_update_with_hessian): one launch per iteration
    for all problems in lock step (one wave per problem: step, then evaluation); QR solver
    (tinyqr::lm, as BASELINE words the config): a step kernel between evaluation launches. The
    line's `value` is the solver --lm-solver names; the other solver is timed in the same run on
    the same resident data and reported as `config.other_solver`. The timed region is the whole
    solve divided by its iteration count; the roofline object describes the evaluation kernel
    (shared by both solvers) timed on its own."""
    import nlsolver_amd
    m, n, iters = 512, args.lm_n, 20
    wide = n > 64  # workgroup-per-problem kernels; the class's own (Cholesky) solve only
    if wide and args.lm_solver != "cholesky":
        raise SystemExit("--lm-n > 64: the tinyqr solve is built for n <= 64")
    batch = (1024 if wide else 8192) if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    # the design matrices are built in page-locked memory (nlsolver_amd.pinned_empty): the upload
    # at engine creation is then DMA at the link's rate (--lm-pageable: ordinary memory)
    A = np.empty((batch, m, n)) if args.lm_pageable else nlsolver_amd.pinned_empty((batch, m, n))
    for b0 in range(0, batch, 512):
        A[b0:b0 + 512] = (2 * rng.random((min(512, batch - b0), m, n)) - 1) / np.sqrt(n)
    star = 2 * rng.random((batch, n)) - 1
    y = np.tanh(np.einsum("bmn,bn->bm", A, star))
    theta0 = 0.5 * star + 0.1 * (2 * rng.random((batch, n)) - 1)
    from nlsolver_amd import _capi
    model = nlsolver_amd.TanhRegression(A, y)
    solvers = {"cholesky": _capi.LM_CHOLESKY, "qr": _capi.LM_QR}
    t_up = time.perf_counter()
    eng = nlsolver_amd.LMEngine(model, lam=10.0, max_iter=iters, f_delta=0.0,
                                device=ranks.local_rank, solver=solvers[args.lm_solver])
    # the boundary hands over HOST buffers (A: 2 GiB at batch 8192): engine creation = allocation
    # + upload + device repack; reported beside `value`, never inside it
    upload_s = time.perf_counter() - t_up
    eng.time_solve(theta0, 3)  # warm-up (three solves, ~45 ms: a fresh process starts at idle clocks)
    ms = timed_solves(ranks, eng, theta0, 3)
    th, st, lam = eng.minimize(theta0.copy())
    # the other solver on the same resident data
    other_name = "qr" if args.lm_solver == "cholesky" else "cholesky"
    if not wide:
        eng.set_solver(solvers[other_name])
        eng.time_solve(theta0, 1)
        ms_other = timed_solves(ranks, eng, theta0, 3)
        th_o, st_o, _ = eng.minimize(theta0.copy())
        eng.set_solver(solvers[args.lm_solver])
    evals = iters + 1
    npad = 64 if not wide else n
    hbm_eval = (m * npad * 8 + m * 8) * batch  # A and y streamed once per evaluation
    # the evaluation launch (both solvers share it), timed on its own: ten lower 16 x 16 tiles of
    # J^T J per 4-row k-step are what the matrix cores execute (the matrix is symmetric)
    eng.time_eval_kernel(theta0, 60)  # untimed: clocks back up after the host-side pauses
    kname = ("lm_wide128x8_tanh_eval_kernel" if 64 < n <= 128 else "lm_wide256x8_tanh_eval_kernel" if 128 < n <= 256
             else "lm_wide_mfma_tanh_eval_kernel" if wide else "lm_iter_kernel (evaluation-only launches)")
    kms = eng.time_eval_kernel(theta0, 20) / 20
    # executed on the matrix cores: the lower 16 x 16 tiles of J^T J (the matrix is bitwise
    # symmetric), 2 * 16 * 16 flop per tile and row — 10 tiles at n = 64, 36 at n = 128
    nb = (n + 15) // 16
    flops = 2.0 * m * (nb * (nb + 1) // 2) * 256 * batch
    tflops = flops / (kms * 1e-3) / 1e12
    hbm_gbps = hbm_eval / (kms * 1e-3) / 1e9
    within = check_kernel_within_step(kms, ms / iters, "lm")
    if ranks.rank == 0:
        print(json.dumps({
            "kernel_within_step": within, "solves_timed": getattr(ranks, "solves_timed", None),
            "metric": f"LM iterations x problems / s (NLLS m=512 n={n})",
            "value": ranks.world * batch * iters / (ms * 1e-3), "unit": "iteration-problems/s",
            "n_gpus": ranks.world,
            "steps": iters, "warmup": 1, "ms_per_step": ms / iters, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"Levenberg-Marquardt tanh-regression NLLS m={m} n={n}, "
                                   f"batch={batch} per GPU ({'BASELINE configs[3]' if n == 64 else 'past the one-wave size'}), "
                                   f"{args.lm_solver} solve",
                       "solver": args.lm_solver,
                       "max_final_f": max(s.f_value for s in st),
                       # what an iteration spends outside the evaluation launch (the damped solve)
                       "solve_ms_per_iteration": ms / iters - kms * evals / iters,
                       **({} if wide else {"other_solver": {
                           "solver": other_name,
                           "value": ranks.world * batch * iters / (ms_other * 1e-3),
                           "ms_per_step": ms_other / iters,
                           "solve_ms_per_iteration": ms_other / iters - kms * evals / iters,
                           "max_final_f": max(s.f_value for s in st_o),
                           "max_rel_diff_theta": float(np.max(np.abs(th_o - th) /
                                                              (1e-300 + np.abs(th))))}}),
                       # host buffers in, host buffers out: data upload + one whole solve
                       "upload_s": upload_s, "upload_GBps": (A.nbytes + y.nbytes) / upload_s / 1e9,
                       "upload_from": "pageable host memory" if args.lm_pageable
                                      else "page-locked host memory (nlsg_host_alloc)",
                       "pcie_inclusive_value": batch * iters / (upload_s + ms * 1e-3),
                       "parallelism": ranks.replicas()},
            # achieved / frac are on SURVEY §8d's ALGORITHMIC count m n (n + 1) (J^T J exploiting
            # symmetry); what the matrix cores execute — whole lower 16 x 16 tiles, 10 at n = 64, 36 at
            # n = 128: 11 % more — is reported beside it
            "roofline": {"bound": "mfma", "achieved": m * n * (n + 1) * batch / (kms * 1e-3) / 1e12,
                         "peak": 78.6, "unit": "TFLOP/s",
                         "frac": m * n * (n + 1) * batch / (kms * 1e-3) / 1e12 / 78.6,
                         "frac_executed_tiles": tflops / 78.6,
                         **pmc_bytes("lm", ["lm_iter_kernel"], batch == 8192 and not wide),
                         "kernel": kname,
                         "kernel_ms": kms, "algorithmic_flops_per_launch": float(m * n * (n + 1) * batch),
                         "executed_tile_flops_per_launch": flops,
                         # SURVEY §8d's counts: m n (n + 1) exploiting symmetry, 2 m n^2 without
                         "frac_on_m_n_n1": m * n * (n + 1) * batch / (kms * 1e-3) / 1e12 / 78.6,
                         "frac_on_2_m_n2": 2.0 * m * n * n * batch / (kms * 1e-3) / 1e12 / 78.6,
                         "hbm_GBps": hbm_gbps, "hbm_frac": hbm_gbps / 8000.0},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-lm", m, n, 256 if n <= 64 else 48, iters], "iterations_per_s", "iteration-problems/s",
                f"reference LevenbergMarquardt + GN functors, m={m} n={n}, {256 if n <= 64 else 48} problems x {iters} "
                "iterations")})}))
    eng.close()
    ranks.close()


def main_tinyqr(args):
    """Batched tinyqr::lm (tinyqr.h:461-470): 8192 independent least-squares systems
    of 576 x 64 — the augmented damped system of configs[3], [J; sqrt(lambda) I] — solved side by
    side by Givens QR (`nlsg_tinyqr_lm`). One step = one batch solved; the systems are resident in
    HBM inside the timed region (the kernel's HIP events), the PCIe legs are reported beside it."""
    import nlsolver_amd
    n, p = 576, 64
    batch = 8192 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(12374563468 % 2**32))
    X = 2 * rng.random((batch, p, n)) - 1
    y = 2 * rng.random((batch, n)) - 1
    steps = max(2, min(args.steps, 5))
    nlsolver_amd.tinyqr.lm(X, y, device=ranks.local_rank)  # warm-up
    ranks.barrier()
    t0 = time.perf_counter()
    ms = []
    for _ in range(steps):
        beta, k_ms = nlsolver_amd.tinyqr.lm(X, y, device=ranks.local_rank, return_ms=True)
        ms.append(k_ms)
    ranks.barrier()
    wall = ranks.max_over_ranks(time.perf_counter() - t0)
    kms = ranks.max_over_ranks(sum(ms) / len(ms))
    resid = y[:64] - np.einsum("bpn,bp->bn", X[:64], beta[:64])
    ortho = float(np.max(np.abs(np.einsum("bpn,bn->bp", X[:64], resid))))
    rotations = batch * sum(n - 1 - j for j in range(p))
    if ranks.rank == 0:
        print(json.dumps({
            "metric": f"tinyqr::lm systems / s ({n} x {p} least squares)",
            "value": ranks.world * batch / (kms * 1e-3), "unit": "systems/s",
            "n_gpus": ranks.world, "steps": steps, "warmup": 1, "ms_per_step": kms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"tinyqr::lm, batch={batch} systems of {n} x {p} per GPU",
                       "givens_rotations_per_s": ranks.world * rotations / (kms * 1e-3),
                       "max_abs_Xt_residual_first_64_systems": ortho,
                       "pcie_inclusive_value": ranks.world * batch * steps / wall,
                       "parallelism": ranks.replicas()},
            "roofline": {"bound": "latency", "achieved": None, "peak": None, "unit": None,
                         "frac": None, "traffic": None, "kernel": "tinyqr_lm_kernel", "kernel_ms": kms,
                         "hbm_GBps": batch * (n * p + n + p) * 8 / (kms * 1e-3) / 1e9,
                         "note": "wavefront Givens QR: n + p - 2 dependent steps of a Givens pair (~45 "
                                 "dependent fp64 instructions) and two barriers; not roofline-graded "
                                 "(SURVEY §8d)"},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-tinyqr", n, p, 24], "systems_per_s", "systems/s",
                f"reference tinyqr::lm on 24 systems of {n} x {p}")})}))
    ranks.close()


def main_nm(args):
    """Batched Nelder-Mead (no BASELINE config names it): Rosenbrock-128D,
    2000 iterations per start, eps = 0, batch = 4096 independent simplexes, one per workgroup, the
    129 x 128 simplex resident in LDS. One step = one simplex iteration of every start."""
    import nlsolver_amd
    n, iters = 128, 2000
    batch = 4096 if args.pop_per_gpu == POP_PER_GPU else args.pop_per_gpu
    ranks = Ranks(args)
    rng = np.random.default_rng(ranks.slice_seed(7))
    x0 = 0.5 + 0.2 * (rng.random((batch, n)) - 0.5)
    eng = nlsolver_amd.NMEngine("rosenbrock", batch, n, eps=0.0, max_iter=iters,
                                no_change_best_tol=10**9, device=ranks.local_rank)
    eng.time_solve(x0, 1)
    ms = timed_solves(ranks, eng, x0, 2)
    x, st, _ = eng.minimize(x0.copy())
    fcalls = sum(s.function_calls_used for s in st)
    # the same starts in REFERENCE ORDER (what the drop-in classes run: the objective's terms and std_err's
    # sums in the reference's index order — its runs bit for bit), reported beside `value`
    with nlsolver_amd.NMEngine("rosenbrock", batch, n, eps=0.0, max_iter=iters, no_change_best_tol=10**9,
                               device=ranks.local_rank, reference_order=True) as ref_eng:
        ref_eng.time_solve(x0, 1)
        ms_ref = ranks.max_over_ranks(ref_eng.time_solve(x0, 1))
    if ranks.rank == 0:
        print(json.dumps({
            "metric": "Nelder-Mead iterations x starts / s (Rosenbrock-128D)",
            "value": ranks.world * batch * iters / (ms * 1e-3), "unit": "iteration-starts/s",
            "n_gpus": ranks.world,
            "steps": iters, "warmup": 1, "ms_per_step": ms / iters, "higher_is_better": True,
            "solves_timed": getattr(ranks, "solves_timed", None),
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"Nelder-Mead Rosenbrock-{n}D, {iters} iterations, batch={batch} per GPU",
                       "objective_calls_per_s": ranks.world * fcalls / (ms * 1e-3),
                       "reference_order": {"value": ranks.world * batch * iters / (ms_ref * 1e-3),
                                           "ms_per_step": ms_ref / iters, "kernel": "nm_solve_driver_kernel<0, true>"},
                       "parallelism": ranks.replicas()},
            "roofline": {"bound": "latency", "achieved": None, "peak": None, "unit": None,
                         # the whole solve is ONE launch of nm_solve_driver_kernel: its duration per
                         # simplex iteration is the step
                         "frac": None, "traffic": None, "kernel": "nm_solve_driver_kernel",
                         "kernel_ms": ms / iters, "launch_ms": ms,
                         "note": "LDS-resident, decision chain; not roofline-graded (SURVEY §8d)"},
            **({} if (args.no_cpu_baseline or ranks.world > 1) else {"cpu_baseline": ref_baseline(
                ["bench-nm", n, 400000], "iterations_per_s", "iteration-starts/s",
                f"reference NelderMead Rosenbrock-{n}D, one start, 400000 iterations")})}))
    eng.close()
    ranks.close()

TTS_BIN = os.path.join(ROOT, "tests", "cpp", "bin", "tts")


def tts_device(argv, timeout=600):
    """One case through the drop-in header in a FRESH process (so `cold` is a process's first
    device call): tests/cpp/tts.cpp -> include/nlsolver_mi/nlsolver.h -> dlopen -> C-ABI."""
    env = dict(os.environ, NLSG_LIBRARY=os.path.join(ROOT, "nlsolver_amd", "libnlsolver_hip.so"))
    r = subprocess.run([TTS_BIN, *map(str, argv)], capture_output=True, text=True, env=env,
                       timeout=timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not line:
        raise RuntimeError(f"tts {argv}: rc={r.returncode} {r.stdout.strip()[-200:]} {r.stderr.strip()[-200:]}")
    return json.loads(line[-1])


def tts_reference(argv, scale=1.0):
    """The unmodified reference solving the same problem on one core (oracle/_ref/ref_driver
    tts-*), or a bounded sample of the batch scaled up (`scale`); None without the binary."""
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    if not os.path.exists(drv):
        return None
    r = json.loads(subprocess.check_output([drv, *map(str, argv)], text=True))
    r["ms"] = r["seconds"] * 1e3 * scale
    r["scaled_by"] = scale
    return r


def main_tts(args):
    """Time-to-solution through the drop-in header ("honest end-to-end minimize()
    latency, not only kernel throughput"; the reference's loop nlsolver.h:2429-2447).

    Every case: `Solver<device objective, ...>(f, gen, ctor defaults).minimize(x)` to its DEFAULT
    stop rule, cold (first device call of a process) and warm (the same call again), with the
    library's phase laps; beside it the reference itself on one core solving the same problem to
    the same stop rule. `value` = warm wall time of BASELINE configs[1]'s shape (pop 65536 x D 128);
    the table's point is the break-even: below which pop x D the host path is the faster one."""
    grid = [(2, 40), (2, 4096), (2, 65536), (128, 40), (128, 4096), (128, 65536)]
    if args.tts_grid:
        grid = [(Dd, n) for Dd in (2, 16, 128) for n in (40, 256, 1024, 4096, 16384, 65536)]
    cases = []
    for Dd, n in grid:
        x0 = "5,7" if Dd == 2 else "4.096"
        dev = tts_device(["de", Dd, n])
        ref = None if args.no_cpu_baseline else tts_reference(
            ["tts-de", Dd, n, 1000, 10e-4, 50, x0])
        cases.append({"solver": "DE<device::Rosenbrock, xorshift, double, random>", "D": Dd, "pop": n,
                      "cold": dev["cold"], "warm": dev["warm"],
                      "reference_1core_ms": ref and ref["ms"], "reference_iters": ref and ref["iters"],
                      "warm_speedup": ref and ref["ms"] / dev["warm"]["wall_ms"]})
    pso = []
    for Dd, n in ([(2, 40), (128, 4096), (128, 65536)] if not args.tts_grid else
                  [(Dd, n) for Dd in (2, 16, 128) for n in (40, 1024, 16384, 65536)]):
        dev = tts_device(["pso", Dd, n])
        ref = None if args.no_cpu_baseline else tts_reference(
            ["tts-pso", Dd, n, 5000, 10e-4, 50, "2.048"])
        pso.append({"solver": "PSO<device::Rosenbrock, xorshift, double, Accelerated>", "D": Dd,
                    "particles": n, "cold": dev["cold"], "warm": dev["warm"],
                    "reference_1core_ms": ref and ref["ms"], "reference_iters": ref and ref["iters"],
                    "warm_speedup": ref and ref["ms"] / dev["warm"]["wall_ms"]})
    batch = []
    dev = tts_device(["bfgs", 1024, 4096])
    sample = 4
    ref = None if args.no_cpu_baseline else tts_reference(["tts-bfgs", 1024, sample, 100, 5e-3],
                                                          4096 / sample)
    batch.append({"solver": "BFGS<device::QuadDiagRank1>::minimize_batch (configs[2]: n 1024 x 4096 "
                            "starts, defaults max_iter 100 grad_eps 5e-3; reference order, the header's "
                            "default: the reference's results bit for bit)",
                  "cold": dev["cold"], "warm": dev["warm"], "reference_1core_ms": ref and ref["ms"],
                  "reference_sample": f"{sample} of 4096 problems, scaled",
                  "warm_speedup": ref and ref["ms"] / dev["warm"]["wall_ms"]})
    dev = tts_device(["lm", 512, 64, 8192])
    sample = 16
    ref = None if args.no_cpu_baseline else tts_reference(["tts-lm", 512, 64, sample, 100, 1e-12],
                                                          8192 / sample)
    batch.append({"solver": "LevenbergMarquardt<device::TanhRegression>::minimize_batch (configs[3]: "
                            "m 512 n 64 x 8192 problems, defaults max_iter 100 f_delta 1e-12)",
                  "cold": dev["cold"], "warm": dev["warm"], "reference_1core_ms": ref and ref["ms"],
                  "reference_sample": f"{sample} of 8192 problems, scaled",
                  "warm_speedup": ref and ref["ms"] / dev["warm"]["wall_ms"]})
    head = next(c for c in cases if c["D"] == 128 and c["pop"] == 65536)
    # break-even: the smallest population per D at which the warm device call beats the reference
    breakeven = {}
    for c in cases:
        if c["warm_speedup"] and c["warm_speedup"] >= 1.0:
            key = f"D={c['D']}"
            breakeven[key] = min(breakeven.get(key, c["pop"]), c["pop"])
    print(json.dumps({
        "metric": "time-to-solution of minimize() through the drop-in header, default stop rule",
        "value": head["warm"]["wall_ms"], "unit": "ms", "n_gpus": 1, "steps": 1, "warmup": 1,
        "ms_per_step": head["warm"]["wall_ms"], "higher_is_better": False, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "DE Rosenbrock-128D pop=65536 to the default stop (value); table: DE "
                               "pop {40, 4096, 65536} x D {2, 128}, Accelerated PSO, BFGS configs[2], "
                               "LM configs[3] — each cold (first device call of a process) and warm",
                   "phases": "create / upload / init / iterate / readback / destroy = host wall-clock "
                             "laps inside the library (nlsg_call_timing); wall_ms = the whole call",
                   "break_even_pop": breakeven},
        "cases": cases, "pso_cases": pso, "batch_cases": batch,
        "roofline": {"bound": "latency", "achieved": None, "peak": None, "unit": None, "frac": None,
                     "traffic": None, "kernel": None,
                     "note": "an end-to-end latency line, not a kernel line"},
        **({} if args.no_cpu_baseline else {"cpu_baseline": {
            "value": head["reference_1core_ms"], "unit": "ms", "cores": 1, "kind": "reference",
            "sample": "the reference's DE<random> solving the same problem to the same stop rule "
                      "(oracle/_ref/ref_driver tts-de 128 65536)"}})}))


def rehearsal_device(local_rank):
    """NLSG_BENCH_REHEARSAL=1: every rank uses GPU 0 and the ranks talk over gloo — the N > 1
    control flow of this file on a one-GPU box (RCCL refuses two ranks on one device). Numbers
    from such a run mean nothing; it exists so that the multi-rank path is executed before the
    scaling run."""
    if os.environ.get("NLSG_BENCH_REHEARSAL") != "1":
        return local_rank
    os.environ["NLSG_DIST_NATIVE"] = "0"  # host-ordered turns over gloo
    return 0


def pg_args(rank, world, device):
    if os.environ.get("NLSG_BENCH_REHEARSAL") == "1":
        return dict(backend="gloo", rank=rank, world_size=world)
    return dict(backend="nccl", rank=rank, world_size=world, device_id=device)


def main_pso(args):
    """BASELINE configs[4]: PSO swarm = 2^20 particles x D=256 sharded over 8 GPUs ->
    131072 particles per GPU (weak scaling). One step = best update + stop tests + one
    position update + evaluation of the whole swarm."""
    import nlsolver_amd
    Dp, n_local = 256, 131072
    if args.pop_per_gpu != POP_PER_GPU:
        n_local = args.pop_per_gpu
    ranks = Ranks(args)
    world, rank, local_rank, device = ranks.world, ranks.rank, ranks.local_rank, ranks.device
    distributed, dist = ranks.distributed, ranks.dist
    vanilla = args.workload == "pso-vanilla"
    n = n_local * world
    kw = dict(type=nlsolver_amd.PSO_VANILLA if vanilla else nlsolver_amd.PSO_ACCELERATED,
              bounded=False, inertia=0.8, cognitive=1.8, social=1.8, eps=0.0, max_iter=10**12,
              best_val_no_change=10**12, device=local_rank)

    drv = None
    if distributed:
        from nlsolver_amd.dist import ShardedPSO
        drv = ShardedPSO(dist, lambda lo, m_, stream: nlsolver_amd.PSOEngine(
            "rosenbrock", n, Dp, shard_lo=lo, shard_n=m_, stream=stream, **kw), n, Dp, device)
        eng = drv.engine
        stepper = drv.step
    else:
        eng = nlsolver_amd.PSOEngine("rosenbrock", n, Dp, **kw)
        stepper = eng.step
    eng.init(-2.048, 2.048)
    stepper(300)  # untimed device wake-up (see the DE benchmark), then start over
    eng.init(-2.048, 2.048)
    stepper(args.warmup)
    dt, steps_timed = timed_steps(ranks, stepper, args.steps)
    assert eng.status().iteration == args.warmup + steps_timed
    stepper(200)  # untimed, every rank (a sharded turn is collective): clocks back up after the pauses
    if rank == 0:
        launches = max(min(args.steps, 200), 20)
        kern_ms = eng.time_move_kernel(launches) / launches
        bytes_per = (40 if vanilla else 16) * Dp + 24  # rows r/w + cur/pbest values
        achieved = bytes_per * n_local / (kern_ms * 1e-3) / 1e9
        hbm = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": achieved / HBM_PEAK_GBS}
        valu = None if vanilla else valu_roofline(kern_ms, n_local, Dp)
        within = check_kernel_within_step(kern_ms, dt / steps_timed * 1e3, args.workload)
        print(json.dumps({
            "metric": "particle-evals/sec Rosenbrock-256D PSO", "value": n * steps_timed / dt,
            "unit": "particle-evals/s", "n_gpus": world, "steps": args.steps, "steps_timed": steps_timed,
            "kernel_within_step": within,
            "warmup": args.warmup, "ms_per_step": dt / steps_timed * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"Rosenbrock-{Dp}D PSO {'Vanilla' if vanilla else 'Accelerated'}"
                                   f", {n_local} particles per GPU (BASELINE configs[4] shard)",
                       "global_swarm": n, "dim": Dp,
                       "parallelism": f"swarm-sharded x{world} (one all-gather of the best record "
                                      "per iteration)",
                       "turn_driver": turn_driver(drv), "rccl_ranks": rccl_ranks(drv)},
            # The Accelerated move is bound by the vector unit ("fp64 vector ALU at the
            # ridge"; its HBM traffic equals the algorithmic bytes), so its roof is instruction issue;
            # the HBM figure rides along as `hbm`. Vanilla is HBM-bound.
            "roofline": {**(valu if valu else hbm), **({"hbm": hbm} if valu else {}),
                         **pmc_bytes("pso_vanilla" if vanilla else "pso_accel",
                                     ["pso_move_kernel"], n_local == 131072),
                         "kernel": "pso_move_kernel", "kernel_ms": kern_ms,
                         "algorithmic_bytes_per_launch": bytes_per * n_local},
            **({} if (args.no_cpu_baseline or world > 1 or vanilla) else {"cpu_baseline": ref_baseline(
                ["bench-pso", Dp, 4096, 40], "particle_evals_per_s", "particle-evals/s",
                f"reference PSO Accelerated Rosenbrock-{Dp}D, 4096 particles x 40 iterations")})}))
    if distributed:
        dist.barrier()  # no rank tears its communicator down while another is still measuring
    eng.close()
    ranks.close()


VALU_WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 4  # 1024 SIMDs, one 64-lane instruction per 4 cycles at 2.4 GHz


def valu_roofline(kern_ms, n_local, Dp):
    """Vector-issue roofline of pso_move_kernel<Accelerated>: frac = issued vector instructions x 4
    cycles / (SIMDs x peak clock x kernel time). The instruction count per launch is read from the
    committed rocprofv3 SQ_INSTS_VALU pass of this workload (profiles/rNN/pso_issue_summary.json,
    made by scripts/pmc_pso_issue.sh); None-valued when no profile matches the size."""
    insts = busy = None
    src = None
    for d in PMC_DIRS:
        path = os.path.join(ROOT, d, "pso_issue_summary.json")
        if os.path.exists(path) and n_local == 131072 and Dp == 256:
            prof = json.load(open(path))
            k = next((v for name, v in prof.items() if "pso_move_kernel" in name), None)
            if k and "SQ_INSTS_VALU" in k:
                insts = k["SQ_INSTS_VALU"]["mean"]
                if "SQ_ACTIVE_INST_VALU" in k and "SQ_BUSY_CYCLES" in k:
                    # quad-cycles the vector units were issuing / cycles x SIMDs available
                    # (SQ_BUSY_CYCLES is summed over the chip's 32 shader-engine counters)
                    busy = k["SQ_ACTIVE_INST_VALU"]["mean"] * 4 / (k["SQ_BUSY_CYCLES"]["mean"] / 32 * 1024)
                src = f"{d}/pso_issue_summary.json (committed rocprofv3 --pmc passes of this workload)"
                break
    ach = None if insts is None else insts / (kern_ms * 1e-3)
    return {"bound": "valu", "achieved": None if ach is None else ach / 1e9,
            "peak": VALU_WAVE_INSTR_PER_S / 1e9, "unit": "G wave-instructions/s",
            "frac": None if ach is None else ach / VALU_WAVE_INSTR_PER_S,
            "valu_instructions_per_launch": insts, "valu_busy_measured": busy, "valu_source": src,
            "frac_note": "frac prices every vector instruction at 4 cycles of a 2.4 GHz SIMD; under fp64 load "
                         "the chip sustains about 2.0 GHz, which is why valu_busy_measured (the counter's own "
                         "ratio, taken at the clock the run had) is the higher of the two"}


def turn_driver(drv):
    """Who orders a sharded turn: the library over its own RCCL communicator, or this host over
    torch.distributed (see nlsolver_amd.dist); None for an unsharded engine."""
    if drv is None:
        return None
    return "library (RCCL all-gather issued by the engine)" if drv.native else \
        "host (torch.distributed all_gather_into_tensor)"


def rccl_ranks(drv):
    """Communicator size as RCCL itself reports it (ncclCommCount on the engine's communicator);
    None when the exchange does not go through the library's communicator."""
    if drv is None or not drv.native:
        return None
    return drv.comm_ranks()[0]


def north_star_pass(steps, pop=1 << 20):
    """BASELINE north_star's size — pop = 2^20 x 128 fp64 (1 GiB per population buffer: out of
    reach of the 256 MiB Infinity Cache that holds configs[1]'s working set) — measured in the
    same process after the configs[1] pass: whole turns and the generation kernel alone, both by
    HIP events on the engine's stream. pop = 2^22 (4 GiB per buffer, 16x the Infinity Cache) is
    the point past ANY cache help: a quarter of a 2^20 population still fits the cache."""
    import nlsolver_amd
    steps = max(20, min(steps, 200 if pop <= (1 << 20) else 60))
    with nlsolver_amd.DEEngine("rosenbrock", pop, D, minimize=True, strategy=nlsolver_amd.DE_RANDOM,
                               CR=0.9, F=0.8, eps=1e-300, max_iter=10**12,
                               best_val_no_change=10**12, seed=12374563468) as eng:
        eng.init(np.full(D, 4.096))
        eng.step(60)  # untimed
        turn_ms = eng.time_turns(steps) / steps
        assert eng.status().iteration == 60 + steps
        kern_ms = eng.time_generation_kernel(steps) / steps
    # strategy best (nlsolver.h:2454-2457: every trial is built around the best agent) at the same
    # size: the head decides the generation's base row, so head and generation are two launches
    best = None
    if pop == (1 << 20):
        with nlsolver_amd.DEEngine("rosenbrock", pop, D, minimize=True, strategy=nlsolver_amd.DE_BEST,
                                   CR=0.9, F=0.8, eps=1e-300, max_iter=10**12,
                                   best_val_no_change=10**12, seed=12374563468) as eng:
            eng.init(np.full(D, 4.096))
            eng.step(30)  # untimed
            tb = eng.time_turns(steps) / steps
            best = {"turn_us": tb * 1e3, "value": pop / (tb * 1e-3), "unit": "candidate-evals/s"}
    achieved = BYTES_PER_CANDIDATE * pop / (kern_ms * 1e-3) / 1e9
    return {"pop": pop, "dim": D, "turns_timed": steps, "turn_us": turn_ms * 1e3,
            "value": pop / (turn_ms * 1e-3), "unit": "candidate-evals/s",
            **({"strategy_best": best} if best else {}),
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, **pmc_traffic(pop),
                         "kernel": "de_generation_kernel", "kernel_ms": kern_ms,
                         "algorithmic_bytes_per_launch": BYTES_PER_CANDIDATE * pop}}


def other_configs_pass():
    """BASELINE configs[2], [3] and [4] (their one-GPU shard) measured in the same run as the
    headline: each is this script's own --workload line, produced by a CHILD process (a fresh
    HIP context; the parent's engines are closed by now) without the CPU legs, and cut down to
    what the line is read for. A failing child costs its own entry, never the headline."""
    import subprocess
    runs = [("configs[2] BFGS dim=1024 batch=4096", ["--workload", "bfgs"]),
            ("configs[2] BFGS dim=1024 batch=4096, symmetric restatement of the rank-2 update "
             "(upper blocks of H only; values equal to rounding)", ["--workload", "bfgs", "--bfgs-symmetric"]),
            ("configs[3] Levenberg-Marquardt m=512 n=64 batch=8192, tinyqr damped solve (the solver "
             "BASELINE words: tinyqr::lm on J^T J + lambda I)", ["--workload", "lm", "--lm-solver", "qr"]),
            ("configs[3] Levenberg-Marquardt m=512 n=64 batch=8192, Cholesky damped solve (the "
             "reference class's own get_update_with_hessian)", ["--workload", "lm", "--lm-solver", "cholesky"]),
            ("configs[3] past the one-wave size: Levenberg-Marquardt m=512 n=128 batch=1024 (J^T J on fp64 "
             "MFMA in the workgroup-per-problem kernels; no BASELINE config names it)",
             ["--workload", "lm", "--lm-n", "128"]),
            ("configs[3]'s solver as a surface of its own: tinyqr::lm on 8192 systems of 576 x 64 (SURVEY "
             "row a25; latency-bound, not roofline-graded)", ["--workload", "tinyqr", "--steps", "2"]),
            ("north_star's NelderMead simplex reflect / expand / contract: Rosenbrock-128D, 4096 starts x "
             "2000 iterations (SURVEY rows a16-a17; latency-bound, not roofline-graded)", ["--workload", "nm"]),
            ("SURVEY §8f N2: BFGS with the reference's default finite-difference gradient, Rosenbrock-128D x "
             "4096 starts (reference order: the reference's runs bit for bit, a probe per lane)",
             ["--workload", "bfgs-fd"]),
            ("SURVEY §8f N2: LevenbergMarquardt with its default finite-difference functors, Rosenbrock-16D x "
             "8192 starts (reference order)", ["--workload", "lm-fd"]),
            ("configs[4] PSO Accelerated, one GPU's shard 131072 x 256",
             ["--workload", "pso-accel", "--steps", "100", "--warmup", "300"]),
            ("configs[4] PSO Vanilla, one GPU's shard 131072 x 256",
             ["--workload", "pso-vanilla", "--steps", "100", "--warmup", "300"])]
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = []
    for name, extra in runs:
        entry = {"config": name}
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra,
                               capture_output=True, text=True, timeout=240, env=env)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"rc={r.returncode}: {r.stderr.strip()[-200:]}")
            d = json.loads(line[-1])
            roof = d.get("roofline", {})
            entry.update({k: d[k] for k in ("metric", "value", "unit", "steps", "ms_per_step", "dtype")})
            entry["workload"] = d["config"]["workload"]
            entry["roofline"] = {k: roof.get(k) for k in ("bound", "achieved", "peak", "unit", "frac",
                                                          "kernel", "kernel_ms")}
            # a line is self-consistent only if its dominant kernel fits into its step
            km, sm = entry["roofline"]["kernel_ms"], entry["ms_per_step"]
            entry["kernel_within_step"] = None if km is None else bool(km <= 1.03 * sm)
            if d.get("cpu_baseline"):  # the reference binary on one core, timed by the child
                entry["cpu_baseline"] = d["cpu_baseline"]
            for k in ("steps_timed", "solves_timed"):
                if d.get(k) is not None:
                    entry[k] = d[k]
            # (reference_order / tree_order: the same workload in the other summation order)
            for k in ("solver", "solve_ms_per_iteration", "whole_run", "timed_iterations", "reference_order",
                      "tree_order"):
                if k in d["config"]:
                    entry[k] = d["config"][k]
            other = d["config"].get("other_solver")
            if other:
                entry["other_solver"] = {k: other[k] for k in ("solver", "value", "ms_per_step")}
        except Exception as exc:
            entry["error"] = str(exc)[:300]
        out.append(entry)
    return out


def tts_pass():
    """`--workload tts` (minimize() through the drop-in header to its default stop, cold and warm,
    beside the reference on one core) run by a child process and cut down to one row per case."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", "tts"],
                           capture_output=True, text=True, timeout=400, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            raise RuntimeError(f"rc={r.returncode}: {r.stderr.strip()[-200:]}")
        d = json.loads(line[-1])
        rows = []
        for c in d["cases"] + d["pso_cases"] + d["batch_cases"]:
            rows.append({"solver": c["solver"], **{k: c[k] for k in ("D", "pop", "particles") if k in c},
                         "cold_ms": c["cold"]["wall_ms"], "warm_ms": c["warm"]["wall_ms"],
                         "warm_phases_ms": {k[:-3]: c["warm"][k] for k in
                                            ("create_ms", "upload_ms", "init_ms", "iterate_ms",
                                             "readback_ms", "destroy_ms")},
                         "iters": c["warm"]["iters"], "reference_1core_ms": c["reference_1core_ms"],
                         "warm_speedup": c["warm_speedup"]})
        return {"metric": d["metric"], "unit": "ms", "break_even_pop": d["config"]["break_even_pop"],
                "rows": rows}
    except Exception as exc:
        return {"error": str(exc)[:300]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--pop-per-gpu", type=int, default=POP_PER_GPU)
    ap.add_argument("--full", action="store_true",
                    help="de workload: everything beside the headline figure as well — the accepting "
                         "regime, the generation kernel timed alone (roofline), the north_star sizes, "
                         "the CPU baselines, other_configs and time_to_solution; without it the run "
                         "sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="de workload: after the timed steps write what the last step left a caller "
                         "(scores, best agent, status, a fixed sample of population rows) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-north-star", action="store_true",
                    help="de workload, --full: skip the pop = 2^20 pass after the configs[1] pass")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="de workload, --full: skip the configs[2..4] passes (child processes) whose "
                         "summaries ride in the headline line as `other_configs`")
    ap.add_argument("--lm-solver", choices=["cholesky", "qr"], default="cholesky",
                    help="lm workload: damped-system solver whose rate is the line's value (cholesky "
                         "= the reference class's get_update_with_hessian; qr = tinyqr::lm, as "
                         "BASELINE configs[3] words it); the other one is reported beside it")
    ap.add_argument("--lm-n", type=int, default=64,
                    help="lm workload: parameters per problem (64 = BASELINE configs[3]; 65 .. 1024 run "
                         "the workgroup-per-problem kernels, batch 1024 by default)")
    ap.add_argument("--lm-pageable", action="store_true",
                    help="lm workload: hand the design matrices over from ordinary (pageable) host "
                         "memory instead of page-locked memory")
    ap.add_argument("--bfgs-symmetric", action="store_true",
                    help="bfgs workload: the symmetric restatement of the rank-2 update (streams "
                         "the upper blocks of H only) instead of the reference's literal one")
    ap.add_argument("--bfgs-reference-order", action="store_true",
                    help="bfgs workload: NLSG_BFGS_REFERENCE_ORDER (every sum in the reference's index order)")
    ap.add_argument("--workload", choices=["de", "pso-accel", "pso-vanilla", "bfgs", "bfgs-fd", "lm", "lm-fd", "nm", "sann", "nmpso", "tinyqr", "tts"],
                    default="de",
                    help="de = the headline benchmark (BASELINE metric); pso-* = config 5's "
                         "per-GPU shard (secondary, same JSON shape)")
    ap.add_argument("--tts-grid", action="store_true",
                    help="tts workload: the full pop x D grid instead of the six DE cases")
    args = ap.parse_args()
    if args.dump_outputs and args.workload != "de":
        raise SystemExit("--dump-outputs: only the de workload (the headline) writes its outputs")
    if args.workload == "tts":
        return main_tts(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args)  # before torch is imported or a GPU is touched
    if args.workload == "bfgs":
        return main_bfgs(args)
    if args.workload == "bfgs-fd":
        return main_bfgs_fd(args)
    if args.workload == "lm-fd":
        return main_lm_fd(args)
    if args.workload == "sann":
        return main_sann(args)
    if args.workload == "nmpso":
        return main_nmpso(args)
    if args.workload == "lm":
        return main_lm(args)
    if args.workload == "nm":
        return main_nm(args)
    if args.workload == "tinyqr":
        return main_tinyqr(args)
    if args.workload != "de":
        return main_pso(args)

    import nlsolver_amd

    ranks = Ranks(args)
    world, rank, local_rank, device = ranks.world, ranks.rank, ranks.local_rank, ranks.device
    distributed, dist = ranks.distributed, ranks.dist

    pop_local = args.pop_per_gpu
    pop = pop_local * world
    # eps > 0 (too small to ever fire): std_err of all scores is evaluated in every generation's
    # stop test, as DE::solve does (nlsolver.h:2443), not skipped as it may be for eps <= 0
    common = dict(minimize=True, strategy=nlsolver_amd.DE_RANDOM, CR=0.9, F=0.8, eps=1e-300,
                  max_iter=10**12, best_val_no_change=10**12, seed=12374563468,
                  device=local_rank)
    x0 = np.full(D, 4.096)

    drv = None
    if distributed:
        from nlsolver_amd.dist import ShardedDE
        drv = ShardedDE(dist, lambda lo, n, stream: nlsolver_amd.DEEngine(
            "rosenbrock", pop, D, shard_lo=lo, shard_n=n, stream=stream, **common),
            pop, D, device)
        eng = drv.engine
        stepper = drv.step
    else:
        eng = nlsolver_amd.DEEngine("rosenbrock", pop, D, **common)
        stepper = eng.step
    # No host-side pause may sit right before the timed region: ~15 ms of GPU idleness (e.g. the
    # 64 MB download below) drops the clocks and the next ~25 ms of kernels run 3-4x slower
    # (measured: the first 200 turns after the download took 36 ms instead of 9.8 ms). So the
    # reference scores are read first, then the device is kept busy (untimed) until it is timed.
    eng.init(x0)
    scores_before = eng.download()[1] if args.full else None
    stepper(2000)
    eng.init(x0)
    stepper(args.warmup)
    # exactly --steps steps: the outputs of the last step depend on warmup + steps alone
    dt, steps_timed = timed_steps(ranks, stepper, args.steps, min_s=0.0)
    st = eng.status()
    assert st.iteration == args.warmup + steps_timed, (st.iteration, args.warmup + steps_timed)
    improved = None
    if args.full or (args.dump_outputs and rank == 0):
        population, scores = eng.download()
        if args.dump_outputs and rank == 0:
            dump_de_outputs(args.dump_outputs, eng, st, population, scores)
        if args.full:
            improved = float(np.mean(scores < scores_before))

    # the same pass in a regime where selection does accept (~10 % per generation: CR = 0.2,
    # F = 0.5, x0 = 0.6): evidence that throughput does not hinge on the acceptance rate
    accepting = None
    if args.full and not distributed:
        torch = ranks.torch
        with nlsolver_amd.DEEngine("rosenbrock", pop, D, **dict(common, CR=0.2, F=0.5)) as e2:
            e2.init(np.full(D, 0.6))
            s0 = e2.download()[1]
            e2.step(2000)
            e2.init(np.full(D, 0.6))
            e2.step(args.warmup)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            e2.step(args.steps)
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t1
            accepting = {"value": pop * args.steps / dt2, "CR": 0.2, "F": 0.5, "x0": 0.6,
                         "agents_improved_frac": float(np.mean(e2.download()[1] < s0))}

    out = None
    if rank == 0:
        out = {
            "metric": "candidate-evals/sec (pop x iters/s) Rosenbrock-128D DE",
            "value": pop * steps_timed / dt,
            "unit": "candidate-evals/s",
            "n_gpus": world, "steps": args.steps, "steps_timed": steps_timed, "warmup": args.warmup,
            "ms_per_step": dt / steps_timed * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"Rosenbrock-{D}D DE strategy=random CR=0.9 F=0.8, "
                                   f"pop={pop_local} per GPU (BASELINE configs[1]), "
                                   "one step = best scan + std_err + stop tests + one generation",
                       "global_pop": pop, "dim": D,
                       "parallelism": f"population-sharded x{world} (island donors, "
                                      "one all-gather of the best record per generation)",
                       "turn_driver": turn_driver(drv), "rccl_ranks": rccl_ranks(drv)},
        }
    if args.full:
        # untimed, every rank (a sharded turn is collective): clocks back up after the host-side
        # pauses (status, downloads) before rank 0 times the dominant kernel
        stepper(1000)
    if args.full and rank == 0:
        # dominant kernel: de_generation_kernel, timed alone with hipEvents on its stream
        launches = max(args.steps, 20)
        kern_ms = eng.time_generation_kernel(launches) / launches
        if kern_ms > 1.03 * dt / steps_timed * 1e3 and not distributed:
            # the kernel alone slower than the step that contains it: the clocks had dropped
            # between the two measurements — bring them back up and time it once more (the
            # kernel timing leaves the engine without a population: initialise it again first)
            try:
                eng.init(x0)
                stepper(2000)
                kern_ms = min(kern_ms, eng.time_generation_kernel(launches) / launches)
            except Exception as exc:  # never lose the line to the second attempt
                print(f"bench.py: second kernel timing failed: {exc}", file=sys.stderr)
        achieved = BYTES_PER_CANDIDATE * pop_local / (kern_ms * 1e-3) / 1e9
        out["kernel_within_step"] = check_kernel_within_step(kern_ms, dt / steps_timed * 1e3, "de")
        # share of rank 0's agents that accepted at least one trial during the
        # warm-up + timed steps (selection is data dependent; the kernel does
        # the same loads, evaluation and row store either way)
        out["config"]["agents_improved_frac"] = improved
        out["config"]["accepting_regime"] = accepting
        out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                           **pmc_traffic(pop_local),
                           "kernel": "de_generation_kernel",
                           "kernel_ms": kern_ms,
                           "algorithmic_bytes_per_launch": BYTES_PER_CANDIDATE * pop_local}
    if distributed:
        dist.barrier()  # no rank tears its communicator down while another is still measuring
    eng.close()
    if args.full and rank == 0:
        if world == 1 and not args.no_north_star and pop_local == POP_PER_GPU:
            try:
                out["north_star"] = north_star_pass(args.steps)
                try:  # the same kernel where no cache can hold any useful share of the population
                    out["north_star"]["pop_2p22"] = north_star_pass(args.steps, 1 << 22)
                except Exception as exc:
                    out["north_star"]["pop_2p22"] = {"error": str(exc)[:200]}
                # the HBM-honest fraction next to the headline one: configs[1]'s 128 MiB working
                # set lives in the 256 MiB Infinity Cache, the north-star population does not
                ns = out["north_star"]["roofline"]
                out["roofline"]["frac_at_north_star_size"] = ns["frac"]
                out["roofline"]["frac_note"] = (
                    f"frac = {out['roofline']['frac']:.3f} is configs[1] (pop 65536: both population "
                    f"buffers sit in the Infinity Cache); the HBM-bound figure is pop = 2^20: "
                    f"{ns['frac']:.3f} of peak ({ns['achieved']:.0f} GB/s), see north_star")
                out["config"]["hbm_frac_at_north_star_size"] = ns["frac"]
            except Exception as exc:  # never lose the headline line to the second pass
                out["north_star"] = {"error": str(exc)[:300]}
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline()
            try:
                out["cpu_baseline_all_cores"] = cpu_baseline_all_cores()
            except Exception as exc:  # the checker library is optional here; never lose the line
                out["cpu_baseline_all_cores"] = {"error": str(exc)[:200]}
        if world == 1 and not args.no_other_configs and pop_local == POP_PER_GPU:
            out["other_configs"] = other_configs_pass()
            out["time_to_solution"] = tts_pass()
    ranks.close()
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    # Exactly one line on stdout: libraries write banners to file descriptor 1 (RCCL prints its
    # version block there when a communicator is created), so everything written to fd 1 while
    # the benchmark runs is sent to stderr and only the result line goes to the real stdout.
    sys.stdout.flush()
    _real_stdout = os.dup(1)
    os.dup2(2, 1)
    _buf = io.StringIO()
    with contextlib.redirect_stdout(_buf):
        main()
    sys.stdout.flush()
    os.dup2(_real_stdout, 1)
    _lines = [l for l in _buf.getvalue().splitlines() if l.strip()]
    for l in _lines[:-1]:
        print(l, file=sys.stderr)
    if _lines:
        os.write(1, (_lines[-1] + "\n").encode())
    if CONSISTENCY_VIOLATIONS:  # after the line: it is never lost to this check
        for v in CONSISTENCY_VIOLATIONS:
            print("bench.py: " + v, file=sys.stderr)
        sys.exit(3)
