"""Resident batch PSO (nlsg_pso_batch_*) against the turn engine (nlsg_pso_*) on one MI355X — the
cases of DESIGN.md §4c. One JSON line per case. The two drivers run alternating in the same
process: after one warm-up call each, WINDOWS windows per driver, every window at least 0.2 s of
wall clock around calls that end in a synchronise; reported per call: the median window and the
lowest / highest one. `event_ms` is PSOBatchEngine.time_solve (hipEvents, init kernel and polls
included); `phases_ms` is nlsg_call_timing's create / init / iterate / read-back split of the last
call. `requirement_met`: the resident path's median window is below the turn engine's lowest one.
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/pso_resident_time.py`
(a run of its own)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlsolver_amd  # noqa: E402
from nlsolver_amd import _capi  # noqa: E402

WINDOWS = 5
SEED0 = 12374563468
TYPES = {"accelerated": nlsolver_amd.PSO_ACCELERATED, "vanilla": nlsolver_amd.PSO_VANILLA}


def seeds_for(n):
    return [SEED0 + 7919 * b for b in range(n)]


def phases():
    t = (C.c_double * 6)()
    _capi.check(_capi.lib().nlsg_call_timing(t))
    return {k: round(v, 4) for k, v in zip(("create", "upload", "init", "iterate", "readback", "destroy"), t)}


def window(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def reps_for(fn):
    """calls per window so that a window lasts at least 0.2 s (after one warm-up call)"""
    fn()
    reps = 1
    while True:
        ms = window(fn, reps)
        if ms * reps >= 200.0:
            return reps
        reps = max(reps * 2, int(reps * 220.0 / max(ms * reps, 1e-3)) + 1)


def alternate(resident, turns):
    """{driver: per-call ms of each window} with the drivers' windows alternating"""
    fns = {"resident": resident, "turns": turns}
    reps = {k: reps_for(f) for k, f in fns.items()}
    out = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, f in fns.items():
            out[k].append(window(f, reps[k]))
    return out, reps


def summary(ms, scale=1.0):
    return {"median_ms": round(statistics.median(ms) * scale, 4), "min_ms": round(min(ms) * scale, 4),
            "max_ms": round(max(ms) * scale, 4)}


def report(case, win, reps, scale_turns=1.0, **extra):
    r, t = summary(win["resident"]), summary(win["turns"], scale_turns)
    ratios = [tt * scale_turns / rr for rr, tt in zip(win["resident"], win["turns"])]
    print(json.dumps(dict(case=case, resident=r, turns=t, calls_per_window=reps,
                          requirement_met=bool(r["median_ms"] < t["min_ms"]),
                          turns_over_resident={"median": round(statistics.median(ratios), 3),
                                               "min": round(min(ratios), 3), "max": round(max(ratios), 3)},
                          **extra)), flush=True)


def case_a():
    for name, type_ in TYPES.items():
        # (a1) the drop-in class with its defaults, construction to status
        def drop_in(driver):
            def run():
                x = np.array([5.0, 7.0])
                return nlsolver_amd.PSO("rosenbrock", None, type=type_, driver=driver).minimize(x)
            return run
        win, reps = alternate(drop_in("resident"), drop_in("turns"))
        st = drop_in("resident")()
        split = phases()
        drop_in("turns")()
        report(f"a_one_default_solve_drop_in_{name}", win, reps, iters=int(st.iteration),
               phases_ms_resident=split, phases_ms_turns=phases())
        # (a2) kept engines
        lo, hi = np.array([[-5.0, -7.0]]), np.array([[5.0, 7.0]])
        with nlsolver_amd.PSOBatchEngine("rosenbrock", 1, 10, 2, type=type_) as be, \
                nlsolver_amd.PSOEngine("rosenbrock", 10, 2, type=type_, seed=SEED0) as te:
            def turns():
                te.minimize(np.zeros(2), lo[0], hi[0])
            win, reps = alternate(lambda: be.minimize(lo, hi, [SEED0]), turns)
            ev = be.time_solve(lo, hi, [SEED0], 50) / 50
            be.minimize(lo, hi, [SEED0])
            split = phases()
            turns()
            report(f"a_one_default_solve_kept_engine_{name}", win, reps, event_ms_resident=round(ev, 4),
                   phases_ms_resident=split, phases_ms_turns=phases())


def case_b():
    B, part = 4096, 64
    lo, hi = np.tile([-5.0, -7.0], (B, 1)), np.tile([5.0, 7.0], (B, 1))
    seeds = seeds_for(B)
    for name, type_ in TYPES.items():
        with nlsolver_amd.PSOBatchEngine("rosenbrock", B, 10, 2, type=type_) as be, \
                nlsolver_amd.PSOEngine("rosenbrock", 10, 2, type=type_, seed=SEED0) as te:
            def turns():  # 64 solves through the one reused engine (its seed is fixed: the same solve)
                for _ in range(part):
                    te.minimize(np.zeros(2), lo[0], hi[0])
            win, reps = alternate(lambda: be.minimize(lo, hi, seeds), turns)
            ev = be.time_solve(lo, hi, seeds, 5) / 5
            # the work differs: the reused engine repeats its one seed, the batch runs 4096 seeds
            _, sts = be.minimize(lo, hi, seeds)
            its = [int(s.iteration) for s in sts]
            report(f"b_4096_default_solves_{name}", win, reps, scale_turns=B / part,
                   event_ms_resident=round(ev, 4),
                   turns_turn_engine=int(te.minimize(np.zeros(2), lo[0], hi[0]).iteration),
                   turns_resident={"mean": round(statistics.mean(its), 2), "min": min(its), "max": max(its)},
                   note=f"turns: {part} solves of seed {SEED0} through one reused PSOEngine timed, scaled "
                        f"by {B // part}; resident: {B} different seeds")


def case_c():
    B, part, D = 256, 8, 128
    seeds = seeds_for(B)
    for name, n in (("vanilla", 40), ("accelerated", 120)):
        type_ = TYPES[name]
        kw = dict(type=type_, eps=0.0, max_iter=200, best_val_no_change=10 ** 6)
        with nlsolver_amd.PSOBatchEngine("rosenbrock", B, n, D, **kw) as be, \
                nlsolver_amd.PSOEngine("rosenbrock", n, D, seed=SEED0, **kw) as te:
            def turns():
                for _ in range(part):
                    te.minimize(np.zeros(D), -2.048, 2.048)
            win, reps = alternate(lambda: be.minimize(-2.048, 2.048, seeds), turns)
            ev = be.time_solve(-2.048, 2.048, seeds, 3) / 3
            _, sts = be.minimize(-2.048, 2.048, seeds)
            report(f"c_256_solves_{name}_{n}x{D}_200_turns", win, reps, scale_turns=B / part,
                   event_ms_resident=round(ev, 4), iters=int(sts[0].iteration),
                   note=f"turns: {part} PSOEngine solves timed, scaled by {B // part}; reported, not required")


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b", "c"]
    for w in which:
        {"a": case_a, "b": case_b, "c": case_c}[w]()
