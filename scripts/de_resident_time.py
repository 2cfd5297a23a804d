"""Resident batch DE (nlsg_de_batch_*) against the turn engine (nlsg_de_*) on one MI355X — the
cases of DESIGN.md §3c. One JSON line per case. The two drivers run alternating in the same
process: after one warm-up call each, WINDOWS windows per driver, every window at least 0.2 s of
wall clock around calls that end in a synchronise; reported per call: the median window and the
lowest / highest one. `event_ms` is DEBatchEngine.time_solve (hipEvents, init kernel and polls
included); `phases_ms` is nlsg_call_timing's create / init / iterate / read-back split of the last
call. Kernel times: run under `rocprofv3 --kernel-trace --stats -- python
scripts/de_resident_time.py` (a run of its own)."""
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
                          turns_over_resident={"median": round(statistics.median(ratios), 3),
                                               "min": round(min(ratios), 3), "max": round(max(ratios), 3)},
                          **extra)), flush=True)


C1 = dict(CR=0.9, F=0.8, eps=10e-4)


def case_a():
    # (a1) the drop-in class, construction to status
    def drop_in(driver):
        def run():
            x = np.array([5.0, 7.0])
            return nlsolver_amd.DE("rosenbrock", None, 0.9, 0.8, 10e-4, 40, driver=driver).minimize(x)
        return run
    win, reps = alternate(drop_in("resident"), drop_in("turns"))
    st = drop_in("resident")()
    split = phases()
    drop_in("turns")()
    report("a_one_c1_solve_drop_in", win, reps, iters=int(st.iteration), phases_ms_resident=split,
           phases_ms_turns=phases())
    # (a2) kept engines
    x0 = np.array([[5.0, 7.0]])
    with nlsolver_amd.DEBatchEngine("rosenbrock", 1, 40, 2, **C1) as be, \
            nlsolver_amd.DEEngine("rosenbrock", 40, 2, seed=SEED0, **C1) as te:
        def turns():
            x = np.array([5.0, 7.0])
            te.minimize(x)
        win, reps = alternate(lambda: be.minimize(x0, [SEED0]), turns)
        ev = be.time_solve(x0, [SEED0], 50) / 50
        be.minimize(x0, [SEED0])
        report("a_one_c1_solve_kept_engine", win, reps, event_ms_resident=round(ev, 4),
               phases_ms_resident=phases())


def case_b():
    B, part = 4096, 64
    x0 = np.tile([5.0, 7.0], (B, 1))
    seeds = seeds_for(B)
    with nlsolver_amd.DEBatchEngine("rosenbrock", B, 40, 2, **C1) as be, \
            nlsolver_amd.DEEngine("rosenbrock", 40, 2, seed=SEED0, **C1) as te:
        def turns():  # 64 solves through the one reused engine (its seed is fixed: the same solve)
            for _ in range(part):
                x = np.array([5.0, 7.0])
                te.minimize(x)
        win, reps = alternate(lambda: be.minimize(x0, seeds), turns)
        ev = be.time_solve(x0, seeds, 5) / 5
        # the work differs slightly: the reused engine repeats its one seed, the batch runs 4096 seeds
        _, sts = be.minimize(x0, seeds)
        gens = [int(s.iteration) for s in sts]
        x = np.array([5.0, 7.0])
        report("b_4096_c1_solves", win, reps, scale_turns=B / part, event_ms_resident=round(ev, 4),
               generations_turns=int(te.minimize(x).iteration),
               generations_resident={"mean": round(statistics.mean(gens), 2), "min": min(gens), "max": max(gens)},
               note=f"turns: {part} solves of seed {SEED0} through one reused DEEngine timed, scaled by "
                    f"{B // part}; resident: {B} different seeds")


def case_c():
    B, part, pop, D = 256, 8, 70, 128
    kw = dict(CR=0.9, F=0.8, eps=0.0, max_iter=200, best_val_no_change=10 ** 6)
    x0 = np.full((B, D), 4.096)
    seeds = seeds_for(B)
    with nlsolver_amd.DEBatchEngine("rosenbrock", B, pop, D, **kw) as be, \
            nlsolver_amd.DEEngine("rosenbrock", pop, D, seed=SEED0, **kw) as te:
        def turns():
            for _ in range(part):
                x = np.full(D, 4.096)
                te.minimize(x)
        win, reps = alternate(lambda: be.minimize(x0, seeds), turns)
        ev = be.time_solve(x0, seeds, 3) / 3
        _, sts = be.minimize(x0, seeds)
        report("c_256_solves_pop70_D128_200gen", win, reps, scale_turns=B / part,
               event_ms_resident=round(ev, 4), iters=int(sts[0].iteration),
               note=f"turns: {part} DEEngine solves timed, scaled by {B // part}")


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b", "c"]
    for w in which:
        {"a": case_a, "b": case_b, "c": case_c}[w]()
