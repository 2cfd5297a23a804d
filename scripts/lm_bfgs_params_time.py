"""Run-time objective parameters of Levenberg-Marquardt and BFGS on one MI355X — the measurements of
DESIGN.md §5 / §6 ("run-time parameters"). One JSON line per case.

  indirection  what p(k) costs: a parametrised batch (every row the same numbers) against the same
               batch of the objective with those numbers as literals -- the path that existed
               before these engines took parameters. 4096 problems; LM at n = 2, 16 and 130 (tree
               order; LM_ITERS iterations, fewer at n = 130 where an evaluation is 16 n^2 probes),
               BFGS at dim = 2, 16 and 130 (tree order) and at dim 16 with 4096 parameters, where
               128 KiB of rows leave one block per CU. The two engines alternate in one process:
               after a warm-up solve each, REPEATS repeats (LM: time_solve, hipEvents around whole
               solves; BFGS: init, then time_steps over BFGS_ITERS iterations, hipEvents around the
               iterations); reported per solve: the median repeat and the lowest / highest one, and
               the ratio of medians beside the literal engine's own highest / lowest.
  sweep        what the feature replaces: SWEEP values of one coefficient as ONE parametrised engine
               (a batch of SWEEP problems) against one literal engine per value. Wall clock around
               create + minimize + close. Only LITERAL_ENGINES literal engines are really built (each
               costs a run-time compilation); the figure for SWEEP engines is that total scaled, and
               is labelled so.
The objective is the Rosenbrock chain with its two constants as parameters (with 4096 parameters:
the first and the last of the row)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlsolver_amd  # noqa: E402

REPEATS = 7
SWEEP = 64
LITERAL_ENGINES = 6
BATCH = 4096
LM_ITERS = {2: 8, 16: 8, 130: 2}
BFGS_ITERS = 12
CHAIN = "double t1 = {a} - xi, t2 = xn - xi * xi; return t1 * t1 + {b} * t2 * t2;"


def lit(v):
    return "(" + float(v).hex() + ")"


def objective(row=None, n_params=2):
    if row is None:
        return nlsolver_amd.CustomObjective(CHAIN.format(a="p(0)", b=f"p({n_params - 1})"), chain=True,
                                            n_params=n_params)
    return nlsolver_amd.CustomObjective(CHAIN.format(a=lit(row[0]), b=lit(row[-1])), chain=True)


def make(kind, obj, batch, n):
    if kind == "lm":
        return nlsolver_amd.LMEngine(obj, batch=batch, n=n, max_iter=LM_ITERS.get(n, 8))
    return nlsolver_amd.BFGSEngine(obj, batch, dim=n, max_iter=BFGS_ITERS)


def starts(batch, n):
    """distinct starts, so that the problems do not run in lock step"""
    scale = 0.5 + 1.5 * (np.arange(batch) % 97) / 97.0
    return np.ascontiguousarray(scale[:, None] * np.linspace(0.8, 1.2, n)[None, :])


def spread(ms):
    return {"median": round(statistics.median(ms), 6), "min": round(min(ms), 6), "max": round(max(ms), 6)}


def timed(kind, eng, x0):
    """ms of one batch solve on the device"""
    if kind == "lm":
        return eng.time_solve(x0)
    eng.init(x0)
    return eng.time_steps(BFGS_ITERS)[0]


def indirection(kind, n, n_params=2, batch=BATCH):
    row = np.zeros(n_params)
    row[0], row[-1] = 1.0, 100.0
    x0 = starts(batch, n)
    with make(kind, objective(None, n_params), batch, n) as par, make(kind, objective(row), batch, n) as baked:
        par.set_params(np.tile(row, (batch, 1)))
        rp, rb = par.minimize(x0.copy()), baked.minimize(x0.copy())  # (the warm-up solves)
        same = bool(np.array_equal(rp[0].view(np.uint64), rb[0].view(np.uint64)) and
                    [s.iteration for s in rp[1]] == [s.iteration for s in rb[1]])
        ms = {"params": [], "literals": []}
        for _ in range(REPEATS):
            ms["params"].append(timed(kind, par, x0) * 1e3 / batch)
            ms["literals"].append(timed(kind, baked, x0) * 1e3 / batch)
    p, b = spread(ms["params"]), spread(ms["literals"])
    print(json.dumps(dict(case="indirection", engine=kind, n=n, batch=batch, n_params=n_params,
                          same_bits=same, us_per_solve_params=p, us_per_solve_literals=b,
                          params_over_literals=round(p["median"] / b["median"], 4),
                          literals_spread=round(b["max"] / b["min"], 4),
                          mean_iterations=round(statistics.mean(s.iteration for s in rp[1]), 1))), flush=True)


def sweep(kind, n):
    values = np.linspace(50.0, 150.0, SWEEP)
    rows = np.stack([np.ones(SWEEP), values], axis=1)
    x0 = np.tile(np.linspace(0.8, 1.2, n), (SWEEP, 1))
    t0 = time.perf_counter()
    with make(kind, objective(), SWEEP, n) as par:
        par.minimize(x0.copy(), params=rows)
        one_engine_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b in range(LITERAL_ENGINES):
        with make(kind, objective(rows[b]), 1, n) as baked:
            baked.minimize(x0[:1].copy())
    literal_wall = time.perf_counter() - t0
    print(json.dumps(dict(case="sweep", engine=kind, n=n, values=SWEEP,
                          one_engine_wall_s=round(one_engine_wall, 3),
                          literal_engines_built=LITERAL_ENGINES,
                          literal_engines_built_wall_s=round(literal_wall, 3),
                          literal_engines_wall_s_scaled_to_values=round(literal_wall * SWEEP / LITERAL_ENGINES, 2))),
          flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["indirection", "sweep"]
    if "indirection" in which:
        for n in (2, 16, 130):
            indirection("lm", n)
        for n in (2, 16, 130):
            indirection("bfgs", n)
        indirection("bfgs", 16, n_params=4096)
    if "sweep" in which:
        sweep("lm", 2)
        sweep("bfgs", 2)
