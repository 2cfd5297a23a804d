"""Run-time objective parameters of the resident batch engines on one MI355X — the measurements of
DESIGN.md §3d. One JSON line per case.

  indirection  what p(k) costs: a parametrised batch (every row the same numbers) against the same
               batch of the objective with those numbers as literals -- the path that existed
               before parameters did. DE and PSO, 4096 solves of (40, D 2) and (64, D 16). The two
               engines alternate in one process: after a warm-up each, REPEATS repeats of
               time_solve (hipEvents around whole solves, init kernel and polls included); reported
               per solve: the median repeat and the lowest / highest one, and the ratio of medians.
  sweep        what the feature replaces: SWEEP values of one coefficient as ONE parametrised engine
               (a batch of SWEEP solves) against one literal engine per value. Wall clock around
               create + minimize + close. Only LITERAL_ENGINES literal engines are really built (each
               costs a run-time compilation of seconds); the figure for SWEEP engines is that total
               scaled, and is labelled so. Without create: the event time of the one batch against
               SWEEP times one literal engine's solve.
The objective is the Rosenbrock chain with its two constants as parameters."""
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
SEED0 = 12374563468
CHAIN = "double t1 = {a} - xi, t2 = xn - xi * xi; return t1 * t1 + {b} * t2 * t2;"


def lit(v):
    return "(" + float(v).hex() + ")"


def objective(row=None):
    if row is None:
        return nlsolver_amd.CustomObjective(CHAIN.format(a="p(0)", b="p(1)"), chain=True, n_params=2)
    return nlsolver_amd.CustomObjective(CHAIN.format(a=lit(row[0]), b=lit(row[1])), chain=True)


def seeds_for(n):
    return [SEED0 + 7919 * b for b in range(n)]


def make(kind, obj, batch, n, D):
    if kind == "de":
        return nlsolver_amd.DEBatchEngine(obj, batch, n, D, CR=0.9, F=0.8, eps=10e-4, max_iter=300)
    return nlsolver_amd.PSOBatchEngine(obj, batch, n, D, eps=10e-4, max_iter=300)


def inputs(kind, batch, D):
    x0 = np.tile(np.linspace(5.0, 7.0, D), (batch, 1))
    return (x0, seeds_for(batch)) if kind == "de" else (-x0, x0, seeds_for(batch))


def spread(ms):
    return {"median": round(statistics.median(ms), 6), "min": round(min(ms), 6), "max": round(max(ms), 6)}


def indirection(kind, n, D, batch=4096):
    row = (1.0, 100.0)
    args = inputs(kind, batch, D)
    with make(kind, objective(), batch, n, D) as par, make(kind, objective(row), batch, n, D) as baked:
        par.set_params(np.tile(row, (batch, 1)))
        xp, sp = par.minimize(*args)
        xb, sb = baked.minimize(*args)
        same = bool(np.array_equal(xp.view(np.uint64), xb.view(np.uint64)) and
                    [s.iteration for s in sp] == [s.iteration for s in sb])
        ms = {"params": [], "literals": []}
        for _ in range(REPEATS):  # (the two minimize calls above were the warm-up)
            ms["params"].append(par.time_solve(*args) * 1e3 / batch)
            ms["literals"].append(baked.time_solve(*args) * 1e3 / batch)
    p, b = spread(ms["params"]), spread(ms["literals"])
    print(json.dumps(dict(case="indirection", engine=kind, n=n, D=D, batch=batch, same_bits=same,
                          us_per_solve_params=p, us_per_solve_literals=b,
                          params_over_literals=round(p["median"] / b["median"], 4),
                          literals_spread=round(b["max"] / b["min"], 4),
                          mean_iterations=round(statistics.mean(s.iteration for s in sp), 1))), flush=True)


def sweep(kind, n, D):
    values = np.linspace(50.0, 150.0, SWEEP)
    rows = np.stack([np.ones(SWEEP), values], axis=1)
    args = inputs(kind, SWEEP, D)
    t0 = time.perf_counter()
    with make(kind, objective(), SWEEP, n, D) as par:
        par.minimize(*args, params=rows)
        one_engine_wall = time.perf_counter() - t0
        one_engine_event = par.time_solve(*args, repeats=REPEATS) / REPEATS
    one = inputs(kind, 1, D)
    t0 = time.perf_counter()
    for b in range(LITERAL_ENGINES):
        with make(kind, objective(rows[b]), 1, n, D) as baked:
            baked.minimize(*one)
            if b == LITERAL_ENGINES - 1:
                literal_wall = time.perf_counter() - t0
                literal_event = baked.time_solve(*one, repeats=REPEATS) / REPEATS
    print(json.dumps(dict(case="sweep", engine=kind, n=n, D=D, values=SWEEP,
                          one_engine_wall_s=round(one_engine_wall, 3),
                          literal_engines_built=LITERAL_ENGINES,
                          literal_engines_built_wall_s=round(literal_wall, 3),
                          literal_engines_wall_s_scaled_to_values=round(literal_wall * SWEEP / LITERAL_ENGINES, 2),
                          one_engine_solves_event_ms=round(one_engine_event, 4),
                          one_literal_solve_event_ms=round(literal_event, 4),
                          literal_solves_event_ms_times_values=round(literal_event * SWEEP, 3))), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["indirection", "sweep"]
    if "indirection" in which:
        for kind in ("de", "pso"):
            for n, D in ((40, 2), (64, 16)):
                indirection(kind, n, D)
    if "sweep" in which:
        for kind in ("de", "pso"):
            sweep(kind, 40, 2)
