"""Run-time objective parameters of simulated annealing on one MI355X — the measurements of
DESIGN.md §9b. One JSON line per case.

  indirection  what p(k) costs: a parametrised batch (every row the same numbers) against the same
               batch of the objective with those numbers as literals -- the path that existed
               before the engine took parameters. 4096 chains at dim 2 and 16 (16 and 8 chains per
               wave, a row per lane group) and at dim 128 (one wave per chain, a row per wave). The
               two engines alternate in one process: after a warm-up solve each, REPEATS repeats of
               time_solve (hipEvents around whole solves); reported per chain: the median repeat and
               the lowest / highest one, and the ratio of medians beside the literal engine's own
               highest / lowest.
  layout       the packed layout against one chain per wave: the same body (it reads p(0) and
               p(n_params - 1)) with the largest n_params whose group rows fit in LDS and with one
               more, which runs one chain per wave; 4096 chains at dim 8 and 16 (and at dim 64, where
               packing saves the least: 2 chains per wave). Alternating, as above.
  sweep        what the feature replaces: SWEEP values of one coefficient as ONE parametrised engine
               (a batch of SWEEP chains) against one literal engine per value. Wall clock around
               create + minimize + close. Only LITERAL_ENGINES literal engines are really built (each
               costs a run-time compilation); the figure for SWEEP engines is that total scaled, and
               is labelled so. The sweep's body is written differently from the other cases', so the
               one engine pays its compilation too.
The objective is the shifted, weighted sphere  p(1) (x_i - p(0))^2."""
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
SEED = 12374563468
MAX_ITER = 200
BODY = "double r = xi - {a}; return {b} * r * r;"
SWEEP_BODY = "double r = xi - {a}; return r * r * {b};"  # (a source of its own: no code kept from the other cases serves it)


def lit(v):
    return "(" + float(v).hex() + ")"


def objective(row=None, n_params=2, body=BODY):
    if row is None:
        return nlsolver_amd.CustomObjective(body.format(a="p(0)", b=f"p({n_params - 1})"), n_params=n_params)
    return nlsolver_amd.CustomObjective(body.format(a=lit(row[0]), b=lit(row[1])))


def make(obj, batch, dim):
    return nlsolver_amd.SANNEngine(obj, batch, dim, seed=SEED, max_iter=MAX_ITER)


def starts(batch, dim):
    """distinct starts outside the bowl, so that the chains accept trials and do not run in lock step"""
    scale = (4.0 + 3.0 * np.sqrt(dim)) * (1.0 + (np.arange(batch) % 97) / 97.0)
    return np.ascontiguousarray(scale[:, None] * np.linspace(0.8, 1.2, dim)[None, :])


def spread(ms):
    return {"median": round(statistics.median(ms), 6), "min": round(min(ms), 6), "max": round(max(ms), 6)}


def alternate(first, second, x0, batch):
    """REPEATS alternating repeats of time_solve: microseconds per chain"""
    ms = ([], [])
    for _ in range(REPEATS):
        ms[0].append(first.time_solve(x0) * 1e3 / batch)
        ms[1].append(second.time_solve(x0) * 1e3 / batch)
    return spread(ms[0]), spread(ms[1])


def same_results(ra, rb):
    return bool(np.array_equal(ra[0].view(np.uint64), rb[0].view(np.uint64)) and
                [s.f_value for s in ra[1]] == [s.f_value for s in rb[1]])


def indirection(batch, dim):
    row = (0.5, 1.5)
    x0 = starts(batch, dim)
    with make(objective(), batch, dim) as par, make(objective(row), batch, dim) as baked:
        par.set_params(np.tile(row, (batch, 1)))
        same = same_results(par.minimize(x0), baked.minimize(x0))  # (the warm-up solves)
        p, b = alternate(par, baked, x0, batch)
    print(json.dumps(dict(case="indirection", dim=dim, batch=batch, max_iter=MAX_ITER,
                          chains_per_wave=nlsolver_amd.SANNEngine.chains_per_wave(dim, 2), same_bits=same,
                          us_per_chain_params=p, us_per_chain_literals=b,
                          params_over_literals=round(p["median"] / b["median"], 4),
                          literals_spread=round(b["max"] / b["min"], 4))), flush=True)


def layout(batch, dim):
    S = nlsolver_amd.SANNEngine
    last = max(k for k in range(2, 4097) if S.chains_per_wave(dim, k) > 1)
    x0 = starts(batch, dim)

    def rows(n):
        r = np.zeros((batch, n))
        r[:, 0], r[:, n - 1] = 0.5, 1.5
        return r

    with make(objective(n_params=last), batch, dim) as packed, make(objective(n_params=last + 1), batch, dim) as solo:
        packed.set_params(rows(last))
        solo.set_params(rows(last + 1))
        same = same_results(packed.minimize(x0), solo.minimize(x0))
        g, w = alternate(packed, solo, x0, batch)
    print(json.dumps(dict(case="layout", dim=dim, batch=batch, max_iter=MAX_ITER, same_bits=same,
                          packed=dict(n_params=last, chains_per_wave=S.chains_per_wave(dim, last),
                                      lds_bytes=S.lds_bytes(dim, last), us_per_chain=g),
                          one_chain_per_wave=dict(n_params=last + 1, chains_per_wave=S.chains_per_wave(dim, last + 1),
                                                  lds_bytes=S.lds_bytes(dim, last + 1), us_per_chain=w),
                          one_per_wave_over_packed=round(w["median"] / g["median"], 4),
                          packed_spread=round(g["max"] / g["min"], 4))), flush=True)


def sweep(dim):
    rows = np.stack([np.linspace(-1.0, 1.0, SWEEP), np.full(SWEEP, 1.5)], axis=1)
    x0 = np.tile(starts(1, dim)[0], (SWEEP, 1))
    t0 = time.perf_counter()
    with make(objective(body=SWEEP_BODY), SWEEP, dim) as par:
        par.minimize(x0, params=rows)
        one_engine_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    for b in range(LITERAL_ENGINES):
        with make(objective(rows[b], body=SWEEP_BODY), 1, dim) as baked:
            baked.minimize(x0[:1])
    literal_wall = time.perf_counter() - t0
    print(json.dumps(dict(case="sweep", dim=dim, values=SWEEP, one_engine_wall_s=round(one_engine_wall, 3),
                          literal_engines_built=LITERAL_ENGINES,
                          literal_engines_built_wall_s=round(literal_wall, 3),
                          literal_engines_wall_s_scaled_to_values=round(literal_wall * SWEEP / LITERAL_ENGINES, 2))),
          flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["indirection", "layout", "sweep"]
    if "indirection" in which:
        for dim in (2, 16, 128):
            indirection(4096, dim)
    if "layout" in which:
        for dim in (8, 16, 64):
            layout(4096, dim)
    if "sweep" in which:
        sweep(2)
