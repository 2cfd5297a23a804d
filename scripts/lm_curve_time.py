"""Levenberg-Marquardt curve models on one MI355X — the measurements of DESIGN.md §6d. One JSON line per case.

  fd        exponential decay, m 64, batch 4096, to convergence: the curve engine (CurveModel.exp_decay)
            against the only other route for the same fits, LMEngine(CustomObjective(..., n_params=128)) with
            (t, y) in p(k) and the default finite-difference functors (1 + 4 n + 16 n^2 probes of the objective
            per evaluation, each a pass over the data). The finite-difference engine runs no code the curve
            model touched: it is the baseline as it was before curve models existed. Start: the optimum times
            (0.8, 1.2, 0.9). The finite-difference Hessian is the whole Hessian, not 2 J^T J, and need not be
            positive definite away from the optimum: the problems that end in NaN are counted.
  fd_near   the same from the optimum times (0.98, 1.02, 0.99)
  price16   r = y - tanh(sum_j theta_j T_j(t)) (Chebyshev basis by recurrence in the body) as a curve model
  price64   against TanhRegression on the same basis as a design matrix, n 16 and 64, m 512, batch 8192:
            the evaluation kernel alone (time_eval_kernel) and whole solves. The curve model recomputes its
            basis every evaluation, the regression streams A.

After one warm-up each, REPEATS repeats with the two engines alternating, a repeat being SOLVES solves or
EVAL_LAUNCHES evaluation launches between hipEvents; reported: ms per solve (and per evaluation launch)
of the whole batch, median and lowest / highest repeat, the ratio of medians beside each engine's own
highest / lowest.

Without --case every case runs in a child process of its own under its own time limit, and nothing more is
started after one that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7
EVAL_LAUNCHES = 20
SOLVES = 10  # per repeat
LIMITS = {"fd": 240, "fd_near": 240, "price16": 240, "price64": 420}  # seconds
CHEBYSHEV_TANH = """const double x = t(0);
double a = 1.0, b = x, z = 0.0;
for (int j = 0; j < n; j++) { z += a * th(j); const double c = 2.0 * x * b - a; a = b; b = c; }
const double v = det_tanh(z);
r = y - v;
const double w = 1 - v * v;
a = 1.0; b = x;
for (int j = 0; j < n; j++) { J(j) = -(w * a); const double c = 2.0 * x * b - a; a = b; b = c; }"""
EXP_DECAY_OBJECTIVE = ("double s = 0.0; for (int i = 0; i < 64; i++) {"
                       " const double r = p(64 + i) - (x(0) * det_exp(-x(1) * p(i)) + x(2)); s += r * r; } return s;")


def spread(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def alternate(a, b):
    """REPEATS alternating calls of the two timers after a warm-up each: two lists of ms"""
    a(), b()
    ta, tb = [], []
    for _ in range(REPEATS):
        ta.append(a())
        tb.append(b())
    return ta, tb


def iterations(st):
    its = [s.iteration for s in st]
    return {"mean": round(statistics.mean(its), 2), "max": max(its)}


def case_fd(name, scale):
    import nlsolver_amd
    m, batch = 64, 4096
    rng = np.random.default_rng(1)
    t = np.tile(np.linspace(0.0, 4.0, m), (batch, 1))
    star = np.stack([rng.uniform(1.5, 2.5, batch), rng.uniform(0.5, 1.0, batch), rng.uniform(0.3, 0.7, batch)], axis=1)
    y = star[:, :1] * np.exp(-star[:, 1:2] * t) + star[:, 2:] + 0.01 * rng.uniform(-1.0, 1.0, t.shape)
    x0 = star * np.array(scale)
    rows = np.ascontiguousarray(np.concatenate([t, y], axis=1))
    obj = nlsolver_amd.CustomObjective(EXP_DECAY_OBJECTIVE, vector=True, n_params=2 * m)
    with nlsolver_amd.LMEngine(nlsolver_amd.CurveModel.exp_decay(t, y)) as curve, \
            nlsolver_amd.LMEngine(obj, batch=batch, n=3) as fd:
        fd.set_params(rows)
        xc, sc, _ = curve.minimize(x0.copy())
        xf, sf, _ = fd.minimize(x0.copy())
        tc, tf = alternate(lambda: curve.time_solve(x0, SOLVES) / SOLVES, lambda: fd.time_solve(x0, SOLVES) / SOLVES)
    c, f = spread(tc), spread(tf)
    ok = np.array([np.isfinite(s.f_value) for s in sf]) & np.all(np.isfinite(xf), axis=1)
    print(json.dumps(dict(case=name, model="exp_decay", start_over_optimum=list(scale), m=m, batch=batch,
                          ms_solve_curve=c, ms_solve_fd=f,
                          fd_over_curve=round(f["median"] / c["median"], 2),
                          curve_spread=round(c["max"] / c["min"], 4), fd_spread=round(f["max"] / f["min"], 4),
                          iterations_curve=iterations(sc), iterations_fd=iterations(sf),
                          fd_problems_ending_not_finite=int(np.sum(~ok)),
                          curve_problems_ending_not_finite=int(np.sum(~np.isfinite([s.f_value for s in sc]))),
                          max_abs_theta_difference_where_fd_is_finite=float(np.max(np.abs(xc - xf)[ok])),
                          median_f_curve=float(np.median([s.f_value for s in sc])),
                          median_f_fd_where_finite=float(np.median(np.array([s.f_value for s in sf])[ok])))),
          flush=True)


def case_price(n):
    import nlsolver_amd
    m, batch = 512, 8192
    rng = np.random.default_rng(n)
    nodes = np.cos(np.pi * (2 * np.arange(m) + 1) / (2 * m))
    basis = np.empty((m, n))
    a, b = np.ones(m), nodes.copy()
    for j in range(n):
        basis[:, j] = a
        a, b = b, 2.0 * nodes * b - a
    star = rng.uniform(-1.0, 1.0, (batch, n)) / np.sqrt(n)
    y = np.tanh(star @ basis.T) + 0.01 * rng.uniform(-1.0, 1.0, (batch, m))
    x0 = 0.5 * star + 0.1 * rng.uniform(-1.0, 1.0, (batch, n)) / np.sqrt(n)
    t = np.tile(nodes, (batch, 1))
    A = np.ascontiguousarray(np.broadcast_to(basis, (batch, m, n)))
    with nlsolver_amd.LMEngine(nlsolver_amd.CurveModel(t, y, CHEBYSHEV_TANH, n)) as curve, \
            nlsolver_amd.LMEngine(nlsolver_amd.TanhRegression(A, y)) as tanh:
        del A
        xc, sc, _ = curve.minimize(x0.copy())
        xt, st, _ = tanh.minimize(x0.copy())
        ec, et = alternate(lambda: curve.time_eval_kernel(x0, EVAL_LAUNCHES) / EVAL_LAUNCHES,
                           lambda: tanh.time_eval_kernel(x0, EVAL_LAUNCHES) / EVAL_LAUNCHES)
        tc, tt = alternate(lambda: curve.time_solve(x0, SOLVES) / SOLVES,
                           lambda: tanh.time_solve(x0, SOLVES) / SOLVES)
    e_c, e_t, s_c, s_t = spread(ec), spread(et), spread(tc), spread(tt)
    print(json.dumps(dict(case="price", n=n, m=m, batch=batch, ms_eval_curve=e_c, ms_eval_tanh=e_t,
                          eval_curve_over_tanh=round(e_c["median"] / e_t["median"], 3),
                          eval_curve_spread=round(e_c["max"] / e_c["min"], 4),
                          eval_tanh_spread=round(e_t["max"] / e_t["min"], 4),
                          ms_solve_curve=s_c, ms_solve_tanh=s_t,
                          solve_curve_over_tanh=round(s_c["median"] / s_t["median"], 3),
                          solve_curve_spread=round(s_c["max"] / s_c["min"], 4),
                          solve_tanh_spread=round(s_t["max"] / s_t["min"], 4),
                          iterations_curve=iterations(sc), iterations_tanh=iterations(st),
                          max_abs_theta_difference=float(np.max(np.abs(xc - xt))))), flush=True)


CASES = {"fd": lambda: case_fd("fd", (0.8, 1.2, 0.9)), "fd_near": lambda: case_fd("fd_near", (0.98, 1.02, 0.99)),
         "price16": lambda: case_price(16), "price64": lambda: case_price(64)}

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        CASES[args.case]()
        sys.exit(0)
    for name in ("fd", "fd_near", "price16", "price64"):
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name],
                                timeout=LIMITS[name]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(json.dumps(dict(case=name, failed=rc)), flush=True)
            sys.exit(rc if rc > 0 else 1)
