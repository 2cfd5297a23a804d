"""What a covariance call costs on one MI355X, in iterations of the fit it belongs to — the measurements
of DESIGN.md §6e. One JSON line per case, batch 4096:

  exp3     exponential decay (CurveModel.exp_decay), n 3, m 64
  cheb64   r = y - tanh(sum_j theta_j T_j(t)) (Chebyshev basis by recurrence in the body), n 64, m 512

One process. After a warm-up of each, REPEATS repeats alternate between LMEngine.covariance(theta) and the
same engine's solve. The covariance call is read from nlsg_call_timing (host wall clock of the call's
phases): `iterate` is the evaluation launch plus lm_cov_kernel up to the synchronisation, `readback` the
copy of batch * n^2 doubles (134 MB at n = 64) and of s2 and ok to pageable host memory. The evaluation
launch alone (time_eval_kernel, hipEvents) is reported beside it, so that the covariance kernel's own
share can be read off. The yardstick is the engine's iteration — the kernels of the solve, which the
covariance code does not touch: time_solve (hipEvents around the whole solve) of a solve of exactly
ITERATIONS iterations (f_delta = 0), divided by ITERATIONS. Reported: medians, lowest and highest repeat,
and the covariance call and its kernel part in iterations."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 7
ITERATIONS = 10
EVAL_LAUNCHES = 20
BATCH = 4096
CHEBYSHEV_TANH = """const double x = t(0);
double a = 1.0, b = x, z = 0.0;
for (int j = 0; j < n; j++) { z += a * th(j); const double c = 2.0 * x * b - a; a = b; b = c; }
const double v = det_tanh(z);
r = y - v;
const double w = 1 - v * v;
a = 1.0; b = x;
for (int j = 0; j < n; j++) { J(j) = -(w * a); const double c = 2.0 * x * b - a; a = b; b = c; }"""


def spread(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def call_timing():
    from nlsolver_amd import _capi
    ms = (C.c_double * 6)()
    _capi.check(_capi.lib().nlsg_call_timing(ms))
    return dict(zip(("create", "upload", "init", "iterate", "readback", "destroy"), ms))


def measure(name, model, x0, **shape):
    import nlsolver_amd
    with nlsolver_amd.LMEngine(model, max_iter=ITERATIONS, f_delta=0.0) as eng:
        theta, st, _ = eng.minimize(x0.copy())
        assert all(s.iteration == ITERATIONS for s in st)
        cov, s2, ok = eng.covariance(theta)  # warm-up (the solve above was the other one)
        eng.time_solve(x0, 1)
        kernel, copy, solve = [], [], []
        for _ in range(REPEATS):
            eng.covariance(theta)
            t = call_timing()
            kernel.append(t["iterate"])
            copy.append(t["readback"])
            solve.append(eng.time_solve(x0, 1))
        evaluation = [eng.time_eval_kernel(theta, EVAL_LAUNCHES) / EVAL_LAUNCHES for _ in range(REPEATS)]
    k, c, s, e = spread(kernel), spread(copy), spread(solve), spread(evaluation)
    one = s["median"] / ITERATIONS
    print(json.dumps(dict(case=name, batch=BATCH, **shape, problems_ok=int(ok.sum()),
                          ms_cov_kernels=k, ms_cov_copy_back=c, ms_evaluation_launch=e,
                          ms_solve_of_10_iterations=s, ms_one_iteration=round(one, 5),
                          cov_kernels_in_iterations=round(k["median"] / one, 2),
                          cov_call_in_iterations=round((k["median"] + c["median"]) / one, 2),
                          cov_kernels_spread=round(k["max"] / k["min"], 4), cov_copy_spread=round(c["max"] / c["min"], 4),
                          solve_spread=round(s["max"] / s["min"], 4),
                          copy_back_megabytes=round(cov.nbytes / 1e6, 1))), flush=True)


def case_exp3():
    import nlsolver_amd
    m = 64
    rng = np.random.default_rng(1)
    t = np.tile(np.linspace(0.0, 4.0, m), (BATCH, 1))
    star = np.stack([rng.uniform(1.5, 2.5, BATCH), rng.uniform(0.5, 1.0, BATCH), rng.uniform(0.3, 0.7, BATCH)], axis=1)
    y = star[:, :1] * np.exp(-star[:, 1:2] * t) + star[:, 2:] + 0.01 * rng.uniform(-1.0, 1.0, t.shape)
    measure("exp3", nlsolver_amd.CurveModel.exp_decay(t, y), star * np.array([0.8, 1.2, 0.9]), n=3, m=m)


def case_cheb64():
    import nlsolver_amd
    n, m = 64, 512
    rng = np.random.default_rng(n)
    nodes = np.cos(np.pi * (2 * np.arange(m) + 1) / (2 * m))
    basis = np.empty((m, n))
    a, b = np.ones(m), nodes.copy()
    for j in range(n):
        basis[:, j] = a
        a, b = b, 2.0 * nodes * b - a
    star = rng.uniform(-1.0, 1.0, (BATCH, n)) / np.sqrt(n)
    y = np.tanh(star @ basis.T) + 0.01 * rng.uniform(-1.0, 1.0, (BATCH, m))
    x0 = 0.5 * star + 0.1 * rng.uniform(-1.0, 1.0, (BATCH, n)) / np.sqrt(n)
    measure("cheb64", nlsolver_amd.CurveModel(np.tile(nodes, (BATCH, 1)), y, CHEBYSHEV_TANH, n), x0, n=n, m=m)


if __name__ == "__main__":
    case_exp3()
    case_cheb64()
