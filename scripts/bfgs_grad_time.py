"""BFGS on a compiled objective: its analytic gradient body against the default finite-difference gradient,
on one MI355X — the measurement of DESIGN.md §5c. One JSON line per case.

The Rosenbrock chain as a CustomObjective with grad_body; two engines of it built in the same process,
gradient=None (the body: nlsg_bfgs_create_gradient) and gradient="finite_difference" (4 n probes per
gradient; in reference order a probe per lane). Cases: dim 128 x batch 4096 in both summation orders, dim
1024 x batch 256 in tree order. After one warm-up run each, REPEATS repeats with the two engines
alternating: init, then time_steps over ITERS iterations (hipEvents around the iterations; the share of
the two H passes is reported by the engine, the rest is the search kernel, where the gradient lives).
Reported: ms per iteration of the whole batch, median and lowest / highest repeat, for the iteration and
for its search part; the ratio of medians beside the finite-difference engine's own highest / lowest;
gradient evaluations per iteration and problem of either engine (the work the two did is the same kind,
not the same trajectory)."""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nlsolver_amd  # noqa: E402

REPEATS = 7
ITERS = 10
TERM = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;"
GRAD = ("double g = 0.0; if (i + 1 < D) g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi); "
        "if (i > 0) g = g + 200.0 * (xi - xm * xm); return g;")


def starts(batch, n):
    """distinct starts, so that the problems do not run in lock step"""
    scale = 0.5 + 1.5 * (np.arange(batch) % 97) / 97.0
    return np.ascontiguousarray(scale[:, None] * np.linspace(0.8, 1.2, n)[None, :])


def spread(ms):
    return {"median": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5)}


def run(eng, x0):
    """(ms per iteration, ms per iteration outside the H passes, gradients per iteration and problem)"""
    eng.init(x0)
    total, hess = eng.time_steps(ITERS)
    _, st = eng.download()
    grads = statistics.mean((s.gradient_evals_used - 1) / max(s.iteration, 1) for s in st)
    return total / ITERS, (total - hess) / ITERS, grads


def case(n, batch, reference_order):
    obj = nlsolver_amd.CustomObjective(TERM, chain=True, grad_body=GRAD)
    x0 = starts(batch, n)
    kw = dict(dim=n, max_iter=ITERS, reference_order=reference_order)
    with nlsolver_amd.BFGSEngine(obj, batch, **kw) as ana, \
            nlsolver_amd.BFGSEngine(obj, batch, gradient="finite_difference", **kw) as fd:
        assert (ana.gradient_used, fd.gradient_used) == ("analytic", "finite_difference")
        run(ana, x0), run(fd, x0)  # (the warm-up runs)
        ms = {"analytic": [], "fd": [], "analytic_search": [], "fd_search": []}
        for _ in range(REPEATS):
            ta, sa, ga = run(ana, x0)
            tf, sf, gf = run(fd, x0)
            ms["analytic"].append(ta), ms["analytic_search"].append(sa)
            ms["fd"].append(tf), ms["fd_search"].append(sf)
    a, f = spread(ms["analytic"]), spread(ms["fd"])
    a_s, f_s = spread(ms["analytic_search"]), spread(ms["fd_search"])
    print(json.dumps(dict(case="gradient", dim=n, batch=batch, order="reference" if reference_order else "tree",
                          iterations=ITERS, ms_per_iteration_analytic=a, ms_per_iteration_fd=f,
                          ms_search_analytic=a_s, ms_search_fd=f_s,
                          fd_over_analytic=round(f["median"] / a["median"], 3),
                          fd_over_analytic_search=round(f_s["median"] / a_s["median"], 3),
                          fd_spread=round(f["max"] / f["min"], 4), analytic_spread=round(a["max"] / a["min"], 4),
                          gradients_per_iteration_analytic=round(ga, 2), gradients_per_iteration_fd=round(gf, 2))),
          flush=True)


if __name__ == "__main__":
    case(128, 4096, False)
    case(128, 4096, True)
    case(1024, 256, False)
