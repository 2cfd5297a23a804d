"""BFGS: the resident whole-solve kernel (NLSG_BFGS_RESIDENT, driver="resident") against the lock-step engine
on one MI355X — the measurement of DESIGN.md §5d. One JSON line per case.

The two drivers alternate in one process. After one warm-up solve each, WINDOWS windows per driver; a window
is REPS whole solves (init to every problem's own stop, minimize()), wall clock around calls that end in a
synchronise. Reported per solve in ms: the median window with the lowest and highest one, and the ratio lock
step / resident window by window (window k of one driver against window k of the other, taken back to back).
Every case asserts that the two drivers returned the same x and status, bit for bit.

  (a) one start     Rosenbrock 2-D from the start of tests/golden/bfgs_fd.json's rosenbrock_n2 with default
                    arguments through BFGS(...): construction to status, engine built per call, as the drop-in
                    does; with nlsg_call_timing's create / init / iterate / read-back / destroy split of the
                    last call
  (b) 4096 starts   Rosenbrock n = 16, default gradient, reference order, each problem to its own stop; the
                    spread of the iteration counts is printed beside the times: it is what the lock-step
                    tail costs
  (c) 4096 starts   the quadratic at n = 64 with its analytic gradient, both orders
  (d) 64 starts     of (b): the small-batch regime
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nlsolver_amd  # noqa: E402
from nlsolver_amd import _capi  # noqa: E402

WINDOWS = 7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def status(st):
    return [(int(bits(s.f_value)[0]), s.iteration, s.function_calls_used, s.gradient_evals_used) for s in st]


def phases():
    t = (C.c_double * 6)()
    _capi.check(_capi.lib().nlsg_call_timing(t))
    return {k: round(v, 4) for k, v in zip(("create", "upload", "init", "iterate", "readback", "destroy"), t)}


def spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def windows(run_lock, run_res, reps):
    """alternating windows; ms per call of either driver and the ratio window by window"""
    lock, res = [], []
    for _ in range(WINDOWS):
        for fn, out in ((run_lock, lock), (run_res, res)):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            out.append((time.perf_counter() - t0) * 1e3 / reps)
    ratios = [a / b for a, b in zip(lock, res)]
    return dict(ms_lock_step=spread(lock), ms_resident=spread(res), lock_over_resident=spread(ratios),
                lock_over_resident_windows=[round(r, 3) for r in ratios], windows=WINDOWS, solves_per_window=reps)


def rosen_starts(batch, n):
    """distinct starts: the problems stop at different iterations"""
    scale = 0.5 + 1.5 * (np.arange(batch) % 97) / 97.0
    shift = 0.05 * ((np.arange(batch) * 7) % 13)
    return np.ascontiguousarray(scale[:, None] * np.linspace(0.8, 1.2, n)[None, :] - shift[:, None])


def quad_starts(batch, n):
    scale = 10.0 ** (-2 + 4 * (np.arange(batch) % 101) / 100.0)
    sign = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    return np.ascontiguousarray(scale[:, None] * (1.0 + 0.01 * (np.arange(n) % 11))[None, :] * sign[None, :])


def case_one_start():
    with open(os.path.join(ROOT, "tests", "golden", "bfgs_fd.json")) as fh:
        g = json.load(fh)["rosenbrock_n2"]
    hx = float.fromhex
    x0 = hx(g["x0"]) + hx(g["x0_step"]) * np.arange(g["n"], dtype=np.float64)
    out = {}

    def run(driver):
        def f():
            x = x0.copy()
            solver = nlsolver_amd.BFGS("rosenbrock", driver=driver)
            st = solver.minimize(x)
            out[driver] = (x, status([st]), solver.driver_used, phases())
        return f

    run("turns")(), run("resident")()  # (the warm-up calls)
    r = windows(run("turns"), run("resident"), reps=20)
    assert out["resident"][2] == "resident" and out["turns"][2] == "turns"
    assert np.array_equal(bits(out["turns"][0]), bits(out["resident"][0])) and out["turns"][1] == out["resident"][1]
    print(json.dumps(dict(case="a_one_start_rosenbrock_2d_construct_to_status", iterations=out["turns"][1][0][1],
                          phases_ms_lock_step=out["turns"][3], phases_ms_resident=out["resident"][3], **r)),
          flush=True)


def case_batch(tag, objective, x0, reps, **kw):
    with nlsolver_amd.BFGSEngine(objective, x0.shape[0], **kw) as lock, \
            nlsolver_amd.BFGSEngine(objective, x0.shape[0], resident=True, **kw) as res:
        got = {}

        def run(eng, key):
            def f():
                got[key] = eng.minimize(x0.copy())
            return f

        run(lock, "lock")(), run(res, "res")()  # (the warm-up solves)
        r = windows(run(lock, "lock"), run(res, "res"), reps)
        (xl, sl), (xr, sr) = got["lock"], got["res"]
        assert np.array_equal(bits(xl), bits(xr)) and status(sl) == status(sr)
        iters = np.array([s.iteration for s in sl])
        print(json.dumps(dict(case=tag, batch=int(x0.shape[0]), dim=int(x0.shape[1]),
                              order="reference" if kw.get("reference_order") else "tree",
                              iterations=dict(min=int(iters.min()), median=float(np.median(iters)),
                                              mean=round(float(iters.mean()), 2), max=int(iters.max()),
                                              sum_over_batch=int(iters.sum())),
                              lock_step_turns=int(iters.max()) + 1, **r)), flush=True)


if __name__ == "__main__":
    case_one_start()
    case_batch("b_4096_starts_rosenbrock_16_default_gradient", "rosenbrock", rosen_starts(4096, 16), 3, dim=16,
               reference_order=True)
    # the G6 quadratic: d_i = 1 + 9 i / (n - 1), b_i = sin(0.1 i), c = 0.01
    d, b, c = 1.0 + 9.0 * np.arange(64) / 63.0, np.sin(0.1 * np.arange(64)), 0.01
    for ref in (True, False):
        case_batch("c_4096_starts_quadratic_64_analytic_gradient", nlsolver_amd.QuadDiagRank1(d, b, c),
                   quad_starts(4096, 64), 3, reference_order=ref)
    case_batch("d_64_starts_rosenbrock_16_default_gradient", "rosenbrock", rosen_starts(64, 16), 10, dim=16,
               reference_order=True)
