"""Levenberg-Marquardt: the resident whole-solve kernel (NLSG_LM_RESIDENT) against the lock-step driver on one
MI355X — the measurement of DESIGN.md §6g. One JSON line per case.

ONE engine per case, switched between the drivers with set_solver; the data stay on the device. After one
warm-up solve per driver (which also compiles a TanhRegression engine's resident kernel), WINDOWS windows per
driver, alternating; a window is nlsg_lm_time_solve with REPS repeats: device events around every whole solve
(start point re-uploaded outside the interval), so the host's launches and its polls of the unfinished count
are inside, the transfers of theta are not. Reported per solve in ms: the median window with the lowest and
highest one, and the ratio lock step / resident window by window (window k of one driver against window k
of the other, back to back). Every case asserts that both drivers return the same theta, status and lambda
bit for bit.

  exp_decay n 3, m 64      batch 4096, 64, 1; starts 1-2 % off the planted parameters (the README's curve fit)
  the same, mixed starts   batch 4096 and 64; starts 0.01 % .. 40 % off: iteration counts differ in the batch
  gaussian_peak m 256      batch 4096: four super-steps, the data are streamed again every iteration
  tanh n 16, m 64          batch 4096
  tanh n 64, m 512         batch 8192: the evaluation dominates
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nlsolver_amd  # noqa: E402
from nlsolver_amd import _capi  # noqa: E402

WINDOWS = 7
CH, RES = _capi.LM_CHOLESKY, _capi.LM_RESIDENT


def bits(result):
    theta, st, lam = result
    return (theta.view(np.uint64).tobytes(), b"".join(bytes(s) for s in st), lam.view(np.uint64).tobytes())


def spread(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def case(tag, model, x0, reps, **kw):
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    with nlsolver_amd.LMEngine(model, **kw) as eng:
        got = {}
        for name, solver in (("lock", CH), ("res", CH | RES)):  # warm-up, and the bits
            eng.set_solver(solver)
            got[name] = eng.minimize(x0.copy())
        assert bits(got["lock"]) == bits(got["res"]), tag
        lock, res = [], []
        for _ in range(WINDOWS):
            for solver, out in ((CH, lock), (CH | RES, res)):
                eng.set_solver(solver)
                out.append(eng.time_solve(x0, reps) / reps)
        ratios = [a / b for a, b in zip(lock, res)]
        it = np.array([s.iteration for s in got["lock"][1]])
        print(json.dumps(dict(case=tag, batch=int(x0.shape[0]), n=int(x0.shape[1]),
                              iterations=dict(min=int(it.min()), median=float(np.median(it)), max=int(it.max())),
                              ms_lock_step=spread(lock), ms_resident=spread(res),
                              lock_over_resident=spread(ratios, 3),
                              lock_over_resident_windows=[round(r, 3) for r in ratios],
                              windows=WINDOWS, solves_per_window=reps)), flush=True)


def decay(batch, mixed, m=64):
    rng = np.random.default_rng(1)
    t = np.tile(np.linspace(0.0, 4.0, m), (batch, 1))
    star = np.stack([rng.uniform(1.5, 3.0, batch), rng.uniform(0.5, 1.5, batch), rng.uniform(0.2, 0.8, batch)], axis=1)
    y = star[:, :1] * np.exp(-star[:, 1:2] * t) + star[:, 2:] + 0.01 * rng.uniform(-1, 1, (batch, m))
    off = 10.0 ** rng.uniform(-4, np.log10(0.4), batch) if mixed else rng.uniform(0.01, 0.02, batch)
    x0 = star * (1 + off[:, None] * rng.choice([-1.0, 1.0], (batch, 3)))
    return nlsolver_amd.CurveModel.exp_decay(t, y), x0


def peak(batch, m=256):
    rng = np.random.default_rng(2)
    t = np.tile(np.linspace(-3.0, 3.0, m), (batch, 1))
    star = np.stack([rng.uniform(1.0, 2.0, batch), rng.uniform(-0.5, 0.5, batch), rng.uniform(0.6, 1.0, batch),
                     rng.uniform(0.1, 0.3, batch)], axis=1)
    u = (t - star[:, 1:2]) / star[:, 2:3]
    y = star[:, :1] * np.exp(-0.5 * u * u) + star[:, 3:] + 0.01 * rng.uniform(-1, 1, (batch, m))
    x0 = star + rng.uniform(0.01, 0.02, (batch, 1)) * np.array([1.0, 1.0, 1.0, -1.0]) * np.abs(star)
    return nlsolver_amd.CurveModel.gaussian_peak(t, y), x0


def tanh(batch, n, m):
    rng = np.random.default_rng(3)
    A = rng.standard_normal((batch, m, n)) / np.sqrt(n)
    star = rng.uniform(-1, 1, (batch, n))
    y = np.tanh(np.einsum("bmn,bn->bm", A, star)) + 0.01 * rng.uniform(-1, 1, (batch, m))
    return nlsolver_amd.TanhRegression(A, y), star + 0.05 * rng.uniform(-1, 1, (batch, n))


if __name__ == "__main__":
    only = set(sys.argv[1:])
    cases = [
        ("exp_decay_4096", lambda: decay(4096, False), 20),
        ("exp_decay_64", lambda: decay(64, False), 50),
        ("exp_decay_1", lambda: decay(1, False), 50),
        ("exp_decay_mixed_4096", lambda: decay(4096, True), 20),
        ("exp_decay_mixed_64", lambda: decay(64, True), 50),
        ("gaussian_peak_m256_4096", lambda: peak(4096), 10),
        ("tanh_n16_m64_4096", lambda: tanh(4096, 16, 64), 10),
        ("tanh_n64_m512_8192", lambda: tanh(8192, 64, 512), 3),
    ]
    for tag, make, reps in cases:
        if not only or tag in only:
            model, x0 = make()
            case(tag, model, x0, reps)
