"""Levenberg-Marquardt curve models (CurveModel, nlsg_lm_create_curve): the residual and its Jacobian row
given as one body of source, evaluated a lane per observation, J^T J on the matrix cores from an LDS tile.

Problems (batch 3, problem b; every y carries the noise 0.01 U(-1, 1), so that f at the optimum is a number
whose relative error means something):
  1. exponential decay, n 3, t = linspace(0, 4, m), theta* = (2 + 0.25 b, 0.7 + 0.1 b, 0.5),
     start theta* (0.8, 1.2, 0.9); m = 70, 64 and 1
  2. Gaussian peak, n 4, m 70, t = linspace(-3, 3, m), theta* = (1.5, 0.3 b - 0.2, 0.8, 0.2),
     start theta* + (0.2, 0.15, 0.1, -0.05)
  3. r = y - tanh(sum_j theta_j T_j(t)), the Chebyshev basis by recurrence in the body, t at the m
     Chebyshev nodes, theta* = U(-1, 1) / sqrt(n), start 0.5 theta* + 0.1 U(-1, 1) / sqrt(n);
     (m, n) = (70, 20), (70, 33), (150, 64): the padded column counts 32 and 64, full width, a third
     super-step with a partial last one

1. Against the serial numpy loop (tests/test_lm_curve_cpu.py lm_curve_solve), max_iter 1, 2, 3 and to
   convergence: iterations and final lambda equal, |theta - ref| <= 1e-12, |f - ref| <= 1e-12 ref — the
   bounds tests/test_lm_gpu.py and tests/test_lm_link_gpu.py hold the regression kernels to (to convergence,
   m = 1: an absolute bound on f, see the test).
2. The QR step against the Cholesky step of the same engine.
3. Problem 3 against TanhRegression on the basis built in numpy.
4. A linear model on small integers: f is numpy's, bit for bit; one more row adds its square exactly.
5. Rows past m contribute nothing, NaN and inf included.
6. The body rules: an unwritten J(j) is 0, a J(j) outside [0, n) is dropped, a typo is named.
7. Problem b alone has the bits it has in the batch.
8. The C++ header's device::CurveModel returns the Python drop-in's bits.

A curve engine's first creation compiles its kernel (seconds); the library keeps the code object by source
text."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_lm_curve_cpu import (chebyshev_basis, lm_curve_solve, rj_chebyshev_tanh, rj_exp_decay,
                                     rj_gaussian_peak)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3
CHEBYSHEV_TANH = """const double x = t(0);
double a = 1.0, b = x, z = 0.0;
for (int j = 0; j < n; j++) { z += a * th(j); const double c = 2.0 * x * b - a; a = b; b = c; }
const double v = det_tanh(z);
r = y - v;
const double w = 1 - v * v;
a = 1.0; b = x;
for (int j = 0; j < n; j++) { J(j) = -(w * a); const double c = 2.0 * x * b - a; a = b; b = c; }"""
LINEAR = "r = y - (th(0) + th(1) * t(0));\nJ(0) = -1.0;  J(1) = -t(0);"


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the problems: (t [B, m], y [B, m], start [B, n], rj), built once, read-only -----------------------
_DATA = {}


def problem(key):
    """key: ("exp", m), ("gauss", 70), ("cheb", m, n)"""
    if key not in _DATA:
        rng = np.random.default_rng(sum(map(ord, repr(key))))
        b = np.arange(B, dtype=np.float64)
        if key[0] == "exp":
            m = key[1]
            t = np.tile(np.linspace(0.0, 4.0, m), (B, 1))
            star = np.stack([2 + 0.25 * b, 0.7 + 0.1 * b, np.full(B, 0.5)], axis=1)
            start = star * np.array([0.8, 1.2, 0.9])
            rj = rj_exp_decay
        elif key[0] == "gauss":
            m = key[1]
            t = np.tile(np.linspace(-3.0, 3.0, m), (B, 1))
            star = np.stack([np.full(B, 1.5), 0.3 * b - 0.2, np.full(B, 0.8), np.full(B, 0.2)], axis=1)
            start = star + np.array([0.2, 0.15, 0.1, -0.05])
            rj = rj_gaussian_peak
        else:
            m, n = key[1:]
            t = np.tile(np.cos(np.pi * (2 * np.arange(m) + 1) / (2 * m)), (B, 1))
            star = rng.uniform(-1.0, 1.0, (B, n)) / np.sqrt(n)
            start = 0.5 * star + 0.1 * rng.uniform(-1.0, 1.0, (B, n)) / np.sqrt(n)
            rj = rj_chebyshev_tanh
        y = np.stack([-rj(t[i][:, None], np.zeros(t.shape[1]), star[i])[0] for i in range(B)])  # the model's values
        y = y + 0.01 * rng.uniform(-1.0, 1.0, y.shape)
        for a in (t, y, start):
            a.setflags(write=False)
        _DATA[key] = (t, y, start, rj)
    return _DATA[key]


def model_of(mod, key, t=None, y=None):
    t0, y0, _, _ = problem(key)
    t, y = t0 if t is None else t, y0 if y is None else y
    if key[0] == "exp":
        return mod.CurveModel.exp_decay(t, y)
    if key[0] == "gauss":
        return mod.CurveModel.gaussian_peak(t, y)
    return mod.CurveModel(t, y, CHEBYSHEV_TANH, key[2])


_SERIAL = {}


def serial(key, b, kw):
    """the yardstick's run of problem b, computed once"""
    tag = (key, b, tuple(sorted(kw.items())))
    if tag not in _SERIAL:
        t, y, start, rj = problem(key)
        _SERIAL[tag] = lm_curve_solve(rj, t[b][:, None], y[b], start[b], **kw)
    return _SERIAL[tag]


def run(mod, model, start, solver=None, **kw):
    """theta, [(f bits, iterations, done)], lambda"""
    from nlsolver_amd import _capi
    with mod.LMEngine(model, solver=_capi.LM_CHOLESKY if solver is None else solver, **kw) as eng:
        th, st, lam = eng.minimize(np.array(start))
    return th, st, lam


KEYS = [("exp", 70), ("exp", 64), ("exp", 1), ("gauss", 70), ("cheb", 70, 20), ("cheb", 70, 33), ("cheb", 150, 64)]
IDS = ["-".join(map(str, k)) for k in KEYS]


# ---- 1. against the yardstick -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_against_the_serial_loop(mod, key, k):
    kw = dict(lam=10.0, max_iter=k, f_delta=0.0)
    th, st, lam = run(mod, model_of(mod, key), problem(key)[2], **kw)
    figures = []
    for b in range(B):
        f_ref, it_ref, x_ref, lam_ref = serial(key, b, kw)
        figures.append((np.max(np.abs(th[b] - x_ref)), abs(st[b].f_value - f_ref) / f_ref, st[b].iteration, it_ref,
                        lam[b], lam_ref))
        print(f"{key} max_iter {k} problem {b}: |theta - ref| {figures[-1][0]:.3e}, f rel {figures[-1][1]:.3e}")
    for dx, df, it, it_ref, l, l_ref in figures:
        assert it == it_ref == k and l == l_ref
        assert dx <= 1e-12
        assert df <= 1e-12


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_to_convergence_against_the_serial_loop(mod, key):
    """The one-observation variant of problem 1 fits one number with three parameters exactly: the serial loop
    ends at f = 6e-28, a squared rounding error of which no digit is determined, so a relative bound on f
    decides nothing there. For that key alone f is held to an absolute bound instead, and theta to the 1e-12
    of the other runs. The bound: the only observation is at t = 0, where r = y - (theta0 + theta2) is linear
    in theta and a step takes r to r lambda / (4 + lambda) (J = (-1, 0, -1), 2 J^T J has the one eigenvalue
    4); lambda is 10 before the first step and falls tenfold with every decrease of f, so from the second
    step on f falls at least (1 / 5)^2 = 0.04-fold per step. The stop test needs prev - cur < 1e-12, hence
    prev < 1e-12 / 0.96 and the final f < 0.04 * 1.05e-12 < 1e-13."""
    kw = dict(lam=10.0, max_iter=100, f_delta=1e-12)
    th, st, lam = run(mod, model_of(mod, key), problem(key)[2], **kw)
    exact_fit = key == ("exp", 1)
    figures = []
    for b in range(B):
        f_ref, it_ref, x_ref, lam_ref = serial(key, b, kw)
        figures.append((abs(st[b].f_value - f_ref) / f_ref, st[b].iteration, it_ref, st[b].done, st[b].f_value,
                        np.max(np.abs(th[b] - x_ref))))
        print(f"{key} problem {b}: iterations {st[b].iteration} (ref {it_ref}), f {st[b].f_value:.3e} (ref {f_ref:.3e}), "
              f"f rel {figures[-1][0]:.3e}, |theta - ref| {figures[-1][5]:.3e}")
    for df, it, it_ref, done, f, dx in figures:
        assert it == it_ref and 1 <= it < 100 and done == 1
        if exact_fit:
            assert 0.0 <= f <= 1e-13 and dx <= 1e-12
        else:
            assert df <= 1e-12


def test_the_status_counts_are_a_tanh_engines(mod):
    key = ("exp", 70)
    th, st, lam = run(mod, model_of(mod, key), problem(key)[2], lam=10.0, max_iter=3, f_delta=0.0)
    for b in range(B):
        s = st[b]
        assert (s.iteration, s.function_calls_used, s.gradient_evals_used, s.hessian_evals_used) == (3, 4, 4, 4)
        assert (s.best_index, s.val_no_change, s.done, s.reserved) == (b, 0, 1, 0) and s.std_err == lam[b]


# ---- 2. the QR step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("key", [("exp", 70), ("cheb", 70, 20)], ids=["exp-70", "cheb-70-20"])
def test_the_qr_step_against_the_cholesky_step(mod, key, k):
    from nlsolver_amd import _capi
    start = problem(key)[2]
    with mod.LMEngine(model_of(mod, key), lam=10.0, max_iter=k, f_delta=0.0) as eng:
        chol = eng.minimize(np.array(start))
        eng.set_solver(_capi.LM_QR)
        qr = eng.minimize(np.array(start))
        eng.set_solver(_capi.LM_CHOLESKY)
        again = eng.minimize(np.array(start))
    fresh = run(mod, model_of(mod, key), start, solver=_capi.LM_QR, lam=10.0, max_iter=k, f_delta=0.0)
    print(f"{key} max_iter {k}: |theta_qr - theta_chol| {np.max(np.abs(qr[0] - chol[0])):.3e}")
    assert np.max(np.abs(qr[0] - chol[0])) <= 1e-12
    assert not np.array_equal(bits(qr[0]), bits(chol[0]))       # (it is the other step that ran)
    assert np.array_equal(bits(again[0]), bits(chol[0]))        # set_solver switches back as well
    assert np.array_equal(bits(fresh[0]), bits(qr[0]))          # and an engine made with LM_QR agrees
    assert all(s.iteration == k for s in qr[1])


def test_the_timers_work_on_a_curve_engine_and_the_other_setters_name_the_right_call(mod):
    from nlsolver_amd import _capi
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    with mod.LMEngine(model_of(mod, key), lam=10.0, max_iter=3, f_delta=0.0) as eng:
        assert eng.time_solve(start) > 0 and eng.time_eval_kernel(start, 2) > 0 and eng.time_qr_kernel(start, 2) > 0
        lib = _capi.lib()
        assert lib.nlsg_lm_set_data(eng._h, t.ctypes.data_as(_capi.pd), y.ctypes.data_as(_capi.pd)) == 1
        assert "nlsg_lm_set_curve_data" in lib.nlsg_last_error().decode()
        assert lib.nlsg_lm_set_params(eng._h, y.ctypes.data_as(_capi.pd)) == 1
        assert "nlsg_lm_set_curve_data" in lib.nlsg_last_error().decode()
        with pytest.raises(mod.NlsgError) as ei:
            eng.set_params(np.zeros((B, 1)))
        assert ei.value.code == 1
    A = np.zeros((B, 20, 5))
    with mod.LMEngine(mod.TanhRegression(A, np.zeros((B, 20)))) as eng:   # and the new setter on another engine
        assert _capi.lib().nlsg_lm_set_curve_data(eng._h, A.ctypes.data_as(_capi.pd), A.ctypes.data_as(_capi.pd)) == 1


# ---- 3. device against device -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("key", [("cheb", 70, 20), ("cheb", 150, 64)], ids=["cheb-70-20", "cheb-150-64"])
def test_the_chebyshev_body_against_tanh_regression_on_the_basis(mod, key, k):
    t, y, start, _ = problem(key)
    A = np.stack([chebyshev_basis(t[b], key[2]) for b in range(B)])
    kw = dict(lam=10.0, max_iter=k, f_delta=0.0)
    want = run(mod, mod.TanhRegression(A, y), start, **kw)
    got = run(mod, model_of(mod, key), start, **kw)
    for b in range(B):
        dx = np.max(np.abs(got[0][b] - want[0][b]))
        df = abs(got[1][b].f_value - want[1][b].f_value) / want[1][b].f_value
        print(f"{key} max_iter {k} problem {b}: |theta - tanh engine's| {dx:.3e}, f rel {df:.3e}")
    for b in range(B):
        assert got[1][b].iteration == want[1][b].iteration == k and got[2][b] == want[2][b]
        assert np.max(np.abs(got[0][b] - want[0][b])) <= 1e-12
        assert abs(got[1][b].f_value - want[1][b].f_value) <= 1e-12 * want[1][b].f_value


# ---- 4. exact evaluation ------------------------------------------------------------------------------
def test_a_linear_model_on_small_integers_is_exact(mod):
    """every product and sum is an integer below 2^53: f is exact whatever the order of the sums"""
    rng = np.random.default_rng(11)
    m = 70
    t = rng.integers(-8, 9, (B, m + 1)).astype(np.float64)
    y = rng.integers(-20, 21, (B, m + 1)).astype(np.float64)
    th = rng.integers(-3, 4, (B, 2)).astype(np.float64)

    def f_of(rows):
        model = mod.CurveModel(t[:, :rows], y[:, :rows], LINEAR, 2)
        _, st, _ = run(mod, model, th, max_iter=0)
        assert all(s.iteration == 0 for s in st)
        return np.array([s.f_value for s in st])

    f70, f71 = f_of(m), f_of(m + 1)
    r = y - (th[:, :1] + th[:, 1:] * t)
    assert np.array_equal(bits(f70), bits(np.sum(r[:, :m] ** 2, axis=1)))
    assert np.array_equal(bits(f71), bits(np.sum(r ** 2, axis=1)))
    assert np.array_equal(f71 - f70, r[:, m] ** 2) and np.all(f70 > 0)   # the row that was padding counts once


# ---- 5. rows past m -----------------------------------------------------------------------------------
def test_rows_past_m_contribute_nothing(mod):
    """r = y - (1 + theta0 tanh(theta1 t)) is -1 on a padded row's zeros. From the generating theta of
    noiseless data every residual is a few ulp of a number below 1: f <= m (8 * 2^-53)^2; one padded row
    would add 1 (m = 70 leaves 58 of them)."""
    m = 70
    t = np.tile(np.linspace(0.1, 3.0, m), (B, 1))
    star = np.array([[-0.5, 0.8], [-0.4, 1.1], [-0.3, 0.6]])
    y = 1.0 + star[:, :1] * np.tanh(star[:, 1:] * t)
    body = ("const double v = det_tanh(th(1) * t(0));\nr = y - (1.0 + th(0) * v);\n"
            "J(0) = -v;  J(1) = -(th(0) * (1 - v * v) * t(0));")
    th, st, lam = run(mod, mod.CurveModel(t, y, body, 2), star, max_iter=1, f_delta=0.0)
    bound = m * (8 * 2.0 ** -53) ** 2
    for b in range(B):
        print(f"problem {b}: f {st[b].f_value:.3e} (bound {bound:.3e}), iterations {st[b].iteration}")
    for b in range(B):
        assert st[b].f_value <= bound and st[b].iteration == 1


def test_a_body_that_is_not_finite_on_zero_data_stays_finite(mod):
    """log(0) on every padded row: masked by a select, so no inf or NaN reaches f, g or H"""
    m = 70
    t = np.tile(np.linspace(0.5, 3.0, m), (B, 1))
    rng = np.random.default_rng(5)
    y = np.array([[0.7], [1.1], [-0.4]]) * np.log(t) + 0.01 * rng.uniform(-1, 1, t.shape)
    body = "const double l = det_log(t(0));\nr = y - th(0) * l + 0.0 * l;\nJ(0) = -l;"
    th, st, lam = run(mod, mod.CurveModel(t, y, body, 1), np.full((B, 1), 0.5), lam=10.0, max_iter=3, f_delta=0.0)
    want = [lm_curve_solve(lambda t, y, x: (y - x[0] * np.log(t[:, 0]), -np.log(t)), t[b][:, None], y[b], [0.5],
                           lam=10.0, max_iter=3, f_delta=0.0) for b in range(B)]
    for b in range(B):
        print(f"problem {b}: f {st[b].f_value:.6e} (serial loop {want[b][0]:.6e}), theta {th[b, 0]:.6f}")
    for b in range(B):
        assert np.isfinite(st[b].f_value) and np.all(np.isfinite(th[b]))
        assert abs(st[b].f_value - want[b][0]) <= 1e-12 * want[b][0] and abs(th[b, 0] - want[b][2][0]) <= 1e-12


# ---- 6. the body rules --------------------------------------------------------------------------------
def test_an_unwritten_jacobian_entry_is_zero(mod):
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    body = mod.CurveModel.exp_decay(t, y).body.replace("  J(2) = -1.0;", "")
    assert "J(2)" not in body and "J(1)" in body
    th, st, lam = run(mod, mod.CurveModel(t, y, body, 3), start, lam=10.0, max_iter=3, f_delta=0.0)
    assert np.array_equal(bits(th[:, 2]), bits(start[:, 2]))
    assert np.all(th[:, 0] != start[:, 0]) and np.all(th[:, 1] != start[:, 1])


def test_jacobian_entries_outside_the_parameters_are_dropped(mod):
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    kw = dict(lam=10.0, max_iter=3, f_delta=0.0)
    want = run(mod, model_of(mod, key), start, **kw)
    body = mod.CurveModel.exp_decay(t, y).body + "\nJ(n) = 1.0;\nJ(-1) = 1.0;\nJ(3) = 1.0;"
    got = run(mod, mod.CurveModel(t, y, body, 3), start, **kw)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[2]), bits(want[2]))
    assert [bits(s.f_value) for s in got[1]] == [bits(s.f_value) for s in want[1]]


def test_a_body_that_does_not_compile_is_named(mod):
    key = ("exp", 70)
    t, y, _, _ = problem(key)
    with pytest.raises(mod.NlsgError) as ei:
        mod.LMEngine(mod.CurveModel(t, y, "const double e = det_exp(-th(1) * t(0));\nr = y - ee;", 3))
    assert ei.value.code == 1 and "curve_body" in str(ei.value)


# ---- 7. batch independence ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("exp", 70), ("cheb", 150, 64)], ids=["exp-70", "cheb-150-64"])
def test_a_problem_alone_has_its_bits_in_the_batch(mod, key):
    t, y, start, _ = problem(key)
    kw = dict(lam=10.0, max_iter=3, f_delta=0.0)
    th, st, lam = run(mod, model_of(mod, key), start, **kw)
    for b in range(B):
        th1, st1, lam1 = run(mod, model_of(mod, key, t[b:b + 1], y[b:b + 1]), start[b:b + 1], **kw)
        assert np.array_equal(bits(th1[0]), bits(th[b])), b
        assert bits(st1[0].f_value) == bits(st[b].f_value) and lam1[0] == lam[b], b


# ---- 8. the C++ header --------------------------------------------------------------------------------
def test_header_curve_model_equals_the_drop_in(mod, tmp_path):
    from nlsolver_amd import _capi
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    x = start[0].copy()
    st = mod.LevenbergMarquardt(mod.CurveModel.exp_decay(t[0], y[0])).minimize(x)
    assert st.iteration >= 3 and st.done == 1
    exe, data = str(tmp_path / "header_lm_curve"), str(tmp_path / "problem.txt")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_lm_curve.cpp"), "-o", exe, "-ldl"])
    with open(data, "w") as fh:
        fh.write(f"{t.shape[1]}\n")
        for arr in (t[0], y[0], start[0]):
            fh.write(" ".join(float(v).hex() for v in arr.ravel()) + "\n")
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    got = json.loads(subprocess.check_output([exe, data], env=env, text=True, timeout=300))
    assert np.array_equal(bits([float.fromhex(v) for v in got["x"]]), bits(x))
    assert bits(float.fromhex(got["f"])) == bits(st.f_value)
    assert (got["iters"], got["fcalls"], got["gcalls"], got["hcalls"]) == \
        (st.iteration, st.function_calls_used, st.gradient_evals_used, st.hessian_evals_used)
