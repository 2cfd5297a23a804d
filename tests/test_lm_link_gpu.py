"""Levenberg-Marquardt regression models with a user-supplied link (LinkRegression, nlsg_lm_create_link):
the Gauss-Newton kernels instantiated at run time on phi / phi' given as source text.

1. LinkRegression.tanh is TanhRegression bit for bit (theta, every Status field, the final lambda), one
   shape per evaluation kernel, every m off the sixteen-row groups.
2. A link that is not tanh, exactly: phi = -tanh with targets -y negates every residual and Jacobian
   entry, so f, g, H and the whole run keep TanhRegression's bits.
3. The logistic link, phi(0) = 0.5: (a) started at the generating parameters f stays at rounding level
   -- a padded row that contributed phi(0)^2 = 0.25 would show at once; (b) against the numpy
   restatement of the reference's serial loop (tests/test_lm_link_cpu.py), within the bounds
   tests/test_lm_gpu.py holds the tanh engine to against that loop.
4. The C++ header's device::LinkRegression returns the Python drop-in's bits.

A link engine's first creation compiles its kernel (seconds); the library keeps the code object by
source text, so the engines of one link and kernel after the first cost a module load. Batch 3."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _oracle as O
from tests.test_lm_link_cpu import lm_link_solve, np_logistic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12374563468
B = 3
STATUS_FIELDS = ("f_value", "iteration", "function_calls_used", "gradient_evals_used", "hessian_evals_used",
                 "best_index", "val_no_change", "std_err", "done", "reserved")
KWS = [dict(lam=10.0, max_iter=6, f_delta=0.0), dict(max_iter=100, f_delta=1e-12)]
# (m, n): the narrow kernel, the narrow kernel at full width, the one-pass kernels to 128 and to 256
# columns, the super-block kernel; no m is a multiple of 16
SHAPES = [(20, 5), (50, 64), (70, 65), (140, 130), (270, 260)]


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


def status_tuple(st):
    return tuple(int(np.float64(getattr(st, f)).view(np.uint64)) if f in ("f_value", "std_err")
                 else int(getattr(st, f)) for f in STATUS_FIELDS)


_TANH_DATA = {}


def tanh_problems(oracle, m, n):
    if (m, n) not in _TANH_DATA:
        A, y, t0 = np.zeros((B, m, n)), np.zeros((B, m)), np.zeros((B, n))
        for b in range(B):
            A[b], y[b], t0[b] = O.tanh_problem(oracle, SEED, b, m, n)
        for a in (A, y, t0):
            a.setflags(write=False)
        _TANH_DATA[m, n] = (A, y, t0)
    return _TANH_DATA[m, n]


def run(mod, model, t0, solver=None, **kw):
    from nlsolver_amd import _capi
    with mod.LMEngine(model, solver=_capi.LM_CHOLESKY if solver is None else solver, **kw) as eng:
        th, st, lam = eng.minimize(t0.copy())
    return th, [status_tuple(s) for s in st], lam


def assert_same_run(got, want, tag):
    (th, st, lam), (th_w, st_w, lam_w) = got, want
    assert np.array_equal(bits(th), bits(th_w)), tag
    assert st == st_w, tag
    assert np.array_equal(bits(lam), bits(lam_w)), tag


# ---- 1. the tanh twin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", KWS, ids=["six", "converge"])
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"m{m}-n{n}" for m, n in SHAPES])
def test_the_tanh_link_is_the_built_in_engine_bit_for_bit(mod, oracle, m, n, kw):
    A, y, t0 = tanh_problems(oracle, m, n)
    want = run(mod, mod.TanhRegression(A, y), t0, **kw)
    got = run(mod, mod.LinkRegression.tanh(A, y), t0, **kw)
    assert_same_run(got, want, (m, n, kw))
    assert all(s[1] >= 3 for s in want[1])  # (iterations: the runs do iterate)


@pytest.mark.parametrize("kw", KWS, ids=["six", "converge"])
def test_the_tanh_link_with_the_qr_step(mod, oracle, kw):
    from nlsolver_amd import _capi
    A, y, t0 = tanh_problems(oracle, 20, 5)
    want = run(mod, mod.TanhRegression(A, y), t0, solver=_capi.LM_QR, **kw)
    got = run(mod, mod.LinkRegression.tanh(A, y), t0, solver=_capi.LM_QR, **kw)
    assert_same_run(got, want, kw)
    chol = run(mod, mod.TanhRegression(A, y), t0, **kw)
    assert not np.array_equal(bits(got[0]), bits(chol[0]))  # (it is the other step that ran)


def test_set_solver_and_the_timers_work_on_a_link_engine(mod, oracle):
    from nlsolver_amd import _capi
    A, y, t0 = tanh_problems(oracle, 20, 5)
    kw = KWS[0]
    with mod.LMEngine(mod.LinkRegression.tanh(A, y), **kw) as eng:
        eng.set_solver(_capi.LM_QR)
        got = eng.minimize(t0.copy())
        assert eng.time_solve(t0) > 0 and eng.time_eval_kernel(t0, 2) > 0 and eng.time_qr_kernel(t0, 2) > 0
        with pytest.raises(mod.NlsgError) as ei:   # as any engine without parameters
            eng.set_params(np.zeros((B, 1)))
        assert ei.value.code == 1
        row = np.zeros(B)
        assert _capi.lib().nlsg_lm_set_params(eng._h, row.ctypes.data_as(_capi.pd)) == 1
    want = run(mod, mod.TanhRegression(A, y), t0, solver=_capi.LM_QR, **kw)
    assert_same_run((got[0], [status_tuple(s) for s in got[1]], got[2]), want, "set_solver")


def test_a_body_that_does_not_compile_is_named(mod, oracle):
    A, y, t0 = tanh_problems(oracle, 20, 5)
    with pytest.raises(mod.NlsgError) as ei:
        mod.LMEngine(mod.LinkRegression(A, y, "return det_tanh(z);", "return 1 - v * w;"))
    assert ei.value.code == 1 and "slope_body" in str(ei.value)


# ---- 2. a link that is not tanh, exactly --------------------------------------------------------------
@pytest.mark.parametrize("kw", KWS, ids=["six", "converge"])
@pytest.mark.parametrize("m,n", [(20, 5), (70, 65)], ids=["m20-n5", "m70-n65"])
def test_the_negated_tanh_link_on_negated_targets(mod, oracle, m, n, kw):
    A, y, t0 = tanh_problems(oracle, m, n)
    want = run(mod, mod.TanhRegression(A, y), t0, **kw)
    neg = mod.LinkRegression(A, -y, "return -det_tanh(z);", "return -(1 - v * v);")
    assert_same_run(run(mod, neg, t0, **kw), want, (m, n, kw))


# ---- 3. the logistic link -----------------------------------------------------------------------------
_LOGISTIC_DATA = {}


def logistic_problems(m, n):
    """A = U(-1, 1) / sqrt(n), theta* = U(-1, 1), y = 1 / (1 + exp(-A theta*)), u = U(-1, 1)"""
    if (m, n) not in _LOGISTIC_DATA:
        rng = np.random.default_rng(7)
        A = rng.uniform(-1.0, 1.0, (B, m, n)) / np.sqrt(n)
        star = rng.uniform(-1.0, 1.0, (B, n))
        y = 1.0 / (1.0 + np.exp(-np.einsum("bmn,bn->bm", A, star)))
        t0 = 0.5 * star + 0.1 * rng.uniform(-1.0, 1.0, (B, n))
        for a in (A, star, y, t0):
            a.setflags(write=False)
        _LOGISTIC_DATA[m, n] = (A, star, y, t0)
    return _LOGISTIC_DATA[m, n]


@pytest.mark.parametrize("m,n", [(20, 5), (70, 65)], ids=["m20-n5", "m70-n65"])
def test_logistic_rows_past_m_contribute_nothing(mod, m, n):
    """from theta* the residuals are a few ulp of a number below 1 each: f <= m (8 * 2^-53)^2. One
    padded row at phi(0) = 0.5 would add 0.25 (m is no multiple of 16)."""
    A, star, y, _ = logistic_problems(m, n)
    th, st, lam = run(mod, mod.LinkRegression.logistic(A, y), star, max_iter=1, f_delta=0.0)
    bound = m * (8 * 2.0 ** -53) ** 2
    for b in range(B):
        f = float(np.uint64(st[b][0]).view(np.float64))
        print(f"m {m} n {n} problem {b}: f {f:.3e} (bound {bound:.3e}), iterations {st[b][1]}")
    for b in range(B):
        assert float(np.uint64(st[b][0]).view(np.float64)) <= bound, b
        assert st[b][1] == 1


_SERIAL = {}


def serial_logistic(m, n, b, k):
    """the restatement's run of problem b with max_iter k, computed once"""
    if (m, n, b, k) not in _SERIAL:
        A, _, y, t0 = logistic_problems(m, n)
        _SERIAL[m, n, b, k] = lm_link_solve(A[b], y[b], t0[b], *np_logistic(), lam=10.0, max_iter=k, f_delta=0.0)
    return _SERIAL[m, n, b, k]


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("m,n", [(48, 5), (70, 65)], ids=["m48-n5", "m70-n65"])
def test_logistic_against_the_serial_restatement(mod, m, n, k):
    A, _, y, t0 = logistic_problems(m, n)
    th, st, lam = run(mod, mod.LinkRegression.logistic(A, y), t0, lam=10.0, max_iter=k, f_delta=0.0)
    figures = []
    for b in range(B):
        f_ref, it_ref, x_ref, lam_ref = serial_logistic(m, n, b, k)
        f = float(np.uint64(st[b][0]).view(np.float64))
        figures.append((np.max(np.abs(th[b] - x_ref)), abs(f - f_ref) / f_ref, st[b][1], it_ref, lam[b], lam_ref))
        print(f"m {m} n {n} max_iter {k} problem {b}: |theta - ref| {figures[-1][0]:.3e}, f rel {figures[-1][1]:.3e}")
    for dx, df, it, it_ref, l, l_ref in figures:
        assert it == it_ref == k and l == l_ref
        assert dx <= 1e-12
        assert df <= 1e-12


# ---- 4. the C++ header --------------------------------------------------------------------------------
def test_header_link_regression_equals_the_drop_in(mod, tmp_path):
    from nlsolver_amd import _capi
    m, n = 20, 5
    A, _, y, t0 = logistic_problems(m, n)
    x = t0[0].copy()
    st = mod.LevenbergMarquardt(mod.LinkRegression.logistic(A[0], y[0])).minimize(x)
    assert st.iteration >= 3 and st.done == 1
    exe, data = str(tmp_path / "header_lm_link"), str(tmp_path / "problem.txt")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_lm_link.cpp"), "-o", exe, "-ldl"])
    with open(data, "w") as fh:
        fh.write(f"{m} {n}\n")
        for arr in (A[0], y[0], t0[0]):
            fh.write(" ".join(float(v).hex() for v in arr.ravel()) + "\n")
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    got = json.loads(subprocess.check_output([exe, data], env=env, text=True, timeout=300))
    assert np.array_equal(bits([float.fromhex(v) for v in got["x"]]), bits(x))
    assert bits(float.fromhex(got["f"])) == bits(st.f_value)
    assert (got["iters"], got["fcalls"], got["gcalls"], got["hcalls"]) == \
        (st.iteration, st.function_calls_used, st.gradient_evals_used, st.hessian_evals_used)
