"""Parameter covariance of a Levenberg-Marquardt fit on the device (lm_cov_kernel, nlsg_lm_covariance,
LMEngine.covariance / stderr, the header's LevenbergMarquardt::covariance). Batch 3 throughout.

1. Exact cases, bit for bit (tests/test_lm_cov_cpu.py proves that every intermediate value of them is a
   dyadic number of at most 40 bits, so any order of operations, fused or not, must return the rational
   inverse): LinkRegression.identity at n = 1, 2, 5, 33, 64 in both modes, at theta = 0 and at an integer
   theta with y shifted; TanhRegression at theta = 0 (the built-in kernel's Hg); a linear CurveModel (the
   curve kernel's Hg); m = n.
2. Failure is local: a zero pivot (two identical columns, an all-zero column) or a NaN in y (residual
   mode) gives ok = 0 and 25 NaN for that problem; its neighbours keep the bits they have alone.
3. Rounded cases against the exact inverse of the exact Gram matrix of the host's float64 J
   (enclosed_inverse), max |cov - exact| <= C kappa_2(G) 2^-52 max |exact|: C = 4 where J is data, C = 16
   where the body calls det_* functions (the host's J then differs from the device's by the few ulp
   tests/test_math_accuracy_* allow, amplified by kappa). Every ratio err / (kappa eps) is printed.
4. The call leaves the engine as it was; the solver does not enter; a problem alone has its bits in the
   batch; symmetry; stderr.
5. Refusals.
6. Recycled, poisoned pool blocks (a child process).
7. The C++ header returns the Python drop-in's bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_lm_cov_cpu import B, EXACT_N, enclosed_inverse, exact_batch
from tests.test_lm_curve_cpu import chebyshev_basis
from tests.test_lm_curve_gpu import model_of, problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
LINEAR5 = """double z = 0.0;
#pragma unroll
for (int j = 0; j < 5; j++) { z += th(j) * t(j);  J(j) = -t(j); }
r = y - z;"""


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


def same(a, b):
    """bit for bit, NaN payloads aside"""
    return np.array_equal(a, b, equal_nan=True)


def covariance(mod, model, theta, scale, **kw):
    """(cov, s2, ok) of a fresh engine; the symmetry every result must have is checked here"""
    with mod.LMEngine(model, **kw) as eng:
        cov, s2, ok = eng.covariance(theta, scale)
    assert cov.shape == (theta.shape[0], theta.shape[1], theta.shape[1]) and s2.shape == ok.shape == theta.shape[:1]
    assert ok.dtype == np.bool_
    assert same(cov, cov.transpose(0, 2, 1)), "cov is not bitwise symmetric"
    return cov, s2, ok


# ---- 1. exact cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EXACT_N)
def test_identity_link_is_exact_in_both_modes(mod, n):
    A, y, ginv = exact_batch(n)
    with mod.LMEngine(mod.LinkRegression.identity(A, y)) as eng:
        theta = np.zeros((B, n))
        for scale, c in (("absolute", 1.0), ("residual", 4.0), (mod._capi.LM_COV_ABSOLUTE, 1.0),
                         (mod._capi.LM_COV_RESIDUAL, 4.0)):
            cov, s2, ok = eng.covariance(theta, scale)
            assert ok.all() and np.array_equal(s2, np.full(B, 4.0))
            assert np.array_equal(cov, c * ginv), (scale, np.max(np.abs(cov - c * ginv)))
            assert np.array_equal(cov, cov.transpose(0, 2, 1))


@pytest.mark.parametrize("n", EXACT_N)
def test_identity_link_is_exact_at_an_integer_theta(mod, n):
    """the model is linear: with y shifted by A theta (small integers, exact) r and J are what they were"""
    A, y, ginv = exact_batch(n)
    theta = np.random.default_rng(n).integers(-3, 4, (B, n)).astype(np.float64)
    theta[:, 0] = 2.0  # (not zero)
    y2 = y + np.einsum("bij,bj->bi", A, theta)
    for scale, c in (("absolute", 1.0), ("residual", 4.0)):
        cov, s2, ok = covariance(mod, mod.LinkRegression.identity(A, y2), theta, scale)
        assert ok.all() and np.array_equal(s2, np.full(B, 4.0))
        assert np.array_equal(cov, c * ginv), scale


def test_tanh_regression_at_zero_is_exact(mod):
    """the slope at theta = 0 is 1 - tanh(0)^2 = 1 exactly: J = -A, from the built-in kernel"""
    A, y, ginv = exact_batch(33)
    for scale, c in (("absolute", 1.0), ("residual", 4.0)):
        cov, s2, ok = covariance(mod, mod.TanhRegression(A, y), np.zeros((B, 33)), scale)
        assert ok.all() and np.array_equal(s2, np.full(B, 4.0))
        assert np.array_equal(cov, c * ginv), scale


def test_a_linear_curve_model_is_exact(mod):
    """r = y - sum_j th(j) t(j) with the design matrix's rows as the observations' data: the curve kernel's Hg"""
    A, y, ginv = exact_batch(5)
    for scale, c in (("absolute", 1.0), ("residual", 4.0)):
        cov, s2, ok = covariance(mod, mod.CurveModel(A, y, LINEAR5, 5), np.zeros((B, 5)), scale)
        assert ok.all() and np.array_equal(s2, np.full(B, 4.0))
        assert np.array_equal(cov, c * ginv), scale


@pytest.mark.parametrize("n", [5, 33])
def test_m_equal_n_is_exact_in_absolute_mode_and_refused_in_residual_mode(mod, n):
    A, y, ginv = exact_batch(n, pad=0)
    assert A.shape == (B, n, n)
    with mod.LMEngine(mod.LinkRegression.identity(A, y)) as eng:
        cov, s2, ok = eng.covariance(np.zeros((B, n)), "absolute")
        assert ok.all() and np.array_equal(cov, ginv) and np.all(np.isnan(s2))  # no residual variance at m = n
        with pytest.raises(mod.NlsgError) as ei:
            eng.covariance(np.zeros((B, n)), "residual")
        assert ei.value.code == 1 and "m > n" in str(ei.value)


# ---- 2. failure is local ------------------------------------------------------------------------------
def _alone(mod, A, y, b, scale):
    return covariance(mod, mod.LinkRegression.identity(A[b:b + 1], y[b:b + 1]), np.zeros((1, A.shape[2])), scale)


@pytest.mark.parametrize("what", ["identical columns", "zero column", "nan in y"])
def test_a_failed_problem_is_all_nan_and_leaves_its_neighbours_alone(mod, what):
    A, y, ginv = (np.array(a) for a in exact_batch(5))
    scale = "absolute"
    if what == "identical columns":
        A[1, :, 3] = A[1, :, 1]  # integers: the pivot is exactly 0
    elif what == "zero column":
        A[1, :, 2] = 0.0
    else:
        y[1, 6] = np.nan
        scale = "residual"
    cov, s2, ok = covariance(mod, mod.LinkRegression.identity(A, y), np.zeros((B, 5)), scale)
    assert ok.tolist() == [True, False, True]
    assert np.all(np.isnan(cov[1])) and cov[1].size == 25
    c = 4.0 if scale == "residual" else 1.0
    for b in (0, 2):
        alone = _alone(mod, A, y, b, scale)
        assert np.array_equal(bits(cov[b]), bits(alone[0][0])) and bits(s2[b]) == bits(alone[1][0]) and alone[2][0]
        assert np.array_equal(cov[b], c * ginv[b])
    if what == "nan in y":  # J does not depend on y: in absolute mode the problem has its covariance
        cov_a, _, ok_a = covariance(mod, mod.LinkRegression.identity(A, y), np.zeros((B, 5)), "absolute")
        assert ok_a.all() and np.array_equal(cov_a, ginv) and np.isnan(s2[1])


# ---- 3. rounded cases ---------------------------------------------------------------------------------
_EXACT = {}


def expected(tag, J):
    """per problem: (the exact inverse of the exact J^T J rounded once, kappa_2 of J^T J); computed once"""
    if tag not in _EXACT:
        _EXACT[tag] = [(enclosed_inverse(Jb), np.linalg.cond(Jb.T @ Jb)) for Jb in J]
    return _EXACT[tag]


def check_rounded(tag, cov, J, C):
    worst = 0.0
    for b, (want, kappa) in enumerate(expected(tag, J)):
        ratio = np.max(np.abs(cov[b] - want)) / (kappa * EPS * np.max(np.abs(want)))
        print(f"{tag} problem {b}: kappa {kappa:.3e}, err / (kappa eps) = {ratio:.3f} (bound {C})")
        worst = max(worst, ratio)
    assert worst <= C, (tag, worst)


def data_problem(key):
    """J is data: U(-1, 1) rows, or the Chebyshev basis at the Chebyshev nodes"""
    kind, m, n = key
    rng = np.random.default_rng(100 * m + n)
    if kind == "uniform":
        A = rng.uniform(-1.0, 1.0, (B, m, n))
    else:
        t = np.cos(np.pi * (2 * np.arange(m) + 1) / (2 * m))
        A = np.stack([chebyshev_basis(t * (1.0 - 0.01 * b), n) for b in range(B)])
    theta = rng.uniform(-1.0, 1.0, (B, n)) / np.sqrt(n)
    y = np.einsum("bij,bj->bi", A, theta) + 0.01 * rng.uniform(-1.0, 1.0, (B, m))
    return A, y, theta


@pytest.mark.parametrize("key", [("uniform", 70, 20), ("uniform", 150, 64), ("chebyshev", 70, 33)],
                         ids=["uniform-70-20", "uniform-150-64", "chebyshev-70-33"])
def test_a_data_jacobian_against_the_exact_inverse(mod, key):
    A, y, theta = data_problem(key)
    m, n = key[1:]
    with mod.LMEngine(mod.LinkRegression.identity(A, y), max_iter=0) as eng:
        cov, s2, ok = eng.covariance(theta, "absolute")
        cov_r, s2_r, ok_r = eng.covariance(theta, "residual")
        f = np.array([s.f_value for s in eng.minimize(theta.copy())[1]])  # max_iter 0: f at theta
    assert ok.all() and ok_r.all()
    check_rounded(repr(key), cov, -A, 4)
    # residual mode is the same inverse times the engine's own f / (m - n), one rounding each
    assert np.array_equal(bits(s2), bits(f / (m - n))) and np.array_equal(bits(s2_r), bits(s2))
    assert np.array_equal(bits(cov_r), bits(s2[:, None, None] * cov))
    r = y - np.einsum("bij,bj->bi", A, theta)
    assert np.max(np.abs(f - np.sum(r * r, axis=1)) / f) <= 1e-12


CURVES = [("exp", 70), ("exp", 64), ("exp", 4), ("gauss", 70), ("cheb", 70, 20)]


@pytest.mark.parametrize("key", CURVES, ids=["-".join(map(str, k)) for k in CURVES])
def test_a_curve_models_jacobian_against_the_exact_inverse(mod, key):
    """at the fit the engine itself returns: theta-hat from minimize, the host's J there"""
    t, y, start, rj = problem(key)
    with mod.LMEngine(model_of(mod, key)) as eng:
        theta, st, _ = eng.minimize(np.array(start))
        cov, s2, ok = eng.covariance(theta, "absolute")
    assert ok.all() and all(s.done == 1 for s in st)
    J = [rj(t[b][:, None], y[b], theta[b])[1] for b in range(B)]
    check_rounded(repr(key), cov, J, 16)
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    m, n = t.shape[1], theta.shape[1]
    f = np.array([s.f_value for s in st])
    assert np.max(np.abs(s2 - f / (m - n)) / s2) <= 1e-12  # (f at theta-hat, evaluated again)


# ---- 4. engine state and independence -----------------------------------------------------------------
@pytest.mark.parametrize("key", [("exp", 70), ("cheb", 70, 20)], ids=["exp-70", "cheb-70-20"])
def test_a_solve_after_the_call_is_the_solve_without_it(mod, key):
    start = problem(key)[2]
    with mod.LMEngine(model_of(mod, key)) as eng:
        first = eng.minimize(np.array(start))
        eng.covariance(first[0], "residual")
        second = eng.minimize(np.array(start))
    fields = lambda s: (bits(s.f_value).item(), s.iteration, s.function_calls_used, s.gradient_evals_used,
                        s.hessian_evals_used, s.best_index, s.val_no_change, bits(s.std_err).item(), s.done, s.reserved)
    assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(bits(first[2]), bits(second[2]))
    assert [fields(s) for s in first[1]] == [fields(s) for s in second[1]]


def test_the_solver_does_not_enter(mod):
    from nlsolver_amd import _capi
    key = ("exp", 70)
    start = problem(key)[2]
    with mod.LMEngine(model_of(mod, key)) as eng:
        theta = eng.minimize(np.array(start))[0]
        chol = eng.covariance(theta)
        eng.set_solver(_capi.LM_QR)
        qr = eng.covariance(theta)
    fresh = covariance(mod, model_of(mod, key), theta, "residual", solver=_capi.LM_QR)
    for got in (qr, fresh):
        assert np.array_equal(bits(got[0]), bits(chol[0])) and np.array_equal(bits(got[1]), bits(chol[1]))
        assert got[2].all()


def test_a_problem_alone_has_its_bits_in_the_batch(mod):
    A, y, ginv = exact_batch(33)
    cov, s2, ok = covariance(mod, mod.LinkRegression.identity(A, y), np.zeros((B, 33)), "residual")
    for b in range(B):
        alone = _alone(mod, A, y, b, "residual")
        assert np.array_equal(bits(alone[0][0]), bits(cov[b])) and bits(alone[1][0]) == bits(s2[b])
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    cov, s2, ok = covariance(mod, model_of(mod, key), np.array(start), "residual")
    for b in range(B):
        alone = covariance(mod, model_of(mod, key, t[b:b + 1], y[b:b + 1]), np.array(start[b:b + 1]), "residual")
        assert np.array_equal(bits(alone[0][0]), bits(cov[b])) and bits(alone[1][0]) == bits(s2[b]), b


def test_stderr_is_the_root_of_the_diagonal(mod):
    """one rounding in the root (relative 2^-53), doubled by the square, and the square's own: se^2 is
    within 4 * 2^-53 of the diagonal. A failed problem's row is NaN."""
    A, y, _ = (np.array(a) for a in exact_batch(5))
    A[1, :, 3] = A[1, :, 1]
    theta = np.zeros((B, 5))
    with mod.LMEngine(mod.LinkRegression.identity(A, y)) as eng:
        cov, _, ok = eng.covariance(theta, "residual")
        se = eng.stderr(theta, "residual")
    assert se.shape == (B, 5) and ok.tolist() == [True, False, True]
    diag = np.diagonal(cov, axis1=1, axis2=2)
    assert same(se, np.sqrt(diag)) and np.all(np.isnan(se[1]))
    assert np.all(np.abs(se[[0, 2]] ** 2 - diag[[0, 2]]) <= 4 * 2.0 ** -53 * diag[[0, 2]])
    assert np.all(diag[[0, 2]] > 0)


def test_the_drop_in_takes_one_point_or_a_batch(mod):
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    want = covariance(mod, model_of(mod, key), np.array(start), "absolute")[0]
    lm = mod.LevenbergMarquardt(model_of(mod, key))
    assert np.array_equal(bits(lm.covariance(np.array(start), "absolute")), bits(want))
    one = mod.LevenbergMarquardt(mod.CurveModel.exp_decay(t[1], y[1]))
    cov1 = one.covariance(np.array(start[1]), scale="absolute")
    assert cov1.shape == (3, 3) and np.array_equal(bits(cov1), bits(want[1]))
    assert same(one.stderr(np.array(start[1]), scale="absolute"), np.sqrt(np.diag(want[1])))


# ---- 5. refusals --------------------------------------------------------------------------------------
def test_more_than_64_parameters_are_unsupported(mod):
    rng = np.random.default_rng(65)
    A, y = rng.uniform(-1, 1, (B, 80, 65)), rng.uniform(-1, 1, (B, 80))
    with mod.LMEngine(mod.TanhRegression(A, y)) as eng:
        with pytest.raises(mod.NlsgError) as ei:
            eng.covariance(np.zeros((B, 65)))
    assert ei.value.code == 2 and "n = 65 > 64" in str(ei.value)


def test_a_default_functor_engine_is_unsupported(mod):
    with mod.LMEngine("sphere", batch=3, n=4) as eng:
        with pytest.raises(mod.NlsgError) as ei:
            eng.covariance(np.ones((3, 4)))
    assert ei.value.code == 2 and "finite-difference Hessian" in str(ei.value)


def test_an_unknown_scale_and_missing_data_through_the_c_abi(mod):
    import ctypes as C
    from nlsolver_amd import _capi
    lib = _capi.lib()
    A, y, _ = exact_batch(5)
    theta, cov = np.zeros((B, 5)), np.zeros((B, 5, 5))
    pd = _capi.pd
    with mod.LMEngine(mod.TanhRegression(A, y)) as eng:
        assert lib.nlsg_lm_covariance(eng._h, theta.ctypes.data_as(pd), 2, cov.ctypes.data_as(pd), None, None) == 1
        assert b"unknown scale 2" in lib.nlsg_last_error()
        assert lib.nlsg_lm_covariance(eng._h, None, 0, cov.ctypes.data_as(pd), None, None) == 1
        cfg = eng.cfg
        h = C.c_void_p()
        _capi.check(lib.nlsg_lm_create(C.byref(cfg), C.byref(h)))  # a second engine, its data never set
        try:
            assert lib.nlsg_lm_covariance(h, theta.ctypes.data_as(pd), 0, cov.ctypes.data_as(pd), None, None) == 6
            assert b"nlsg_lm_set_data has not been called" in lib.nlsg_last_error()
        finally:
            lib.nlsg_lm_destroy(h)


# ---- 6. recycled memory -------------------------------------------------------------------------------
def child_recycled_blocks(m):
    """after a first engine has come and gone, so that the blocks are recycled ones"""
    A, y, ginv = exact_batch(33)
    with m.LMEngine(m.LinkRegression.identity(A, y)) as eng:
        eng.covariance(np.zeros((B, 33)), "residual")
    for _ in range(2):
        cov, s2, ok = covariance(m, m.LinkRegression.identity(A, y), np.zeros((B, 33)), "residual")
        assert ok.all() and np.array_equal(s2, np.full(B, 4.0)) and np.array_equal(cov, 4.0 * ginv)
    A5, y5, ginv5 = (np.array(a) for a in exact_batch(5))
    A5[1, :, 3] = A5[1, :, 1]
    for _ in range(2):
        cov, s2, ok = covariance(m, m.LinkRegression.identity(A5, y5), np.zeros((B, 5)), "absolute")
        assert ok.tolist() == [True, False, True] and np.all(np.isnan(cov[1]))
        assert np.array_equal(cov[[0, 2]], ginv5[[0, 2]]) and np.array_equal(s2, np.full(B, 4.0))


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
from nlsolver_amd import _capi
assert _capi.lib().nlsg_pool_poison() == 0xC0, _capi.lib().nlsg_pool_poison()
import nlsolver_amd
from tests import test_lm_cov_gpu as T
T.child_recycled_blocks(nlsolver_amd)
print("poison-ok")
"""


def test_recycled_poisoned_blocks_change_nothing(mod):
    """0xC0: a finite double (-8577.5...), so a byte the kernel did not write shows in the singular
    problem's NaN block as well as in the exact values"""
    env = dict(os.environ, NLSG_POOL_POISON="0xC0")
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0 and "poison-ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---- 7. the C++ header --------------------------------------------------------------------------------
def test_header_covariance_equals_the_drop_in(mod, tmp_path):
    from nlsolver_amd import _capi
    key = ("exp", 70)
    t, y, start, _ = problem(key)
    x = start[0].copy()
    lm = mod.LevenbergMarquardt(mod.CurveModel.exp_decay(t[0], y[0]))
    assert lm.minimize(x).done == 1
    want = {s: lm.covariance(x, s) for s in ("residual", "absolute")}
    exe, data = str(tmp_path / "header_lm_cov"), str(tmp_path / "problem.txt")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_lm_cov.cpp"), "-o", exe, "-ldl"])
    with open(data, "w") as fh:
        fh.write(f"{t.shape[1]}\n")
        for arr in (t[0], y[0], x):
            fh.write(" ".join(float(v).hex() for v in arr.ravel()) + "\n")
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    got = json.loads(subprocess.check_output([exe, data], env=env, text=True, timeout=300))
    unhex = lambda name: np.array([float.fromhex(v) for v in got[name]]).reshape(3, 3)
    assert np.array_equal(bits(unhex("residual")), bits(want["residual"]))
    assert np.array_equal(bits(unhex("absolute")), bits(want["absolute"]))
    assert np.array_equal(bits(unhex("batch")), bits(want["residual"])) and got["ok"] == 1
    assert np.all(np.isfinite(want["residual"])) and np.all(np.diag(want["residual"]) > 0)
