"""The resident Levenberg-Marquardt driver (NLSG_LM_RESIDENT) against the lock-step engine of the same
configuration, bit for bit: theta, every byte of every Status, and lambda_out, compared as uint64. The
lock-step engine is pinned to the oracle by test_lm_gpu, test_lm_link_gpu, test_lm_curve_gpu and
test_lm_planted_gpu, so it is the yardstick here.

Inputs: batch 6, the start of problem b at distance SPREAD[b] (1e-9 .. 6; curve models CLOSE[b], 1e-9 .. 1) from
the planted optimum, so that problems stop at different iterations. The damping schedule (lambda 10, divided by
10 per accepted step) makes most starts of one model take nearly the same number of iterations, so the two ends
are made to differ by construction: problem 0 has noise-free data and starts 1e-9 from its optimum, f(x0) is
below f_delta and the first stop test fires (0 iterations); the last regression start lies 6 away, in the
saturated part of the link. Every case that runs to convergence asserts that the iteration counts
of its batch are not all equal and that some problem ran two iterations or more. The cases whose stop rule
pins the count (max_iter 0 / 1 / 3, f_delta = 1e300, f_delta = 0, the launch cut) cannot have unequal counts
among their finite problems; they assert the count the rule gives instead. Every case checks that the
lock-step result is finite, except for the problem that is about NaN.

Source bodies compiled here: the logistic link, and three curve bodies (exponential decay, a polynomial, a
decay with a per-problem constant as second datum)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 6
SPREAD = np.array([1e-9, 1e-3, 1e-2, 0.1, 1.0, 6.0])
CLOSE = np.array([1e-9, 1e-3, 1e-2, 0.1, 0.4, 1.0])  # relative, for the curve models' positive parameters
NOISE = 0.01 * np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0])[:, None]
POLY = ("double pw = 1.0, s = 0.0;\n"
        "for (int j = 0; j < n; j++) { s += th(j) * pw; J(j) = -pw; pw = pw * t(0); }\n"
        "r = y - s;")
DECAY_K2 = ("const double e = det_exp(-th(1) * t(0));\n"
            "r = y - (th(0) * e + t(1));\n"
            "J(0) = -e;  J(1) = th(0) * t(0) * e;")


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    assert nlsolver_amd.LMEngine.has_resident()
    return nlsolver_amd


def bits(result):
    theta, st, lam = result
    return (np.ascontiguousarray(theta).view(np.uint64).copy(),
            np.frombuffer(b"".join(bytes(s) for s in st), dtype=np.uint64).copy(),
            np.ascontiguousarray(lam).view(np.uint64).copy())


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def assert_same(a, b, what=""):
    for name, x, y in zip(("theta", "status", "lambda"), bits(a), bits(b)):
        assert np.array_equal(x, y), f"{what}: {name} differs at {np.flatnonzero(x != y)[:8]}"


def iterations(result):
    return [s.iteration for s in result[1]]


def finite(result, but=()):
    theta, st, lam = result
    keep = [b for b in range(len(st)) if b not in but]
    return bool(np.isfinite(theta[keep]).all() and np.isfinite(lam[keep]).all()
                and all(np.isfinite(st[b].f_value) for b in keep))


def solve(mod, model, x0, resident, **kw):
    from nlsolver_amd import _capi
    kw["solver"] = kw.get("solver", _capi.LM_CHOLESKY) | (_capi.LM_RESIDENT if resident else 0)
    with mod.LMEngine(model, **kw) as eng:
        assert eng.driver == ("resident" if resident else "turns")
        return eng.minimize(x0.copy())


def both(mod, model, x0, converges=True, nan=(), **kw):
    """the lock-step result, after checking that the resident one has its bits"""
    turns = solve(mod, model, x0, False, **kw)
    assert finite(turns, nan), "the lock-step engine left non-finite values: the case's data are wrong"
    assert_same(solve(mod, model, x0, True, **kw), turns)
    if converges:
        it = iterations(turns)
        assert len(set(it)) > 1 and max(it) >= 2, it
    return turns


def regression(n, m, seed, link="tanh"):
    """A (B, m, n), y (B, m), and the starts x0 (B, n) at SPREAD from the planted theta"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, m, n)) / np.sqrt(n)
    star = rng.uniform(-1, 1, (B, n))
    z = np.einsum("bmn,bn->bm", A, star)
    y = (np.tanh(z) if link == "tanh" else 1 / (1 + np.exp(-z))) + NOISE * rng.uniform(-1, 1, (B, m))
    x0 = star + SPREAD[:, None] * rng.uniform(-1, 1, (B, n))
    return A, y, x0


def decay(m, seed):
    rng = np.random.default_rng(seed)
    t = np.tile(np.linspace(0.0, 4.0, m) if m > 1 else np.array([1.0]), (B, 1))
    star = np.stack([2 + 0.25 * np.arange(B), 0.7 + 0.1 * np.arange(B), np.full(B, 0.5)], axis=1)
    y = star[:, :1] * np.exp(-star[:, 1:2] * t) + star[:, 2:] + NOISE * rng.uniform(-1, 1, (B, m))
    x0 = star * (1 + CLOSE[:, None] * np.array([-0.3, 0.4, -0.2]))
    return t, y, x0


# ---- 1. tanh regression ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 63, 64])
def test_tanh_by_n(mod, n):
    A, y, x0 = regression(n, 17, 100 + n)
    both(mod, mod.TanhRegression(A, y), x0)


@pytest.mark.parametrize("m", [1, 16, 17, 64, 65])
def test_tanh_by_m(mod, m):
    A, y, x0 = regression(3, m, 200 + m)
    both(mod, mod.TanhRegression(A, y), x0)


# ---- 2. a link with phi(0) != 0: the masked-row path ----------------------------------------------------
@pytest.mark.parametrize("n", [3, 64])
def test_logistic_link(mod, n):
    A, y, x0 = regression(n, 17, 300 + n, link="logistic")
    both(mod, mod.LinkRegression.logistic(A, y), x0)


# ---- 3. curve models ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 129])
def test_curve_exp_decay(mod, m):
    t, y, x0 = decay(m, 400 + m)
    both(mod, mod.CurveModel.exp_decay(t, y), x0)


@pytest.mark.parametrize("n", [17, 33, 64])
def test_curve_polynomial(mod, n):
    m = 70
    rng = np.random.default_rng(500 + n)
    t = np.tile(np.linspace(-1.0, 1.0, m), (B, 1))
    star = rng.uniform(-1, 1, (B, n))
    y = np.einsum("bmj,bj->bm", t[:, :, None] ** np.arange(n), star) + NOISE * rng.uniform(-1, 1, (B, m))
    x0 = star + CLOSE[:, None] * rng.uniform(-1, 1, (B, n))
    # (the power basis is ill conditioned: the damping stays within 2^-30 .. 2^30 of 1, and the matrix definite)
    both(mod, mod.CurveModel(t, y, POLY, n), x0, lam=1.0, up=2.0, down=2.0, max_iter=30)


def test_curve_two_data(mod):
    m = 40
    rng = np.random.default_rng(600)
    offset = 0.2 + 0.1 * np.arange(B)
    star = np.stack([2 + 0.25 * np.arange(B), 0.7 + 0.1 * np.arange(B)], axis=1)
    tt = np.tile(np.linspace(0.0, 4.0, m), (B, 1))
    t = np.stack([tt, np.broadcast_to(offset[:, None], (B, m))], axis=2)  # the constant rides in column 1
    y = star[:, :1] * np.exp(-star[:, 1:2] * tt) + offset[:, None] + NOISE * rng.uniform(-1, 1, (B, m))
    x0 = star * (1 + CLOSE[:, None] * np.array([-0.3, 0.4]))
    both(mod, mod.CurveModel(t, y, DECAY_K2, 2), x0)


# ---- 4. stop rules --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return regression(3, 17, 700)


@pytest.mark.parametrize("max_iter", [0, 1, 3])
def test_max_iter(mod, small, max_iter):
    A, y, x0 = small
    turns = both(mod, mod.TanhRegression(A, y), x0, converges=False, max_iter=max_iter)
    assert max(iterations(turns)) == max_iter


def test_first_test_fires(mod, small):
    A, y, x0 = small
    turns = both(mod, mod.TanhRegression(A, y), x0, converges=False, f_delta=1e300)
    assert iterations(turns) == [0] * B


def test_runs_to_the_limit(mod, small):
    A, y, x0 = small
    turns = both(mod, mod.TanhRegression(A, y), x0, converges=False, f_delta=0.0, max_iter=40)
    assert iterations(turns) == [40] * B


def test_nan_and_zero_column(mod, small):
    A, y, x0 = (v.copy() for v in small)
    y[2, 5] = np.nan      # problem 2: f is NaN from the first evaluation on
    A[4, :, 1] = 0.0      # problem 4: a zero column, J^T J is singular
    turns = both(mod, mod.TanhRegression(A, y), x0, nan=(2,))
    assert np.isnan(turns[1][2].f_value)
    clean = solve(mod, mod.TanhRegression(*small[:2]), small[2], False)
    for b in (0, 1, 3, 5):  # the neighbours are what they are without the two
        assert np.array_equal(turns[0][b].view(np.uint64), clean[0][b].view(np.uint64))
        assert bytes(turns[1][b])[:64] == bytes(clean[1][b])[:64]


# ---- 5. the launch cut ----------------------------------------------------------------------------------
def test_launch_cut(mod):
    from nlsolver_amd import _capi
    cap = _capi.LM_RESIDENT_CUT
    A, y, x0 = regression(2, 4, 800)
    model = mod.TanhRegression(A, y)
    for max_iter in (cap - 1, cap, cap + 1, 2 * cap + 1):
        # (a constant damping: nothing overflows however long the loop runs)
        turns = both(mod, model, x0, converges=False, f_delta=0.0, max_iter=max_iter, lam=1e-3, up=1.0, down=1.0)
        assert iterations(turns) == [max_iter] * B


# ---- 6. one engine, drivers switched --------------------------------------------------------------------
def test_switching_one_engine(mod):
    from nlsolver_amd import _capi
    from nlsolver_amd._engine import pd_of
    CH, RES = _capi.LM_CHOLESKY, _capi.LM_RESIDENT
    A, y, x0 = regression(3, 17, 900)
    A2, y2, x2 = regression(3, 17, 901)
    model = mod.TanhRegression(A, y)
    fresh = solve(mod, model, x0, True)
    fresh_qr = solve(mod, model, x0, False, solver=_capi.LM_QR)
    with mod.LMEngine(model) as eng:
        turns = eng.minimize(x0.copy())
        assert finite(turns) and len(set(iterations(turns))) > 1 and max(iterations(turns)) >= 2
        assert_same(fresh, turns, "fresh resident engine")
        for k, solver in enumerate((CH | RES, CH, CH | RES)):
            eng.set_solver(solver)
            assert eng.driver == ("resident" if solver & RES else "turns")
            assert_same(eng.minimize(x0.copy()), turns, f"switch {k}")
        # other data in between: nothing of them survives
        assert _capi.lib().nlsg_lm_set_data(eng._h, pd_of(A2), pd_of(y2)) == 0
        other = eng.minimize(x2.copy())
        assert_same(other, solve(mod, mod.TanhRegression(A2, y2), x2, False), "second data set")
        assert not same(other, turns)
        assert _capi.lib().nlsg_lm_set_data(eng._h, pd_of(A), pd_of(y)) == 0
        assert_same(eng.minimize(x0.copy()), fresh, "after other data")
        eng.set_solver(_capi.LM_QR)
        assert eng.driver == "turns"
        assert_same(eng.minimize(x0.copy()), fresh_qr, "QR after resident")


def test_switching_a_curve_engine(mod):
    from nlsolver_amd import _capi
    from nlsolver_amd._engine import pd_of
    t, y, x0 = decay(64, 950)
    t2, y2, x2 = decay(64, 951)
    fresh = solve(mod, mod.CurveModel.exp_decay(t, y), x0, False)
    with mod.LMEngine(mod.CurveModel.exp_decay(t2, y2), solver=_capi.LM_CHOLESKY | _capi.LM_RESIDENT) as eng:
        eng.minimize(x2.copy())
        set_data = _capi.lib().nlsg_lm_set_curve_data
        assert set_data(eng._h, pd_of(np.ascontiguousarray(t[:, :, None])), pd_of(y)) == 0
        assert_same(eng.minimize(x0.copy()), fresh, "resident after other curve data")
        eng.set_solver(_capi.LM_CHOLESKY)
        assert_same(eng.minimize(x0.copy()), fresh, "turns on the same engine")


# ---- 7. covariance --------------------------------------------------------------------------------------
def test_covariance_after_a_resident_solve(mod):
    t, y, x0 = decay(64, 1000)
    model = mod.CurveModel.exp_decay(t, y)
    from nlsolver_amd import _capi
    with mod.LMEngine(model, solver=_capi.LM_CHOLESKY | _capi.LM_RESIDENT) as res, mod.LMEngine(model) as turns:
        assert (res.driver, turns.driver) == ("resident", "turns")
        theta, _, _ = res.minimize(x0.copy())
        got, want = res.covariance(theta), turns.covariance(theta)
        assert got[2].all() and np.isfinite(got[0]).all()
        for a, b in zip(got, want):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        # and the engine still solves afterwards
        assert_same(res.minimize(x0.copy()), turns.minimize(x0.copy()))


# ---- 8. the drop-in -------------------------------------------------------------------------------------
def test_drop_in(mod):
    t, y, x0 = decay(64, 1100)
    for x, model in ((x0[3].copy(), mod.CurveModel.exp_decay(t[3], y[3])), (x0.copy(), mod.CurveModel.exp_decay(t, y))):
        xa, xb = x.copy(), x.copy()
        a = mod.LevenbergMarquardt(model).with_driver("resident")
        b = mod.LevenbergMarquardt(model).with_driver("turns")
        sa, sb = a.minimize(xa), b.minimize(xb)
        assert (a.driver_used, b.driver_used) == ("resident", "turns")
        assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64))
        assert np.array_equal(a.lambdas.view(np.uint64), b.lambdas.view(np.uint64))
        la, lb = (sa, sb) if x.ndim == 2 else ([sa], [sb])
        assert [bytes(s) for s in la] == [bytes(s) for s in lb]
        assert np.isfinite(xa).all()


def test_drop_in_falls_back_past_64(mod):
    rng = np.random.default_rng(1200)
    A = rng.standard_normal((2, 70, 65)) / 8
    y = np.tanh(np.einsum("bmn,bn->bm", A, rng.uniform(-1, 1, (2, 65))))
    x0 = rng.uniform(-0.1, 0.1, (2, 65))
    xa, xb = x0.copy(), x0.copy()
    a = mod.LevenbergMarquardt(mod.TanhRegression(A, y), max_iter=5).with_driver("resident")
    b = mod.LevenbergMarquardt(mod.TanhRegression(A, y), max_iter=5)
    sa, sb = a.minimize(xa), b.minimize(xb)
    assert (a.driver_used, b.driver_used) == ("turns", "turns")
    assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64))
    assert [bytes(s) for s in sa] == [bytes(s) for s in sb]
