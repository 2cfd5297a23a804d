"""Levenberg-Marquardt curve models (nlsg_lm_create_curve, nlsg_lm_set_curve_data, CurveModel), as far as
the host decides them before any device is touched: the entry points, the order and codes of the
creator's checks, the model class's argument handling.

Also here: lm_curve_solve, the serial numpy loop of tests/test_lm_link_cpu.py (lm_link_solve: sequential
sums in row order, the reference's solve) with a residual-and-Jacobian callable in place of the link. With
the tanh regression written as a curve model it must return lm_link_solve's bits: that makes it the
yardstick of tests/test_lm_curve_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import nlsolver_amd
from nlsolver_amd import _capi
from tests import _oracle as O
from tests.test_lm_link_cpu import _update_with_hessian, lm_link_solve, np_tanh

SEED = 12374563468
EXP_DECAY = (b"const double e = det_exp(-th(1) * t(0));\n"
             b"r = y - (th(0) * e + th(2));\n"
             b"J(0) = -e;  J(1) = th(0) * t(0) * e;  J(2) = -1.0;")


# ---- the yardstick --------------------------------------------------------------------------------------
def _gn_all(rj, t, y, x):
    """f = sum r^2, g = 2 J^T r, H = 2 J^T J: sums over the rows in row order (test_lm_link_cpu._gn_all)"""
    r, J = rj(t, y, x)
    n = x.size
    f, g, H = 0.0, np.zeros(n), np.zeros((n, n))
    for i in range(r.size):
        f += r[i] * r[i]
        g += J[i] * r[i]
        H += np.outer(J[i], J[i])
    return f, 2 * g, 2 * H


def lm_curve_solve(rj, t, y, x0, *, lam=10.0, up=10.0, down=10.0, max_iter=100, f_delta=1e-12):
    """lm_link_solve on r, J = rj(t, y, x): t (m, K), y (m,), x (n,) -> r (m,), J (m, n).
    Returns (f, iterations, x, final lambda)."""
    x = np.array(x0, dtype=np.float64)
    n = x.size
    cur, g, H = _gn_all(rj, t, y, x)
    prev, it = 0.0, 0
    while not (it >= max_iter or abs(prev - cur) < f_delta or np.isnan(prev)):
        H[np.arange(n), np.arange(n)] += lam
        x = x - _update_with_hessian(H, g)
        prev = cur
        cur, g, H = _gn_all(rj, t, y, x)
        it += 1
        lam = lam / down if cur < prev else lam * up
    return cur, it, x, lam


def rj_tanh_rows(t, y, x):
    """the tanh regression as a curve model: the observation's data are its row of A"""
    z = np.zeros(y.size)
    for j in range(x.size):
        z += t[:, j] * x[j]
    v = np.tanh(z)
    return y - v, -((1 - v * v)[:, None] * t)


def rj_exp_decay(t, y, x):
    e = np.exp(-x[1] * t[:, 0])
    return y - (x[0] * e + x[2]), np.stack([-e, x[0] * t[:, 0] * e, -np.ones_like(e)], axis=1)


def rj_gaussian_peak(t, y, x):
    u = (t[:, 0] - x[1]) / x[2]
    e = np.exp(-0.5 * (u * u))
    ae = x[0] * e
    return y - (ae + x[3]), np.stack([-e, -(ae * u / x[2]), -(ae * (u * u) / x[2]), -np.ones_like(e)], axis=1)


def rj_chebyshev_tanh(t, y, x):
    """r = y - tanh(sum_j x_j T_j(t)), the basis by recurrence"""
    A = chebyshev_basis(t[:, 0], x.size)
    return rj_tanh_rows(A, y, x)


def chebyshev_basis(t, n):
    """A_ij = T_j(t_i): T_0 = 1, T_1 = t, T_{j+1} = 2 t T_j - T_{j-1}"""
    A = np.empty((t.size, n))
    a, b = np.ones_like(t), t.copy()
    for j in range(n):
        A[:, j] = a
        a, b = b, 2.0 * t * b - a
    return A


@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_curve_loop_on_tanh_rows_is_the_link_loop(oracle, k):
    A, y, t0 = O.tanh_problem(oracle, SEED, 0, 48, 5)
    want = lm_link_solve(A, y, t0, *np_tanh(), lam=10.0, max_iter=k, f_delta=0.0)
    got = lm_curve_solve(rj_tanh_rows, A, y, t0, lam=10.0, max_iter=k, f_delta=0.0)
    assert got[1] == want[1] == k
    assert np.float64(got[0]).view(np.uint64) == np.float64(want[0]).view(np.uint64)
    assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
    assert got[3] == want[3]


@pytest.mark.parametrize("rj,x,K", [(rj_exp_decay, [2.0, 0.7, 0.5], 1), (rj_gaussian_peak, [1.5, 0.1, 0.8, 0.2], 1),
                                    (rj_chebyshev_tanh, [0.3, -0.2, 0.1, 0.25, -0.15], 1)],
                         ids=["exp_decay", "gaussian_peak", "chebyshev_tanh"])
def test_the_yardsticks_jacobians_are_the_residuals_derivatives(rj, x, K):
    """central differences of r at h = 1e-6: the truncation error is h^2 |r'''| / 6 ~ 1e-12, the rounding
    error eps |r| / h ~ 2e-10"""
    t = np.linspace(-0.9, 0.95, 11).reshape(-1, K)
    y = np.cos(3 * t[:, 0])
    x = np.array(x)
    _, J = rj(t, y, x)
    for j in range(x.size):
        d = np.zeros(x.size)
        d[j] = 1e-6
        fd = (rj(t, y, x + d)[0] - rj(t, y, x - d)[0]) / 2e-6
        assert np.max(np.abs(fd - J[:, j])) <= 5e-9, j


# ---- the entry points -----------------------------------------------------------------------------------
def test_the_symbols_exist_with_their_argtypes():
    lib = _capi.lib()
    for name in ("nlsg_lm_create_curve", "nlsg_lm_set_curve_data"):
        assert name in _capi.SYMBOLS and name in _capi.OPTIONAL_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
        assert _capi.require(name) is not None
    assert lib.nlsg_lm_create_curve.argtypes[1] == C.POINTER(_capi.LMCurveC)
    assert [f[0] for f in _capi.LMCurveC._fields_] == ["body", "k"]
    assert _capi.OBJ_CURVE_MODEL == 34 and lib.nlsg_abi_version() == 1


def lm_config(**kw):
    cfg = _capi.LMConfig()
    cfg.struct_size = C.sizeof(_capi.LMConfig)
    cfg.objective, cfg.solver = _capi.OBJ_CURVE_MODEL, _capi.LM_CHOLESKY
    cfg.batch, cfg.m, cfg.n = 3, 20, 3
    cfg.lambda_, cfg.up, cfg.down, cfg.max_iter, cfg.f_delta = 10.0, 10.0, 10.0, 100, 1e-12
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create_curve(cfg, body=EXP_DECAY, k=1):
    """(code, message) of a nlsg_lm_create_curve call that must fail before the device is asked"""
    h = C.c_void_p()
    curve = _capi.LMCurveC(body, k)
    rc = _capi.lib().nlsg_lm_create_curve(C.byref(cfg), C.byref(curve), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    assert rc != 0 and not h.value
    return rc, msg


def test_the_creators_checks_fire_before_the_device_in_their_order():
    """(none of these answers 3, "no device": this test runs where there is none.) Each call breaks one
    rule and every later one: the answer must be the first rule's."""
    lib = _capi.lib()
    h = C.c_void_p()
    curve = _capi.LMCurveC(EXP_DECAY, 1)
    assert lib.nlsg_lm_create_curve(None, C.byref(curve), C.byref(h)) == 1             # 1. null arguments
    assert lib.nlsg_lm_create_curve(C.byref(lm_config()), None, C.byref(h)) == 1
    assert lib.nlsg_lm_create_curve(C.byref(lm_config()), C.byref(curve), None) == 1
    later = dict(struct_size=3, solver=7, m=0, n=0, batch=0)
    for bad in (_capi.OBJ_TANH_REGRESSION, _capi.OBJ_LINK_REGRESSION, _capi.OBJ_CUSTOM, 0, 35):  # 2. the id
        rc, msg = create_curve(lm_config(objective=bad, **later), None, 0)
        assert rc == 1 and "NLSG_OBJ_CURVE_MODEL" in msg, bad
    del later["struct_size"]
    rc, msg = create_curve(lm_config(struct_size=3, **later), None, 0)                   # 3. the struct size
    assert rc == 1 and "size" in msg
    del later["solver"]
    rc, msg = create_curve(lm_config(solver=7, **later), None, 0)                        # 4. an unknown solver
    assert rc == 1 and "unknown solver" in msg
    rc, msg = create_curve(lm_config(solver=_capi.LM_CHOLESKY_REFERENCE_ORDER, **later), None, 0)  # 5.
    assert rc == 2 and "NLSG_LM_CHOLESKY_REFERENCE_ORDER" in msg
    for kw in (dict(m=0), dict(n=0), dict(batch=0)):                                     # 6. m, n, batch >= 1
        rc, msg = create_curve(lm_config(**kw), None, 0)
        assert rc == 1 and ">= 1" in msg, kw
    assert create_curve(lm_config(m=0, n=65), None, 0)[0] == 1
    for solver in (_capi.LM_CHOLESKY, _capi.LM_QR):                                      # 7. n > 64
        rc, msg = create_curve(lm_config(n=65, m=70, solver=solver), None, 0)
        assert rc == 2 and "one wave per problem" in msg, solver
    assert create_curve(lm_config(n=2000, m=70), None, 0)[0] == 2
    for k in (0, 17, 2 ** 31):                                                           # 8. k outside 1 .. 16
        rc, msg = create_curve(lm_config(), None, k)
        assert rc == 1 and "16" in msg, k
        rc, msg = create_curve(lm_config(n=64, m=1), EXP_DECAY, k)
        assert rc == 1 and "16" in msg, k
    for body in (None, b""):                                                             # 9. the body
        for k in (1, 16):
            rc, msg = create_curve(lm_config(), body, k)
            assert rc == 1 and "body" in msg, (body, k)


def test_the_other_creators_keep_rejecting_the_id():
    lib = _capi.lib()
    h = C.c_void_p()
    rc = lib.nlsg_lm_create(C.byref(lm_config()), C.byref(h))
    msg = lib.nlsg_last_error().decode(errors="replace")
    assert rc == 1 and not h.value and "nlsg_lm_create_curve" in msg
    link = _capi.LMLinkC(b"return z;", b"return 1.0;")
    rc = lib.nlsg_lm_create_link(C.byref(lm_config()), C.byref(link), C.byref(h))
    msg = lib.nlsg_last_error().decode(errors="replace")
    assert rc == 1 and not h.value and "NLSG_OBJ_LINK_REGRESSION" in msg


def test_set_curve_data_rejects_null_arguments():
    lib = _capi.lib()
    y = np.zeros(4)
    assert lib.nlsg_lm_set_curve_data(None, y.ctypes.data_as(_capi.pd), y.ctypes.data_as(_capi.pd)) == 1


# ---- the model class ------------------------------------------------------------------------------------
def test_curve_model_validates_its_arguments():
    M = nlsolver_amd.CurveModel
    t, y = np.zeros((3, 20, 2)), np.zeros((3, 20))
    ok = M(t, y, "r = y;", 4)
    assert ok.t.shape == (3, 20, 2) and ok.y.shape == (3, 20) and ok.n == 4 and ok.nlsg_nlls_objective == 34
    flat = M(t[:, :, 0], y, "r = y;", 1)                      # (batch, m): K = 1
    assert flat.t.shape == (3, 20, 1)
    one = M(t[0], y[0], "r = y;", 2)                          # one problem: (m, K) and (m,)
    assert one.t.shape == (1, 20, 2) and one.y.shape == (1, 20)
    one = M(t[0, :, 0], y[0], "r = y;", 2)                    # one problem: (m,) and (m,)
    assert one.t.shape == (1, 20, 1) and one.y.shape == (1, 20)
    for bad_t, bad_y in ((t, y[:, :19]), (t, y[:2]), (t[0], y), (np.zeros((2, 3, 20, 2)), np.zeros((2, 3, 20))),
                         (np.zeros((3, 20, 17)), y), (np.zeros((3, 20, 0)), y), (t, np.zeros(()))):
        with pytest.raises(ValueError):
            M(bad_t, bad_y, "r = y;", 2)
    for n in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            M(t, y, "r = y;", n)
    for body in ("", "  \n", None, b"r = y;"):
        with pytest.raises(TypeError):
            M(t, y, body, 2)


def test_call_needs_a_host_residual():
    M = nlsolver_amd.CurveModel
    rng = np.random.default_rng(3)
    t, y = rng.uniform(0.2, 2.0, (2, 9)), rng.uniform(0.1, 0.9, (2, 9))
    with pytest.raises(TypeError):
        M(t, y, "r = y;", 3)(np.ones(3))
    own = M(t, y, "r = y - th(0) * t(0);", 1, host=lambda th, t, y: y - th[0] * t[:, 0])
    r = y[1] - 0.5 * t[1]
    assert own([0.5], problem=1) == pytest.approx(float(r @ r), rel=1e-15)
    for make, rj, th in ((M.exp_decay, rj_exp_decay, [2.0, 0.7, 0.5]),
                         (M.gaussian_peak, rj_gaussian_peak, [1.5, 0.9, 0.8, 0.2])):
        model = make(t, y)
        assert isinstance(model, M) and model.body and model.n == len(th) and model.t.shape == (2, 9, 1)
        r = rj(t[1][:, None], y[1], np.array(th))[0]
        assert model(th, problem=1) == pytest.approx(float(r @ r), rel=1e-14)
    model = M.logistic4(t, y)
    a, b, c, d = th = [0.1, 2.0, 0.9, 1.1]
    r = y[0] - (d + (a - d) / (1.0 + (t[0] / c) ** b))
    assert model.n == 4 and model(th) == pytest.approx(float(r @ r), rel=1e-14)
