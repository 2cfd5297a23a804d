"""Levenberg-Marquardt regression models with a user-supplied link (nlsg_lm_create_link,
LinkRegression), as far as the host decides them before any device is touched: the entry point, the
order and codes of the creator's checks, the model class's argument handling.

Also used here: lm_link_solve (tests/_lm_planted.py), a numpy restatement of oracle/oracle_lm.c's order-0
loop (sequential sums, libm's functions: the arithmetic of the reference run) with the link as a
parameter. With tanh it must give what the oracle's own serial loop gives, within the bounds
tests/test_lm_gpu.py holds the device to against that loop (parameters 1e-12 absolute, f 1e-12 relative):
that makes it the yardstick of tests/test_lm_link_gpu.py for links the oracle does not have."""
import ctypes as C

import numpy as np
import pytest

import nlsolver_amd
from nlsolver_amd import _capi
from tests import _oracle as O
from tests._lm_planted import _gn_all, _update_with_hessian, lm_link_solve  # noqa: F401

SEED = 12374563468
LOGISTIC = (b"return 1.0 / (1.0 + det_exp(-z));", b"return v * (1.0 - v);")


# ---- the yardstick (tests/_lm_planted.py holds it now) ------------------------------------------------------
def np_tanh():
    return np.tanh, lambda z, v: 1 - v * v


def np_logistic():
    return (lambda z: 1.0 / (1.0 + np.exp(-z))), (lambda z, v: v * (1.0 - v))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_the_restatement_with_tanh_is_the_oracles_serial_loop(oracle, k):
    A, y, t0 = O.tanh_problem(oracle, SEED, 0, 48, 5)
    ref, xr, lam_r, _ = O.lm_solve(oracle, A, y, t0, order=0, lam=10.0, max_iter=k, f_delta=0.0)
    f, it, x, lam = lm_link_solve(A, y, t0, *np_tanh(), lam=10.0, max_iter=k, f_delta=0.0)
    print(f"max_iter {k}: |x - x_ref| {np.max(np.abs(x - xr)):.3e}, f rel {abs(f - ref.f_value) / ref.f_value:.3e}")
    assert it == ref.iteration == k and lam == lam_r
    assert np.max(np.abs(x - xr)) <= 1e-12
    assert abs(f - ref.f_value) <= 1e-12 * ref.f_value


# ---- the entry point ------------------------------------------------------------------------------------
def test_the_symbol_exists_with_its_argtypes():
    lib = _capi.lib()
    name = "nlsg_lm_create_link"
    assert name in _capi.SYMBOLS and name in _capi.OPTIONAL_SYMBOLS and hasattr(lib, name)
    assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]
    assert getattr(lib, name).argtypes[1] == C.POINTER(_capi.LMLinkC)
    assert _capi.require(name) is not None
    assert _capi.OBJ_LINK_REGRESSION == 33 and lib.nlsg_abi_version() == 1


def lm_config(**kw):
    cfg = _capi.LMConfig()
    cfg.struct_size = C.sizeof(_capi.LMConfig)
    cfg.objective, cfg.solver = _capi.OBJ_LINK_REGRESSION, _capi.LM_CHOLESKY
    cfg.batch, cfg.m, cfg.n = 3, 20, 5
    cfg.lambda_, cfg.up, cfg.down, cfg.max_iter, cfg.f_delta = 10.0, 10.0, 10.0, 100, 1e-12
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create_link(cfg, value=LOGISTIC[0], slope=LOGISTIC[1]):
    """(code, message) of a nlsg_lm_create_link call that must fail before the device is asked"""
    h = C.c_void_p()
    link = _capi.LMLinkC(value, slope)
    rc = _capi.lib().nlsg_lm_create_link(C.byref(cfg), C.byref(link), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    assert rc != 0 and not h.value
    return rc, msg


def test_the_creators_checks_fire_before_the_device():
    """(none of these answers 3, "no device": this test runs where there is none)"""
    lib = _capi.lib()
    h = C.c_void_p()
    link = _capi.LMLinkC(*LOGISTIC)
    assert lib.nlsg_lm_create_link(None, C.byref(link), C.byref(h)) == 1
    assert lib.nlsg_lm_create_link(C.byref(lm_config()), None, C.byref(h)) == 1
    for bad in (_capi.OBJ_TANH_REGRESSION, _capi.OBJ_CUSTOM, 0, 34):   # the objective id
        rc, msg = create_link(lm_config(objective=bad))
        assert rc == 1 and "NLSG_OBJ_LINK_REGRESSION" in msg, bad
    assert create_link(lm_config(struct_size=3))[0] == 1
    assert create_link(lm_config(solver=7))[0] == 1
    rc, msg = create_link(lm_config(solver=_capi.LM_CHOLESKY_REFERENCE_ORDER))
    assert rc == 2 and "NLSG_LM_CHOLESKY_REFERENCE_ORDER" in msg
    for kw in (dict(m=0), dict(n=0), dict(batch=0)):
        assert create_link(lm_config(**kw))[0] == 1, kw
    rc, msg = create_link(lm_config(n=1025, m=1100))
    assert rc == 2 and "1024" in msg
    rc, msg = create_link(lm_config(n=65, m=70, solver=_capi.LM_QR))
    assert rc == 2 and "64" in msg
    # the shape checks come before the bodies, as the issue orders them
    assert create_link(lm_config(n=1025, m=1100), None, None)[0] == 2
    for value, slope in ((None, LOGISTIC[1]), (LOGISTIC[0], None), (b"", LOGISTIC[1]), (LOGISTIC[0], b""),
                         (None, None)):
        rc, msg = create_link(lm_config(), value, slope)
        assert rc == 1 and "body" in msg, (value, slope)
        rc, msg = create_link(lm_config(n=64, m=70, solver=_capi.LM_QR), value, slope)
        assert rc == 1 and "body" in msg, (value, slope)


def test_the_plain_creator_names_the_new_one():
    h = C.c_void_p()
    rc = _capi.lib().nlsg_lm_create(C.byref(lm_config()), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    assert rc == 1 and not h.value and "nlsg_lm_create_link" in msg


# ---- the model class ------------------------------------------------------------------------------------
def test_link_regression_validates_its_arguments():
    L = nlsolver_amd.LinkRegression
    A, y = np.zeros((3, 20, 5)), np.zeros((3, 20))
    ok = L(A, y, "return z;", "return 1.0;")
    assert ok.A.shape == (3, 20, 5) and ok.nlsg_nlls_objective == 33
    one = L(A[0], y[0], "return z;", "return 1.0;")          # one problem: (m, n) and (m,)
    assert one.A.shape == (1, 20, 5) and one.y.shape == (1, 20)
    for bad_A, bad_y in ((A, y[:, :19]), (A, y[:2]), (A[0], y), (np.zeros(5), np.zeros(5)),
                         (np.zeros((2, 3, 20, 5)), np.zeros((2, 3, 20)))):
        with pytest.raises(ValueError):
            L(bad_A, bad_y, "return z;", "return 1.0;")
    for value, slope in (("", "return 1.0;"), ("return z;", "  "), (None, "return 1.0;"), (b"return z;", "return 1.0;")):
        with pytest.raises(TypeError):
            L(A, y, value, slope)


def test_call_needs_a_host_link():
    L = nlsolver_amd.LinkRegression
    rng = np.random.default_rng(3)
    A, y, th = rng.uniform(-1, 1, (2, 7, 3)), rng.uniform(0.1, 0.9, (2, 7)), rng.uniform(-1, 1, 3)
    with pytest.raises(TypeError):
        L(A, y, "return z;", "return 1.0;")(th)
    for make, phi in ((L.tanh, np.tanh), (L.logistic, lambda z: 1 / (1 + np.exp(-z))), (L.exp, np.exp),
                      (L.identity, lambda z: z)):
        model = make(A, y)
        assert isinstance(model, L) and model.value_body and model.slope_body
        r = y[1] - phi(A[1] @ th)
        assert model(th, problem=1) == pytest.approx(float(r @ r), rel=1e-15)
    tw = nlsolver_amd.TanhRegression(A, y)
    assert L.tanh(A, y)(th) == tw(th)
