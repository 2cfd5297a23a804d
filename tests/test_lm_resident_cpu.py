"""NLSG_LM_RESIDENT at the library's doors: the capability query, every rejection of the flag with its code and
text, the order of the checks, and the binding's fits_resident / driver= — all before a device is touched."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nlsolver_amd
from nlsolver_amd import _capi
from tests import _engine_lifecycle as L

CH, QR, REF, RES = _capi.LM_CHOLESKY, _capi.LM_QR, _capi.LM_CHOLESKY_REFERENCE_ORDER, _capi.LM_RESIDENT
INVALID_ARG, UNSUPPORTED = 1, 2  # NLSG_ERR_INVALID_ARG, NLSG_ERR_UNSUPPORTED
DOORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_doors.json")

LINK = [_capi.LMLinkC(b"return 1.0 / (1.0 + det_exp(-z));", b"return v * (1.0 - v);")]
CURVE = L.ENGINES["lm_curve"][3]


def _create(symbol, cfg, extras):
    """(return code, nlsg_last_error) of a create that must fail before the device is touched"""
    lib = _capi.lib()
    h = C.c_void_p()
    rc = getattr(lib, symbol)(C.byref(cfg), *[C.byref(x) for x in extras], C.byref(h))
    assert not h.value
    return rc, lib.nlsg_last_error().decode(errors="replace")


def _with(cfg, **kw):
    c = type(cfg).from_buffer_copy(cfg)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_constants():
    assert _capi.LM_RESIDENT == 256 and _capi.LM_RESIDENT_CUT >= 1


def test_lds_bytes_with_the_flag():
    f = _capi.lib().nlsg_lm_lds_bytes
    assert [f(n, CH | RES) != 0 for n in (1, 2, 64)] == [True, True, True]
    assert [f(n, CH | RES) for n in (0, 65)] == [0, 0]
    # the flag with another solver, and other bits above the low byte, describe no workgroup
    assert [f(2, QR | RES), f(2, REF | RES), f(2, CH | 512), f(2, CH | RES | 512)] == [0, 0, 0, 0]
    assert nlsolver_amd.LMEngine.has_resident()


def test_lds_bytes_without_the_flag_are_the_recorded_ones():
    f = _capi.lib().nlsg_lm_lds_bytes
    with open(DOORS) as fh:
        doors = json.load(fh)["pure"]
    seen = 0
    for key, want in doors.items():
        if key.startswith("nlsg_lm_lds_bytes("):
            n, solver = (int(v) for v in key[len("nlsg_lm_lds_bytes("):-1].split(","))
            assert -1 <= solver <= 3
            assert f(n, solver) == want, key
            seen += 1
    assert seen >= 5 * 5


REJECTIONS = [
    # (case, create symbol, config, extras, code, a word of the rule)
    ("qr", "nlsg_lm_create", L.lm_cfg(), [], UNSUPPORTED, "QR"),
    ("qr_link", "nlsg_lm_create_link", L.lm_cfg(_capi.OBJ_LINK_REGRESSION), LINK, UNSUPPORTED, "QR"),
    ("qr_curve", "nlsg_lm_create_curve", L.lm_cfg(_capi.OBJ_CURVE_MODEL), CURVE, UNSUPPORTED, "QR"),
]


@pytest.mark.parametrize("case", REJECTIONS, ids=[c[0] for c in REJECTIONS])
def test_flag_with_qr(case):
    _, symbol, cfg, extras, code, word = case
    rc, text = _create(symbol, _with(cfg, solver=QR | RES), extras)
    assert rc == code and word in text and "NLSG_LM_RESIDENT" in text


def test_flag_with_reference_order():
    # a finite-difference objective is what takes the reference order; on a Gauss-Newton model the order is
    # refused by the check it always had, with or without the flag
    rc, text = _create("nlsg_lm_create", _with(L.lm_cfg(objective=0, m=0), solver=REF | RES), [])
    assert rc == UNSUPPORTED and "NLSG_LM_CHOLESKY_REFERENCE_ORDER" in text and "NLSG_LM_RESIDENT" in text
    plain = _create("nlsg_lm_create", _with(L.lm_cfg(), solver=REF), [])
    assert _create("nlsg_lm_create", _with(L.lm_cfg(), solver=REF | RES), []) == plain
    assert plain[0] == UNSUPPORTED and plain[1]


FD = [
    ("builtin", "nlsg_lm_create", L.lm_cfg(objective=0, m=0), []),
    ("custom", "nlsg_lm_create_custom", L.lm_cfg(_capi.OBJ_CUSTOM, m=0), [L._obj(L.GOOD)]),
    ("params", "nlsg_lm_create_params", L.lm_cfg(_capi.OBJ_CUSTOM, m=0), [L._obj(L.WITH_P, 1)]),
]


@pytest.mark.parametrize("case", FD, ids=[c[0] for c in FD])
def test_flag_with_a_finite_difference_objective(case):
    _, symbol, cfg, extras = case
    rc, text = _create(symbol, _with(cfg, solver=CH | RES), extras)
    assert rc == UNSUPPORTED and "finite-difference" in text and "NLSG_LM_RESIDENT" in text


def test_flag_past_64_parameters():
    rc, text = _create("nlsg_lm_create", _with(L.lm_cfg(m=66, n=65), solver=CH | RES), [])
    assert rc == UNSUPPORTED and "65" in text and "NLSG_LM_RESIDENT" in text
    rc, text = _create("nlsg_lm_create_link", _with(L.lm_cfg(_capi.OBJ_LINK_REGRESSION, m=66, n=65), solver=CH | RES),
                       LINK)
    assert rc == UNSUPPORTED and "65" in text and "NLSG_LM_RESIDENT" in text


@pytest.mark.parametrize("solver", [CH | 512, CH | RES | 512, CH | RES | 1024, QR | 4096, CH | (1 << 30)])
def test_unknown_bits(solver):
    for symbol, cfg, extras in (("nlsg_lm_create", L.lm_cfg(), []),
                                ("nlsg_lm_create_link", L.lm_cfg(_capi.OBJ_LINK_REGRESSION), LINK),
                                ("nlsg_lm_create_curve", L.lm_cfg(_capi.OBJ_CURVE_MODEL), CURVE),
                                ("nlsg_lm_create_custom", L.lm_cfg(_capi.OBJ_CUSTOM, m=0), [L._obj(L.GOOD)])):
        if symbol == "nlsg_lm_create_custom" and solver & 0xff == QR:
            continue  # (a finite-difference objective with QR is refused by the earlier rule)
        rc, text = _create(symbol, _with(cfg, solver=solver), extras)
        assert rc == INVALID_ARG and "256" in text, (symbol, text)


def test_earlier_checks_still_win():
    """what a shape or solver check answered without the flag it answers with it, word for word"""
    cases = [
        ("nlsg_lm_create", L.lm_cfg(m=0), []),                      # m = 0
        ("nlsg_lm_create", L.lm_cfg(n=0), []),                      # n = 0
        ("nlsg_lm_create", _with(L.lm_cfg(), batch=0), []),         # batch = 0
        ("nlsg_lm_create", L.lm_cfg(m=2000, n=1025), []),           # past the engine's n
        ("nlsg_lm_create", _with(L.lm_cfg(), struct_size=8), []),   # struct size
        ("nlsg_lm_create_curve", L.lm_cfg(_capi.OBJ_CURVE_MODEL, m=66, n=65), CURVE),  # a curve model's own n <= 64
        ("nlsg_lm_create_curve", L.lm_cfg(_capi.OBJ_CURVE_MODEL), [_capi.LMCurveC(b"r = y;", 17)]),  # k
        ("nlsg_lm_create_link", L.lm_cfg(_capi.OBJ_LINK_REGRESSION), [_capi.LMLinkC(b"", b"return 1.0;")]),
    ]
    for symbol, cfg, extras in cases:
        plain = _create(symbol, cfg, extras)
        assert plain[0] != 0 and plain[1]
        assert _create(symbol, _with(cfg, solver=cfg.solver | RES), extras) == plain, (symbol, plain)
    # an unknown solver in the low byte is named as that solver
    rc, text = _create("nlsg_lm_create", _with(L.lm_cfg(), solver=3 | RES), [])
    assert (rc, text) == _create("nlsg_lm_create", _with(L.lm_cfg(), solver=3), [])
    assert rc == INVALID_ARG and "unknown solver 3" in text
    # and a finite-difference objective with QR by the rule it always had
    plain = _create("nlsg_lm_create", _with(L.lm_cfg(objective=0, m=0), solver=QR), [])
    assert _create("nlsg_lm_create", _with(L.lm_cfg(objective=0, m=0), solver=QR | RES), []) == plain


def test_set_solver_on_a_null_engine_with_the_flag():
    lib = _capi.lib()
    assert lib.nlsg_lm_set_solver(None, CH | RES) == INVALID_ARG
    assert lib.nlsg_last_error()


def test_fits_resident_at_the_boundaries():
    fits = nlsolver_amd.LMEngine.fits_resident
    assert [fits(n) for n in (0, 1, 2, 64, 65, 1024)] == [False, True, True, True, False, False]
    assert not fits(3, QR) and not fits(3, REF) and fits(3, CH)
    assert not fits("rosenbrock") and not fits(True)
    assert not fits(nlsolver_amd.CustomObjective("return xi * xi;"))
    rng = np.random.default_rng(0)
    for n, want in ((64, True), (65, False)):
        model = nlsolver_amd.TanhRegression(rng.standard_normal((2, 3, n)), rng.standard_normal((2, 3)))
        assert fits(model) is want
        link = nlsolver_amd.LinkRegression.logistic(model.A, model.y)
        assert fits(link) is want and not fits(link, QR)
    t, y = rng.uniform(0, 1, (2, 5)), rng.standard_normal((2, 5))
    assert fits(nlsolver_amd.CurveModel.exp_decay(t, y))
    assert fits(nlsolver_amd.CurveModel(t, y, "r = y - th(0); J(0) = -1.0;", 64))
    assert not fits(nlsolver_amd.CurveModel(t, y, "r = y - th(0); J(0) = -1.0;", 65))


def test_unknown_driver_raises():
    model = nlsolver_amd.TanhRegression(np.zeros((1, 3, 2)), np.zeros((1, 3)))
    lm = nlsolver_amd.LevenbergMarquardt(model)
    assert lm.driver == "turns" and lm.driver_used is None
    with pytest.raises(ValueError):
        lm.with_driver("x")
    with pytest.raises(ValueError):
        lm.driver = "x"
    assert lm.driver == "turns"
    for driver in ("resident", "turns"):
        assert lm.with_driver(driver) is lm and lm.driver == driver and lm.driver_used is None


def test_drop_in_stays_with_turns_without_hiprtc(monkeypatch):
    """with_driver("resident") where nlsg_rtc_load fails: the engine is made without the flag, and with it
    where the load succeeds"""
    from nlsolver_amd import lm
    made = []

    class Made(Exception):
        pass

    class Engine:
        fits_resident = staticmethod(lambda *a: True)

        def __init__(self, f, **kw):
            made.append(kw["solver"])

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def minimize(self, x, params=None):
            raise Made

    class Lib:
        def __init__(self, rc):
            self.nlsg_rtc_load = lambda path: rc

    monkeypatch.setattr(lm, "LMEngine", Engine)
    model = nlsolver_amd.TanhRegression(np.zeros((1, 3, 2)), np.zeros((1, 3)))
    solver = nlsolver_amd.LevenbergMarquardt(model).with_driver("resident")
    for rc, want in ((UNSUPPORTED, CH), (0, CH | RES)):
        monkeypatch.setattr(lm, "lib", lambda rc=rc: Lib(rc))
        with pytest.raises(Made):
            solver.minimize(np.zeros(2))
        assert made[-1] == want
        assert solver.driver_used == ("resident" if want & RES else "turns")
