"""The analytic gradient of a compiled objective for BFGS (nlsg_bfgs_create_gradient, CustomObjective
grad_body=, BFGSEngine gradient=) as far as the host decides it, before any device is touched: the new
optional symbol, the order and codes of the creator's checks, and the argument rules of the Python
classes."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

TERMS = b"double r = xi - 1.0; return r * r;"
TERMS_GRAD = b"return 2.0 * (xi - 1.0);"
VECTOR = b"return x.sum([](double v, uint64_t) { return v * v; });"
VECTOR_GRAD = b"return 2.0 * x(i);"
BFGS_REF, BFGS_SYM = _capi.BFGS_REFERENCE_ORDER, _capi.BFGS_SYMMETRIC
NAME = "nlsg_bfgs_create_gradient"


def config(**kw):
    cfg = _capi.BFGSConfig()
    cfg.struct_size = C.sizeof(_capi.BFGSConfig)
    cfg.objective = _capi.OBJ_CUSTOM
    cfg.batch, cfg.dim = 3, 2
    cfg.max_iter, cfg.grad_eps, cfg.alpha = 100, 5e-3, 1.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def gradient(body=TERMS_GRAD, struct_size=None):
    size = C.sizeof(_capi.BFGSGradientC) if struct_size is None else struct_size
    return _capi.BFGSGradientC(size, 0, body)


def create(cfg, n_params=0, grad=None, body=TERMS, chain=0):
    """(code, message) of a create call that must fail before the device is asked"""
    h = C.c_void_p()
    obj = _capi.CustomObjectiveC(body, b"return s;", chain, n_params)
    grad = gradient() if grad is None else grad
    rc = getattr(_capi.lib(), NAME)(C.byref(cfg), C.byref(obj), C.byref(grad), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    assert rc != 0 and not h.value
    return rc, msg


def passes_the_host_checks(cfg, n_params):
    """a call whose arguments are in order gets as far as the device: with one it succeeds (and the engine
    is destroyed), without one it answers "no device" (3)"""
    lib = _capi.lib()
    lib.nlsg_rtc_load(nlsolver_amd.de.rtc_library_path().encode())
    h = C.c_void_p()
    body = b"return 2.0 * (xi - 1.0) * p(0);" if n_params else TERMS_GRAD
    term = b"double r = xi - 1.0; return r * r * p(0);" if n_params else TERMS
    obj = _capi.CustomObjectiveC(term, b"return s;", 0, n_params)
    grad = gradient(body)
    rc = getattr(lib, NAME)(C.byref(cfg), C.byref(obj), C.byref(grad), C.byref(h))
    if rc == 0:
        lib.nlsg_bfgs_destroy(h)
    return rc in (0, 3)


def test_the_symbol_exists_with_its_argtypes():
    lib = _capi.lib()
    assert NAME in _capi.OPTIONAL_SYMBOLS and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _capi.SYMBOLS[NAME][1]
    assert getattr(lib, NAME).argtypes[2] == C.POINTER(_capi.BFGSGradientC)
    assert lib.nlsg_abi_version() == 1
    assert C.sizeof(_capi.BFGSGradientC) == 16
    assert C.sizeof(_capi.CustomObjectiveC) == 24      # the objective's struct did not grow


def test_the_creators_checks_and_their_codes():
    lib = _capi.lib()
    h = C.c_void_p()
    obj = _capi.CustomObjectiveC(TERMS, b"return s;", 0, 0)
    cfg, grad = config(), gradient()
    f = getattr(lib, NAME)
    assert f(None, C.byref(obj), C.byref(grad), C.byref(h)) == 1
    assert f(C.byref(cfg), None, C.byref(grad), C.byref(h)) == 1
    assert f(C.byref(cfg), C.byref(obj), None, C.byref(h)) == 1          # a null grad
    assert not h.value
    assert create(config(), grad=gradient(None))[0] == 1                 # a null body
    rc, msg = create(config(), grad=gradient(b""))                       # an empty one
    assert rc == 1 and "gradient body" in msg
    rc, msg = create(config(), grad=gradient(struct_size=8))
    assert rc == 1 and "nlsg_bfgs_gradient" in msg
    assert create(config(), grad=gradient(struct_size=24))[0] == 1
    assert create(config(objective=1))[0] == 1                           # cfg.objective must be custom
    # the old creator's checks, in its order
    assert create(config(struct_size=3), 4097)[0] == 1
    assert create(config(dim=0), 4097)[0] == 1
    assert create(config(batch=0), 4097)[0] == 1
    rc, msg = create(config(dim=1025), -1)
    assert rc == 2 and "1024" in msg
    assert create(config(flags=8), 4097)[0] == 1
    assert create(config(flags=BFGS_REF | BFGS_SYM), 4097)[0] == 1
    rc, msg = create(config(flags=BFGS_REF), 4097, gradient(VECTOR_GRAD), VECTOR, 2)
    assert rc == 2 and "NLSG_BFGS_REFERENCE_ORDER" in msg and "x.sum()" in msg   # today's message
    # ... then the parameters: none is fine here, a negative count invalid, too many unsupported
    rc, msg = create(config(), -1)
    assert rc == 1 and "-1" in msg
    rc, msg = create(config(), 4097)
    assert rc == 2 and "4096" in msg
    rc, msg = create(config(dim=1024, flags=BFGS_REF), 4097)             # the count before the budget
    assert rc == 2 and "4096" in msg and "163840" not in msg
    rc, msg = create(config(dim=1024, flags=BFGS_REF), 4096)             # four rows beside 64 KiB of buffers
    assert rc == 2 and "163840" in msg and "4 rows of 4096 parameters" in msg
    assert passes_the_host_checks(config(flags=BFGS_REF), 0)               # no parameters: accepted here
    assert passes_the_host_checks(config(dim=1024, flags=BFGS_REF), 3072)  # the most that fit beside the buffers


def test_the_old_creators_are_what_they_were():
    h = C.c_void_p()
    lib = _capi.lib()
    for n_params in (1, -1):
        obj = _capi.CustomObjectiveC(TERMS, b"return s;", 0, n_params)
        assert lib.nlsg_bfgs_create_custom(C.byref(config()), C.byref(obj), C.byref(h)) == 2
        assert "nlsg_de_batch_create_custom" in lib.nlsg_last_error().decode()
    obj = _capi.CustomObjectiveC(TERMS, b"return s;", 0, 0)
    assert lib.nlsg_bfgs_create_params(C.byref(config()), C.byref(obj), C.byref(h)) == 1
    assert "nlsg_bfgs_create_custom" in lib.nlsg_last_error().decode()


def test_custom_objective_takes_a_gradient_body():
    Obj = nlsolver_amd.CustomObjective
    assert Obj("return xi * xi;").grad_body is None
    o = Obj("return xi * xi;", grad_body="return 2.0 * xi;")
    assert o.grad_body == "return 2.0 * xi;" and o.n_params == 0 and o.chain == 0
    assert Obj(VECTOR.decode(), vector=True, grad_body=VECTOR_GRAD.decode(), n_params=3).chain == 2
    for bad in ("", "   ", b"return 2.0 * xi;", 3):
        with pytest.raises(ValueError):
            Obj("return xi * xi;", grad_body=bad)


def test_engine_and_drop_in_validate_the_gradient_choice():
    Obj, Eng = nlsolver_amd.CustomObjective, nlsolver_amd.BFGSEngine
    plain = Obj("return xi * xi;")
    with_grad = Obj("return xi * xi;", grad_body="return 2.0 * xi;")
    quad = nlsolver_amd.QuadDiagRank1([1.0, 2.0], [0.0, 0.0], 0.0)
    # all of these are decided before the library is asked for anything
    with pytest.raises(ValueError):
        Eng(plain, 2, dim=3, gradient="analytic")
    with pytest.raises(ValueError):
        Eng("sphere", 2, dim=3, gradient="analytic")
    with pytest.raises(ValueError):
        Eng(with_grad, 2, dim=3, gradient="numeric")
    with pytest.raises(ValueError):
        Eng(quad, 2, gradient="finite_difference")
    with pytest.raises(TypeError):
        Eng(with_grad, 2)                       # dim= is still needed
    B = nlsolver_amd.BFGS
    assert B(with_grad).gradient_used == "analytic"
    assert B(plain).gradient_used == "finite_difference"
    assert B("rosenbrock").gradient_used == "finite_difference"
    assert B(quad).gradient_used == "analytic"
    with pytest.raises(TypeError):
        B(with_grad, g=lambda x: x)             # g stays None-only
    # lds_bytes / fits do not depend on the gradient
    assert Eng.lds_bytes(130, True) == 4 * 2 * 128 * 2 * 8 and Eng.lds_bytes(130) == 0
    assert Eng.fits(1024, True, 3072) and not Eng.fits(1024, True, 3073)
