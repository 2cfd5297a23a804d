"""Run-time objective parameters of Levenberg-Marquardt and BFGS (nlsg_lm_create_params,
nlsg_bfgs_create_params) as far as the host decides them, before any device is touched: the new
entry points, the order and codes of the creators' checks, the LDS a shape needs beside its rows
(BFGS: four rows, one per wave of the search kernel's block), and the pairing of params= with a
parametrised objective in the drop-ins."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

LDS_BUDGET = 160 * 1024
TERMS = b"double r = xi - p(0); return p(1) * r * r + r / p(2);"
VECTOR = b"return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return r * r; });"
NEW = ("nlsg_lm_create_params", "nlsg_lm_set_params", "nlsg_lm_lds_bytes",
       "nlsg_bfgs_create_params", "nlsg_bfgs_set_params", "nlsg_bfgs_lds_bytes")
LM_REF, BFGS_REF, BFGS_SYM = _capi.LM_CHOLESKY_REFERENCE_ORDER, _capi.BFGS_REFERENCE_ORDER, _capi.BFGS_SYMMETRIC


def test_the_six_new_symbols_exist():
    lib = _capi.lib()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1], name
    assert lib.nlsg_abi_version() == 1


def lm_config(**kw):
    cfg = _capi.LMConfig()
    cfg.struct_size = C.sizeof(_capi.LMConfig)
    cfg.objective, cfg.solver = _capi.OBJ_CUSTOM, _capi.LM_CHOLESKY
    cfg.batch, cfg.m, cfg.n = 3, 0, 2
    cfg.lambda_, cfg.up, cfg.down, cfg.max_iter, cfg.f_delta = 10.0, 10.0, 10.0, 100, 1e-12
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def bfgs_config(**kw):
    cfg = _capi.BFGSConfig()
    cfg.struct_size = C.sizeof(_capi.BFGSConfig)
    cfg.objective = _capi.OBJ_CUSTOM
    cfg.batch, cfg.dim = 3, 2
    cfg.max_iter, cfg.grad_eps, cfg.alpha = 100, 5e-3, 1.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create(name, cfg, n_params, body=TERMS, chain=0):
    """(code, message) of a create call that must fail before the device is asked"""
    h = C.c_void_p()
    obj = _capi.CustomObjectiveC(body, b"return s;", chain, n_params)
    rc = getattr(_capi.lib(), name)(C.byref(cfg), C.byref(obj), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    assert rc != 0 and not h.value, name
    return rc, msg


def passes_the_host_checks(name, cfg, n_params):
    """a create call whose arguments are in order gets as far as the device: on a machine with one it
    succeeds (and the engine is destroyed), without one it answers "no device" (3)"""
    lib = _capi.lib()
    lib.nlsg_rtc_load(nlsolver_amd.de.rtc_library_path().encode())
    h = C.c_void_p()
    obj = _capi.CustomObjectiveC(TERMS, b"return s;", 0, n_params)
    rc = getattr(lib, name)(C.byref(cfg), C.byref(obj), C.byref(h))
    if rc == 0:
        getattr(lib, name.replace("create_params", "destroy"))(h)
    return rc in (0, 3)


def test_lm_create_params_checks_in_the_old_creators_order():
    name = "nlsg_lm_create_params"
    h = C.c_void_p()
    assert _capi.lib().nlsg_lm_create_params(None, None, C.byref(h)) == 1
    assert create(name, lm_config(objective=1), 3)[0] == 1            # cfg.objective must be custom
    assert create(name, lm_config(struct_size=3), 4097)[0] == 1       # struct_size first
    assert create(name, lm_config(solver=7), 4097)[0] == 1            # then the solver
    rc, msg = create(name, lm_config(solver=_capi.LM_QR), 4097)
    assert rc == 2 and "Cholesky" in msg
    rc, msg = create(name, lm_config(solver=LM_REF), 4097, VECTOR, 2)  # whole-vector body x reference order
    assert rc == 2 and "NLSG_LM_CHOLESKY_REFERENCE_ORDER" in msg
    assert create(name, lm_config(n=0), 4097)[0] == 1                 # then n and batch
    assert create(name, lm_config(batch=0), 4097)[0] == 1
    rc, msg = create(name, lm_config(n=1025), -1)                     # then the range
    assert rc == 2 and "1024" in msg
    # ... and only then n_params: zero is the old creator's, and the message says so
    for bad in (0, -1):
        rc, msg = create(name, lm_config(), bad)
        assert rc == 1 and "nlsg_lm_create_custom" in msg, bad
    for cfg in (lm_config(), lm_config(n=64, solver=LM_REF), lm_config(n=1024, solver=LM_REF)):
        rc, msg = create(name, cfg, 4097)
        assert rc == 2 and "4096" in msg and str(LDS_BUDGET) not in msg
    # every shape the engine takes has room for the largest row: the budget check cannot be reached
    # through create, so its arithmetic is pinned through fits() below
    L = nlsolver_amd.LMEngine
    assert all(L.fits(n, ref, 4096) for n in (1, 2, 64, 65, 1024) for ref in (False, True))


def test_bfgs_create_params_checks_in_the_old_creators_order():
    name = "nlsg_bfgs_create_params"
    h = C.c_void_p()
    assert _capi.lib().nlsg_bfgs_create_params(None, None, C.byref(h)) == 1
    assert create(name, bfgs_config(objective=1), 3)[0] == 1
    assert create(name, bfgs_config(struct_size=3), 4097)[0] == 1
    assert create(name, bfgs_config(dim=0), 4097)[0] == 1
    assert create(name, bfgs_config(batch=0), 4097)[0] == 1
    rc, msg = create(name, bfgs_config(dim=1025), -1)
    assert rc == 2 and "1024" in msg
    assert create(name, bfgs_config(flags=8), 4097)[0] == 1
    assert create(name, bfgs_config(flags=BFGS_REF | BFGS_SYM), 4097)[0] == 1
    rc, msg = create(name, bfgs_config(flags=BFGS_REF), 4097, VECTOR, 2)
    assert rc == 2 and "NLSG_BFGS_REFERENCE_ORDER" in msg
    for bad in (0, -1):
        rc, msg = create(name, bfgs_config(), bad)
        assert rc == 1 and "nlsg_bfgs_create_custom" in msg, bad
    rc, msg = create(name, bfgs_config(), 4097)
    assert rc == 2 and "4096" in msg
    rc, msg = create(name, bfgs_config(dim=1024, flags=BFGS_REF), 4097)   # the count before the budget
    assert rc == 2 and "4096" in msg and str(LDS_BUDGET) not in msg
    # the budget: four rows beside the reference-order buffers of eight chunks (64 KiB)
    rc, msg = create(name, bfgs_config(dim=1024, flags=BFGS_REF), 3073)
    assert rc == 2 and "163840" in msg and "3073" in msg and "65536" in msg
    assert "4 rows of 3073 parameters" in msg and str(4 * 8 * 3074) in msg   # (rows are rounded to an even count)
    rc, msg = create(name, bfgs_config(dim=513, flags=BFGS_REF), 4096)
    assert rc == 2 and "163840" in msg
    assert passes_the_host_checks(name, bfgs_config(dim=1024, flags=BFGS_REF), 3072)
    assert passes_the_host_checks(name, bfgs_config(dim=512, flags=BFGS_REF), 4096)
    assert passes_the_host_checks(name, bfgs_config(dim=1024), 4096)


def test_the_old_creators_still_reject_parameters():
    for name, cfg in (("nlsg_lm_create_custom", lm_config()), ("nlsg_bfgs_create_custom", bfgs_config())):
        for n_params in (1, -1, 4096):
            rc, msg = create(name, cfg, n_params)
            assert rc == 2 and "nlsg_de_batch_create_custom" in msg and "nlsg_pso_batch_create_custom" in msg, \
                (name, n_params)


def test_set_params_takes_no_null():
    lib = _capi.lib()
    assert lib.nlsg_lm_set_params(None, None) == 1
    assert lib.nlsg_bfgs_set_params(None, None) == 1


def test_lm_lds_bytes_agree_with_fits():
    f = _capi.lib().nlsg_lm_lds_bytes
    L = nlsolver_amd.LMEngine
    CH = _capi.LM_CHOLESKY
    assert [f(0, CH), f(1025, CH), f(2, _capi.LM_QR), f(2, 7)] == [0, 0, 0, 0]
    # n <= 64, either order: rows 0 .. n-1 of the packed triangle in chunks of 64 doubles | g | upd | x, 0 (66)
    for n, chunks in ((1, 1), (2, 1), (9, 1), (33, 10), (64, 33)):
        assert f(n, CH) == f(n, LM_REF) == 8 * (64 * chunks + 128 + 66), n
    # n > 64: nothing in tree order, xs[n + 2] | ts[n] | S[n] in reference order
    for n in (65, 130, 1024):
        assert f(n, CH) == 0 and f(n, LM_REF) == 8 * (3 * n + 2), n
    for n in (2, 64, 65, 1024):
        for ref in (False, True):
            need = f(n, LM_REF if ref else CH)
            assert L.lds_bytes(n, ref) == need
            assert L.lds_bytes(n, ref, 3) == need + 32 and L.lds_bytes(n, ref, 4096) == need + 32768
            assert L.fits(n, ref, 4096) and L.fits(n, ref, 0)
    assert not L.fits(0) and not L.fits(1025) and not L.fits(2, False, 4097) and not L.fits(2, False, -1)


def test_bfgs_lds_bytes_agree_with_fits():
    f = _capi.lib().nlsg_bfgs_lds_bytes
    Bf = nlsolver_amd.BFGSEngine
    assert [f(0, 0), f(1025, 0), f(2, 8), f(2, BFGS_REF | BFGS_SYM)] == [0, 0, 0, 0]
    # reference order: four waves x (xs | ts) x 128 doubles per chunk; tree order and the symmetric update: none
    for n, chunks in ((1, 1), (128, 1), (129, 2), (256, 2), (257, 4), (512, 4), (513, 8), (1024, 8)):
        assert f(n, BFGS_REF) == 4 * 2 * 128 * chunks * 8, n
        assert f(n, 0) == 0 and f(n, BFGS_SYM) == 0
        assert Bf.lds_bytes(n, True) == f(n, BFGS_REF) and Bf.lds_bytes(n) == 0
        assert Bf.lds_bytes(n, True, 3) == f(n, BFGS_REF) + 4 * 32 and Bf.lds_bytes(n, False, 4096) == 4 * 32768
        assert Bf.fits(n, False, 4096)
        assert Bf.fits(n, True, 4096) == (f(n, BFGS_REF) + 4 * 32768 <= LDS_BUDGET) == (n <= 512)
    # the edge the creator has: dim > 512 in reference order
    for n in (513, 600, 1024):
        most = max(k for k in range(1, 4097) if Bf.fits(n, True, k))
        assert most == 3072 and Bf.lds_bytes(n, True, most) == LDS_BUDGET
        assert not Bf.fits(n, True, 3073)
        rc, msg = create("nlsg_bfgs_create_params", bfgs_config(dim=n, flags=BFGS_REF), most + 1)
        assert rc == 2 and "163840" in msg
    assert not Bf.fits(0) and not Bf.fits(1025) and not Bf.fits(2, False, 4097) and not Bf.fits(2, False, -1)


def test_drop_ins_pair_params_with_a_parametrised_objective():
    obj = nlsolver_amd.CustomObjective("return xi * p(0);", n_params=1)
    for cls in (nlsolver_amd.BFGS, nlsolver_amd.LevenbergMarquardt):
        with pytest.raises(ValueError):
            cls(obj)                               # the objective needs its row
        with pytest.raises(ValueError):
            cls("rosenbrock", params=[1.0])
        with pytest.raises(ValueError):
            cls(obj, params=[1.0, 2.0])            # a row of another length
        assert cls(obj, params=[2.0]).params.shape == (1, 1)
        assert cls(obj, params=[[2.0], [3.0]]).params.shape == (2, 1)


def test_engines_refuse_rows_for_an_objective_without_parameters():
    """(host side of set_params: no device needed to say so)"""
    for cls in (nlsolver_amd.LMEngine, nlsolver_amd.BFGSEngine):
        eng = cls.__new__(cls)
        eng.n_params = 0
        with pytest.raises(nlsolver_amd.NlsgError) as ei:
            eng.set_params([[1.0]])
        assert ei.value.code == 1
