"""Run-time objective parameters of Nelder-Mead and the NM/PSO hybrid (nlsg_nm_create_params,
nlsg_nmpso_create_params) as far as the host decides them, before any device is touched: the new
entry points, the order and codes of the creators' checks, the LDS a shape needs beside its row, and
the pairing of params= with a parametrised objective in the drop-ins."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

LDS_BUDGET = 160 * 1024
TERMS = b"double r = xi - p(0); return p(1) * r * r + r / p(2);"
VECTOR = b"return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return r * r; });"
NEW = ("nlsg_nm_create_params", "nlsg_nm_set_params", "nlsg_nm_lds_bytes",
       "nlsg_nmpso_create_params", "nlsg_nmpso_set_params", "nlsg_nmpso_lds_bytes")
REF = _capi.NM_REFERENCE_ORDER


def test_the_six_new_symbols_exist():
    lib = _capi.lib()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1], name
    assert lib.nlsg_abi_version() == 1


def nm_config(**kw):
    cfg = _capi.NMConfig()
    cfg.struct_size = C.sizeof(_capi.NMConfig)
    cfg.objective, cfg.minimize = _capi.OBJ_CUSTOM, 1
    cfg.batch, cfg.dim = 3, 2
    cfg.step, cfg.alpha, cfg.gamma, cfg.rho, cfg.sigma, cfg.eps = -1.0, 1.0, 2.0, 0.5, 0.5, 1e-6
    cfg.max_iter, cfg.no_change_best_tol = 500, 20
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def hyb_config(**kw):
    cfg = _capi.NMPSOConfig()
    cfg.struct_size = C.sizeof(_capi.NMPSOConfig)
    cfg.objective, cfg.minimize = _capi.OBJ_CUSTOM, 1
    cfg.batch, cfg.dim = 3, 2
    cfg.alpha, cfg.gamma, cfg.rho, cfg.sigma = 1.0, 2.0, 0.5, 0.5
    cfg.inertia, cfg.cognitive, cfg.social, cfg.eps = 0.8, 1.8, 1.8, 1e-6
    cfg.max_iter, cfg.no_change_best_iter = 1000, 20
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


def test_nm_create_params_checks_in_the_old_creators_order():
    name = "nlsg_nm_create_params"
    h = C.c_void_p()
    assert _capi.lib().nlsg_nm_create_params(None, None, C.byref(h)) == 1
    assert create(name, nm_config(objective=1), 3)[0] == 1            # cfg.objective must be custom
    assert create(name, nm_config(struct_size=3), 4097)[0] == 1       # struct_size first
    assert create(name, nm_config(dim=0), 4097)[0] == 1               # then dim and batch
    assert create(name, nm_config(batch=0), 4097)[0] == 1
    rc, msg = create(name, nm_config(dim=1025), -1)                   # then the range
    assert rc == 2 and "1024" in msg
    assert create(name, nm_config(flags=4), 4097)[0] == 1             # then the flags
    rc, msg = create(name, nm_config(flags=REF), 4097, VECTOR, 2)     # whole-vector body x reference order
    assert rc == 2 and "NLSG_NM_REFERENCE_ORDER" in msg
    # ... and only then n_params: zero is the old creator's, and the message says so
    for bad in (0, -1):
        rc, msg = create(name, nm_config(), bad)
        assert rc == 1 and "nlsg_nm_create_custom" in msg, bad
    rc, msg = create(name, nm_config(), 4097)
    assert rc == 2 and "4096" in msg
    rc, msg = create(name, nm_config(dim=128), 4097)                  # the count before the budget
    assert rc == 2 and "4096" in msg and str(LDS_BUDGET) not in msg
    rc, msg = create(name, nm_config(dim=128), 4096)                  # the budget includes the row
    assert rc == 2 and "163840" in msg
    rc, msg = create(name, nm_config(dim=128, flags=REF), 4096)
    assert rc == 2 and "163840" in msg


def test_nmpso_create_params_checks_in_the_old_creators_order():
    name = "nlsg_nmpso_create_params"
    h = C.c_void_p()
    assert _capi.lib().nlsg_nmpso_create_params(None, None, C.byref(h)) == 1
    assert create(name, hyb_config(objective=1), 3)[0] == 1
    assert create(name, hyb_config(struct_size=3), 4097)[0] == 1
    assert create(name, hyb_config(batch=0), 4097)[0] == 1
    rc, msg = create(name, hyb_config(dim=1), 4097)
    assert rc == 1 and "one dimension" in msg
    rc, msg = create(name, hyb_config(dim=1025), -1)
    assert rc == 2 and "1024" in msg
    for bad in (0, -1):
        rc, msg = create(name, hyb_config(), bad)
        assert rc == 1 and "nlsg_nmpso_create_custom" in msg, bad
    rc, msg = create(name, hyb_config(), 4097)
    assert rc == 2 and "4096" in msg
    # every shape the hybrid takes has room for the largest row: the budget check cannot be reached
    # through create, so its arithmetic is pinned through fits() below
    H = nlsolver_amd.NMPSOEngine
    assert all(H.fits(n, 4096) for n in (2, 128, 129, 1024))


def test_the_old_creators_still_reject_parameters():
    for name, cfg in (("nlsg_nm_create_custom", nm_config()), ("nlsg_nmpso_create_custom", hyb_config())):
        for n_params in (1, -1, 4096):
            rc, msg = create(name, cfg, n_params)
            assert rc == 2 and "nlsg_de_batch_create_custom" in msg, (name, n_params)


def test_set_params_takes_no_null():
    lib = _capi.lib()
    assert lib.nlsg_nm_set_params(None, None) == 1
    assert lib.nlsg_nmpso_set_params(None, None) == 1


def test_nm_lds_bytes_agree_with_fits():
    f = _capi.lib().nlsg_nm_lds_bytes
    NM = nlsolver_amd.NMEngine
    assert [f(0, 0), f(1025, 0), f(2, 2), f(2, 3)] == [0, 0, 0, 0]
    # the n = 128 image: 129 x 128 vertices, 130 scores, 7 work vectors, control block, phase counters
    assert f(128, 0) == 140504
    # reference order: the image on a 16-byte boundary, ONE term buffer of 128 CHUNKS doubles, 64 bytes of read-ahead
    for n, chunks in ((2, 1), (9, 1), (128, 1), (130, 2), (1024, 8)):
        assert f(n, REF) == (f(n, 0) + 15) // 16 * 16 + 1024 * chunks + 64, n
        assert NM.lds_bytes(n) == f(n, 0) and NM.lds_bytes(n, True) == f(n, REF)
        assert NM.lds_bytes(n, False, 3) == f(n, 0) + 32 and NM.lds_bytes(n, True, 1) == f(n, REF) + 16
    assert NM.lds_bytes(0) == 0 and NM.lds_bytes(2, False, 4097) == 0 and not NM.fits(2, False, 4097)
    for ref in (False, True):
        need = f(128, REF if ref else 0)
        most = max(k for k in range(1, 4097) if NM.fits(128, ref, k))
        assert most % 2 == 0 and need + 8 * most <= LDS_BUDGET < need + 8 * (most + 2)
        assert not NM.fits(128, ref, most + 1)          # (odd counts are rounded up to even)
        # what fits() accepts create accepts, as far as a machine without a device can tell: the
        # first count it refuses is refused by create with the budget in the message
        rc, msg = create("nlsg_nm_create_params", nm_config(dim=128, flags=REF if ref else 0), most + 2)
        assert rc == 2 and "163840" in msg
    assert all(NM.fits(n, ref, 4096) for n in (2, 16, 64, 130, 1024) for ref in (False, True))


def test_nmpso_lds_bytes_agree_with_fits():
    f = _capi.lib().nlsg_nmpso_lds_bytes
    H = nlsolver_amd.NMPSOEngine
    assert [f(0), f(1), f(1025)] == [0, 0, 0]
    assert len({f(n) for n in (2, 9, 33, 128)}) == 1     # the packed kernel's block does not depend on n
    assert f(129) < f(130) < f(1024)                     # the wide kernels' view does
    for n in (2, 128, 130, 1024):
        assert H.lds_bytes(n) == f(n) and H.lds_bytes(n, 3) == f(n) + 32 and H.lds_bytes(n, 4096) == f(n) + 32768
        assert H.fits(n, 4096) == (f(n) + 32768 <= LDS_BUDGET)
    assert H.lds_bytes(1) == 0 and H.lds_bytes(2, 4097) == 0 and not H.fits(2, 4097)


def test_drop_ins_pair_params_with_a_parametrised_objective():
    obj = nlsolver_amd.CustomObjective("return xi * p(0);", n_params=1)
    for cls in (nlsolver_amd.NelderMead, nlsolver_amd.NelderMeadPSO):
        with pytest.raises(ValueError):
            cls(obj)                               # the objective needs its row
        with pytest.raises(ValueError):
            cls("rosenbrock", params=[1.0])
        with pytest.raises(ValueError):
            cls(obj, params=[1.0, 2.0])            # a row of another length
        assert cls(obj, params=[2.0]).params.shape == (1, 1)
        assert cls(obj, params=[[2.0], [3.0]]).params.shape == (2, 1)
