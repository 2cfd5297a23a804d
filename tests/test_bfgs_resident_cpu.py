"""NLSG_BFGS_RESIDENT on the host: the flag's checks, nlsg_bfgs_lds_bytes with it, the parameter budget
of one row, BFGSEngine.fits_resident / lds_bytes(resident=True) and the drop-in's driver=. No device:
every rejection comes before the device is asked, an accepted call gets as far as the device."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi
from nlsolver_amd.bfgs import BFGS, BFGSEngine

SYM, REF, RES = 1, 2, 4
KIB = 1024
ROW_4096 = 4096 * 8
TERMS = b"double r = xi - 1.0; return r * r;"
TERMS_P = b"double r = xi - 1.0; return r * r * p(0);"


def config(**kw):
    cfg = _capi.BFGSConfig()
    cfg.struct_size = C.sizeof(_capi.BFGSConfig)
    cfg.objective = _capi.OBJECTIVES["rosenbrock"]
    cfg.batch, cfg.dim = 3, 2
    cfg.max_iter, cfg.grad_eps, cfg.alpha = 100, 5e-3, 1.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg):
    """(code, message, made) of nlsg_bfgs_create on a built-in objective"""
    lib = _capi.lib()
    h = C.c_void_p()
    rc = lib.nlsg_bfgs_create(C.byref(cfg), None, None, C.byref(h))
    msg = lib.nlsg_last_error().decode(errors="replace")
    if rc == 0:
        lib.nlsg_bfgs_destroy(h)
    return rc, msg


def create_with_rows(name, cfg, n_params):
    lib = _capi.lib()
    lib.nlsg_rtc_load(nlsolver_amd.de.rtc_library_path().encode())
    h = C.c_void_p()
    obj = _capi.CustomObjectiveC(TERMS_P if n_params else TERMS, b"return s;", 0, n_params)
    rc = getattr(lib, name)(C.byref(cfg), C.byref(obj), C.byref(h))
    msg = lib.nlsg_last_error().decode(errors="replace")
    if rc == 0:
        lib.nlsg_bfgs_destroy(h)
    return rc, msg


def passes_the_host_checks(rc):
    """a call whose arguments are in order gets as far as the device: with one it succeeds, without one
    it answers "no device" (3)"""
    return rc in (0, 3)


def test_the_flag_is_4_and_needs_no_new_symbol():
    assert _capi.BFGS_RESIDENT == RES
    assert _capi.lib().nlsg_abi_version() == 1
    assert "nlsg_bfgs_resident" not in " ".join(_capi.SYMBOLS)
    assert BFGSEngine.has_resident()      # the probe: nlsg_bfgs_lds_bytes(2, NLSG_BFGS_RESIDENT) != 0


def test_flag_checks_come_before_the_device():
    assert create(config(flags=8))[0] == 1                      # still the unknown flag
    assert create(config(flags=8 | RES))[0] == 1
    rc, msg = create(config(flags=RES | SYM))
    assert rc == 1 and "NLSG_BFGS_RESIDENT" in msg
    assert create(config(flags=RES | SYM | REF))[0] == 1        # the older check of the two orders first
    rc, msg = create(config(flags=RES, dim=65))
    assert rc == 2 and "64" in msg and "NLSG_BFGS_RESIDENT" in msg
    rc, msg = create(config(flags=RES | REF, dim=65))
    assert rc == 2 and "64" in msg
    # older checks stay in their order: the shape before the flags
    assert create(config(flags=RES, dim=0))[0] == 1
    rc, msg = create(config(flags=RES, dim=1025))
    assert rc == 2 and "1024" in msg
    assert create(config(flags=RES | SYM, dim=65))[0] == 1      # the combination before the cap
    assert passes_the_host_checks(create(config(flags=RES, dim=64))[0])
    assert passes_the_host_checks(create(config(flags=RES | REF, dim=64))[0])
    assert passes_the_host_checks(create(config(flags=RES, dim=1))[0])


def test_lds_bytes_with_the_flag():
    f = _capi.lib().nlsg_bfgs_lds_bytes
    cap = 160 * KIB - ROW_4096
    for flags in (RES, RES | REF):
        assert 0 < f(64, flags) <= cap
        assert f(65, flags) == 0 and f(0, flags) == 0 and f(1024, flags) == 0
        sizes = [f(n, flags) for n in range(1, 65)]
        assert all(s > 0 for s in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        assert f(64, flags) >= 64 * 64 * 8                      # the matrix is in there
    assert f(8, RES | SYM) == 0 and f(8, RES | SYM | REF) == 0
    assert f(8, RES | 8) == 0
    # without the flag: what it was
    assert f(64, 0) == 0 and f(64, REF) == 8192 and f(1024, REF) == 65536 and f(8, SYM | REF) == 0


def test_the_parameter_budget_is_one_row():
    for flags in (RES, RES | REF):
        cfg = config(objective=_capi.OBJ_CUSTOM, flags=flags, dim=64)
        rc, msg = create_with_rows("nlsg_bfgs_create_params", cfg, 4096)
        assert passes_the_host_checks(rc), msg
        rc, msg = create_with_rows("nlsg_bfgs_create_params", cfg, 4097)
        assert rc == 2 and "4096" in msg
        rc, msg = create_with_rows("nlsg_bfgs_create_params", cfg, 0)
        assert rc == 1
        cfg = config(objective=_capi.OBJ_CUSTOM, flags=flags, dim=65)
        assert create_with_rows("nlsg_bfgs_create_params", cfg, 1)[0] == 2
        cfg = config(objective=_capi.OBJ_CUSTOM, flags=flags, dim=64)
        assert passes_the_host_checks(create_with_rows("nlsg_bfgs_create_custom", cfg, 0)[0])
        cfg = config(objective=_capi.OBJ_CUSTOM, flags=flags | SYM, dim=64)
        assert create_with_rows("nlsg_bfgs_create_custom", cfg, 0)[0] == 1
    # the whole block with its row stays inside the workgroup's LDS
    assert _capi.lib().nlsg_bfgs_lds_bytes(64, RES | REF) + ROW_4096 <= 160 * KIB


def test_fits_resident_agrees():
    f = _capi.lib().nlsg_bfgs_lds_bytes
    assert BFGSEngine.fits_resident(1) and BFGSEngine.fits_resident(64)
    assert BFGSEngine.fits_resident(64, n_params=4096)
    assert not BFGSEngine.fits_resident(65) and not BFGSEngine.fits_resident(0)
    assert not BFGSEngine.fits_resident(8, symmetric=True)
    assert not BFGSEngine.fits_resident(8, n_params=4097)
    assert not BFGSEngine.fits_resident(8, n_params=-1)
    for ref in (False, True):
        flags = RES | (REF if ref else 0)
        assert BFGSEngine.lds_bytes(64, ref, resident=True) == f(64, flags)
        assert BFGSEngine.lds_bytes(64, ref, 4096, resident=True) == f(64, flags) + ROW_4096
        assert BFGSEngine.lds_bytes(64, ref, 3, resident=True) == f(64, flags) + 32   # rows are 16-byte sized
        assert BFGSEngine.lds_bytes(65, ref, resident=True) == 0
    # the lock-step figures are what they were
    assert BFGSEngine.lds_bytes(64, True, 4096) == 8192 + 4 * ROW_4096
    assert BFGSEngine.lds_bytes(64) == 0


def test_driver_is_spelt_as_for_de_and_pso():
    assert BFGS("rosenbrock").driver == "turns"
    s = BFGS("rosenbrock", driver="resident")
    assert s.driver == "resident" and s.driver_used is None
    with pytest.raises(ValueError, match="driver must be 'turns' or 'resident'"):
        BFGS("rosenbrock", driver="resdient")
