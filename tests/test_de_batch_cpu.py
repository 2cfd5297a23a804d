"""What the resident batch DE engine decides on the host, before any device is touched: the LDS
need it publishes, the order of create's checks, and the drop-in class's `driver` argument."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

LDS_BUDGET = 160 * 1024


def lds(pop, dim):
    return nlsolver_amd.DEBatchEngine.lds_bytes(pop, dim)


def test_lds_bytes_is_zero_outside_the_ranges_and_monotone_inside():
    for pop, dim in [(3, 2), (1025, 2), (40, 0), (40, 129), (0, 0), (2 ** 40, 2), (40, 2 ** 40)]:
        assert lds(pop, dim) == 0, (pop, dim)
    for pop, dim in [(4, 1), (40, 2), (1024, 1), (4, 128), (1024, 128)]:
        assert lds(pop, dim) > 0, (pop, dim)
    for dim in (1, 2, 7, 8, 64, 65, 128):
        col = [lds(pop, dim) for pop in range(4, 1025)]
        assert all(a < b for a, b in zip(col, col[1:])), dim
    for pop in (4, 40, 1024):
        row = [lds(pop, dim) for dim in range(1, 129)]
        assert all(a <= b for a, b in zip(row, row[1:])), pop
    for pop, dim in [(40, 2), (1024, 8), (70, 128)]:
        assert 0 < lds(pop, dim) <= LDS_BUDGET, (pop, dim)
    # two fp64 buffers of pop x dim rows alone are within the need
    assert lds(1024, 8) >= 2 * 8 * 1024 * 8


def config(**kw):
    cfg = _capi.DEBatchConfig()
    cfg.struct_size = C.sizeof(_capi.DEBatchConfig)
    cfg.objective, cfg.minimize, cfg.strategy = 0, 1, 1
    cfg.batch, cfg.pop, cfg.dim = 3, 40, 2
    cfg.CR, cfg.F, cfg.eps = 0.9, 0.8, 10e-4
    cfg.max_iter, cfg.best_val_no_change = 1000, 50
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg):
    h = C.c_void_p()
    rc = _capi.lib().nlsg_de_batch_create(C.byref(cfg), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    if rc == 0:
        _capi.lib().nlsg_de_batch_destroy(h)
    return rc, msg


def test_create_checks_the_request_before_the_device():
    assert create(config(struct_size=3))[0] == 1
    assert create(config(struct_size=3, pop=2000))[0] == 1  # struct_size is looked at first
    assert create(config(batch=0, pop=2000))[0] == 1         # then batch, then the ranges
    rc, msg = create(config(pop=2000))
    assert rc == 2 and "1024" in msg
    rc, msg = create(config(dim=129))
    assert rc == 2 and "128" in msg
    rc, msg = create(config(pop=1024, dim=128))
    assert rc == 2 and str(LDS_BUDGET) in msg
    assert _capi.lib().nlsg_de_batch_create(None, None) == 1


def test_a_valid_request_needs_a_device():
    if _capi.lib().nlsg_device_count() > 0:
        assert create(config())[0] == 0
    else:
        assert create(config())[0] == 3


def test_drop_in_driver_argument_is_validated():
    with pytest.raises(ValueError):
        nlsolver_amd.DE("rosenbrock", None, driver="bogus")
    with pytest.raises(ValueError):
        nlsolver_amd.DE("rosenbrock", nlsolver_amd.XorShift(), driver="resident", generation="reference")
    assert nlsolver_amd.DE("rosenbrock", None).driver == "turns"
    assert nlsolver_amd.DE("rosenbrock", None, driver="resident").driver == "resident"
