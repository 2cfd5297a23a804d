"""What the resident batch PSO engine decides on the host, before any device is touched: the LDS
need it publishes, the order of create's checks, and the drop-in class's `driver` argument."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

LDS_BUDGET = 160 * 1024
VANILLA, ACCELERATED = 0, 1


def lds(n, dim, type_):
    return nlsolver_amd.PSOBatchEngine.lds_bytes(n, dim, type_)


@pytest.mark.parametrize("type_", [VANILLA, ACCELERATED])
def test_lds_bytes_is_zero_outside_the_ranges_and_monotone_inside(type_):
    for n, dim in [(0, 2), (1025, 2), (10, 0), (10, 129), (0, 0), (2 ** 40, 2), (10, 2 ** 40),
                   (2 ** 63, 2 ** 63)]:
        assert lds(n, dim, type_) == 0, (n, dim)
    for n, dim in [(1, 1), (10, 2), (1024, 1), (1, 128), (1024, 128)]:
        assert lds(n, dim, type_) > 0, (n, dim)
    for dim in (1, 2, 7, 8, 64, 65, 128):
        col = [lds(n, dim, type_) for n in range(1, 1025)]
        assert all(a < b for a, b in zip(col, col[1:])), dim
    for n in (1, 10, 1024):
        row = [lds(n, dim, type_) for dim in range(1, 129)]
        assert all(a <= b for a, b in zip(row, row[1:])), n
        assert row[0] < row[-1]
    # never below the rows' own bytes: positions, and for Vanilla velocities and personal bests too
    arrays = 3 if type_ == VANILLA else 1
    for n in (1, 10, 255, 1024):
        for dim in (1, 2, 9, 64, 65, 128):
            assert lds(n, dim, type_) >= arrays * n * dim * 8, (n, dim)


def test_lds_bytes_of_an_unknown_type_is_zero():
    assert lds(10, 2, 2) == 0 and lds(10, 2, -1) == 0


def test_which_shapes_fit_a_workgroup():
    fits = nlsolver_amd.PSOBatchEngine.fits
    for n, dim, type_ in [(10, 2, VANILLA), (10, 2, ACCELERATED), (1024, 8, ACCELERATED), (512, 8, VANILLA),
                          (120, 128, ACCELERATED), (40, 128, VANILLA)]:
        assert 0 < lds(n, dim, type_) <= LDS_BUDGET and fits(n, dim, type_), (n, dim, type_)
    for n, dim, type_ in [(1024, 8, VANILLA), (1024, 128, ACCELERATED)]:
        assert lds(n, dim, type_) > LDS_BUDGET and not fits(n, dim, type_), (n, dim, type_)
    assert 3 * 1024 * 8 * 8 == 192 * 1024  # Vanilla 1024 x 8: the rows alone


def config(**kw):
    cfg = _capi.PSOBatchConfig()
    cfg.struct_size = C.sizeof(_capi.PSOBatchConfig)
    cfg.objective, cfg.minimize, cfg.type, cfg.bounded = 0, 1, ACCELERATED, 0
    cfg.batch, cfg.n_particles, cfg.dim = 3, 10, 2
    cfg.inertia, cfg.cognitive, cfg.social, cfg.eps = 0.8, 1.8, 1.8, 10e-4
    cfg.max_iter, cfg.best_val_no_change = 5000, 50
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create(cfg):
    h = C.c_void_p()
    rc = _capi.lib().nlsg_pso_batch_create(C.byref(cfg), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    if rc == 0:
        _capi.lib().nlsg_pso_batch_destroy(h)
    return rc, msg


def test_create_checks_the_request_before_the_device():
    assert _capi.lib().nlsg_pso_batch_create(None, None) == 1
    assert create(config(struct_size=3))[0] == 1
    assert create(config(struct_size=3, n_particles=2000))[0] == 1  # struct_size is looked at first
    assert create(config(batch=0, n_particles=2000))[0] == 1         # then batch,
    assert create(config(batch=0, type=7))[0] == 1
    rc, msg = create(config(type=7, n_particles=2000))                # then the type (still code 1),
    assert rc == 1 and "type" in msg
    rc, msg = create(config(n_particles=2000))                        # then the ranges (code 2)
    assert rc == 2 and "1024" in msg
    assert create(config(n_particles=0))[0] == 2
    rc, msg = create(config(dim=129))
    assert rc == 2 and "128" in msg
    assert create(config(dim=0))[0] == 2
    rc, msg = create(config(n_particles=1024, dim=128))               # then the LDS budget
    assert rc == 2 and str(LDS_BUDGET) in msg
    rc, msg = create(config(n_particles=1024, dim=8, type=VANILLA))
    assert rc == 2 and str(LDS_BUDGET) in msg


def test_a_valid_request_needs_a_device():
    if _capi.lib().nlsg_device_count() > 0:
        assert create(config())[0] == 0
    else:
        assert create(config())[0] == 3


def test_config_mirrors_the_header():
    # nlsg_pso_config without shard_lo, shard_n and seed, plus batch and turns_per_launch
    assert C.sizeof(_capi.PSOBatchConfig) == C.sizeof(_capi.PSOConfig) - 3 * 8 + 2 * 8


def test_drop_in_driver_argument_is_validated():
    with pytest.raises(ValueError):
        nlsolver_amd.PSO("rosenbrock", None, driver="bogus")
    assert nlsolver_amd.PSO("rosenbrock", None).driver == "turns"
    assert nlsolver_amd.PSO("rosenbrock", None, driver="resident").driver == "resident"
    assert nlsolver_amd.PSO("rosenbrock", None).driver_used is None
