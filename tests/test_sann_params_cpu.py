"""Run-time objective parameters of simulated annealing (nlsg_sann_create_params) as far as the host
decides them, before any device is touched: the new entry points, the order and codes of the
creator's checks, which layout a shape gets (several chains per wave with a row per lane group, or
one chain per wave) with the LDS it takes, and the pairing of params= with a parametrised objective
in the drop-in."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

LDS_BUDGET = 160 * 1024
TABLE = 4096  # the kernels' static logarithm table (rn_tab), next to the rows
TERMS = b"double r = xi - p(0); return p(1) * r * r + r / p(2);"
VECTOR = b"return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return r * r; });"
NEW = ("nlsg_sann_create_params", "nlsg_sann_set_params", "nlsg_sann_chains_per_wave", "nlsg_sann_lds_bytes")
DIMS = (2, 8, 9, 16, 33, 64, 65, 1025)


def test_the_new_symbols_exist():
    lib = _capi.lib()
    for name in NEW:
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1], name
    assert lib.nlsg_abi_version() == 1


def config(**kw):
    cfg = _capi.SANNConfig()
    cfg.struct_size = C.sizeof(_capi.SANNConfig)
    cfg.objective, cfg.minimize = _capi.OBJ_CUSTOM, 1
    cfg.batch, cfg.dim = 3, 2
    cfg.max_iter, cfg.temperature_iter, cfg.temperature_max, cfg.seed = 50, 10, 10.0, 1
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


def test_create_params_checks_in_the_old_creators_order():
    name = "nlsg_sann_create_params"
    h = C.c_void_p()
    assert _capi.lib().nlsg_sann_create_params(None, None, C.byref(h)) == 1
    assert create(name, config(objective=1), 3)[0] == 1             # cfg.objective must be custom
    assert create(name, config(struct_size=3), 4097)[0] == 1        # struct_size first
    assert create(name, config(dim=0), 4097)[0] == 1                # then dim and batch
    assert create(name, config(batch=0), 4097)[0] == 1
    rc, msg = create(name, config(dim=1025), -1, VECTOR, 2)         # then whole-vector bodies past 1024
    assert rc == 2 and "1024" in msg
    rc, msg = create(name, config(dim=1 << 32), 4097)               # then the ranges
    assert rc == 2 and "2^32" in msg
    rc, msg = create(name, config(batch=1 << 31), -1)
    assert rc == 2 and "batch" in msg
    # ... and only then n_params: zero is the old creator's, and the message says so
    for bad in (0, -1):
        for dim in (2, 65, 1025):
            rc, msg = create(name, config(dim=dim), bad)
            assert rc == 1 and "nlsg_sann_create_custom" in msg, (bad, dim)
    for dim in (2, 65, 1025):
        rc, msg = create(name, config(dim=dim), 4097)
        assert rc == 2 and "4096" in msg, dim


def test_the_old_creator_still_rejects_parameters():
    for n_params in (1, -1, 4096):
        rc, msg = create("nlsg_sann_create_custom", config(), n_params)
        assert rc == 2 and "nlsg_de_batch_create_custom" in msg, n_params


def test_set_params_takes_no_null():
    assert _capi.lib().nlsg_sann_set_params(None, None) == 1


def group_of(dim):
    """lanes per chain of the packed kernel, 0 past 64 coordinates"""
    return 4 if dim <= 8 else 8 if dim <= 16 else 16 if dim <= 32 else 32 if dim <= 64 else 0


def stride(n_params):
    """doubles between two lane groups' rows: the least count >= n_params that is 2 mod 4 -- even (16-byte
    rows), and its half odd, so 16 groups reading one k fall on 16 different bank pairs"""
    s = n_params
    while s % 4 != 2:
        s += 1
    return s


def group_rows_bytes(dim, n_params):
    return 4 * (64 // group_of(dim)) * 8 * stride(n_params)


def rule(dim, n_params):
    """(chains per wave, dynamic LDS bytes): the packed layout iff its rows fit beside the table"""
    if group_of(dim) and TABLE + group_rows_bytes(dim, n_params) <= LDS_BUDGET:
        return 64 // group_of(dim), group_rows_bytes(dim, n_params)
    return 1, 4 * 8 * (n_params + n_params % 2)


def test_the_stride_spreads_sixteen_groups_over_the_banks():
    for n in (1, 2, 3, 4, 5, 6, 7, 30, 31, 32, 33, 64, 310, 311, 4096):
        s = stride(n)
        assert n <= s <= n + 4 and s % 2 == 0 and s % 32 != 0
        assert len({(g * s) % 32 for g in range(16)}) == 16  # (bank pair of p(k) in group g: (k + g s) mod 32)


@pytest.mark.parametrize("dim", DIMS)
def test_chains_per_wave_and_lds_bytes_follow_the_rule(dim):
    S = nlsolver_amd.SANNEngine
    cpw, lds = S.chains_per_wave, S.lds_bytes
    assert cpw(dim) == cpw(dim, 0) == (64 // group_of(dim) if group_of(dim) else 1)
    assert lds(dim) == 0
    counts = [1, 4096]
    if group_of(dim):
        last = max(k for k in range(1, 4097) if TABLE + group_rows_bytes(dim, k) <= LDS_BUDGET)
        assert TABLE + group_rows_bytes(dim, last + 1) > LDS_BUDGET
        assert {4: 310, 8: 622, 16: 1246, 32: 2494}[group_of(dim)] == last
        counts += [last, last + 1]
    for n in counts:
        assert (cpw(dim, n), lds(dim, n)) == rule(dim, n), (dim, n)
        assert TABLE + lds(dim, n) <= LDS_BUDGET, (dim, n)       # every count fits at every dim
        # the two queries agree with each other: the bytes are the rows of the layout the other one names
        rows = 4 * cpw(dim, n) if cpw(dim, n) > 1 else 4
        assert lds(dim, n) == rows * 8 * (stride(n) if cpw(dim, n) > 1 else n + n % 2), (dim, n)
    if group_of(dim):
        assert cpw(dim, last) > 1 and cpw(dim, last + 1) == 1 and cpw(dim, 4096) == 1
    else:
        assert all(cpw(dim, n) == 1 for n in counts)


def test_the_queries_outside_their_ranges():
    f, g = _capi.lib().nlsg_sann_chains_per_wave, _capi.lib().nlsg_sann_lds_bytes
    assert [f(0, 0), f(2, -1), f(2, 4097)] == [0, 0, 0]
    assert [g(0, 1), g(2, 0), g(2, -1), g(2, 4097)] == [0, 0, 0, 0]


def test_drop_in_pairs_params_with_a_parametrised_objective():
    obj = nlsolver_amd.CustomObjective("return xi * p(0);", n_params=1)
    cls = nlsolver_amd.SANN
    with pytest.raises(ValueError):
        cls(obj)                               # the objective needs its row
    with pytest.raises(ValueError):
        cls("rosenbrock", params=[1.0])
    with pytest.raises(ValueError):
        cls(obj, params=[1.0, 2.0])            # a row of another length
    assert cls(obj, params=[2.0]).params.shape == (1, 1)
    assert cls(obj, params=[[2.0], [3.0]]).params.shape == (2, 1)
