"""Run-time objective parameters (nlsg_custom_objective.n_params) as far as the host decides them,
before any device is touched: the LDS the row takes, how it enters the resident engines' budget,
the order and codes of create's checks, and the engines that take no parameters."""
import ctypes as C

import pytest

import nlsolver_amd
from nlsolver_amd import _capi

LDS_BUDGET = 160 * 1024
TERMS = b"double r = xi - p(0); return p(1) * r * r + r / p(2);"


def test_params_lds_bytes():
    f = _capi.lib().nlsg_custom_params_lds_bytes
    assert [f(n) for n in (0, -1, 4097)] == [0, 0, 0]
    assert [f(n) for n in (1, 2, 3, 4096)] == [16, 16, 32, 32768]
    assert _capi.CUSTOM_MAX_PARAMS == 4096


def test_the_parameters_count_against_the_lds_budget():
    DE, PSO = nlsolver_amd.DEBatchEngine, nlsolver_amd.PSOBatchEngine
    assert DE.lds_bytes(40, 2, 3) == DE.lds_bytes(40, 2) + 32
    assert PSO.lds_bytes(10, 2, nlsolver_amd.PSO_VANILLA, 3) == PSO.lds_bytes(10, 2) + 32
    assert DE.lds_bytes(40, 2, 4097) == 0 and DE.lds_bytes(3, 2, 3) == 0
    assert PSO.lds_bytes(10, 2, nlsolver_amd.PSO_VANILLA, 4097) == 0
    de = [(pop, 128) for pop in range(4, 1025) if DE.fits(pop, 128) and not DE.fits(pop, 128, 4096)]
    pso = [(n, 128) for n in range(1, 1025) if PSO.fits(n, 128) and not PSO.fits(n, 128, n_params=4096)]
    assert de and pso
    for pop, dim in de:
        assert DE.lds_bytes(pop, dim) <= LDS_BUDGET < DE.lds_bytes(pop, dim) + 32768
    assert DE.fits(de[0][0] - 1, 128, 4096) and PSO.fits(pso[0][0] - 1, 128, n_params=4096)


def custom(n_params):
    return _capi.CustomObjectiveC(TERMS, b"return s;", 0, n_params)


def de_config(**kw):
    cfg = _capi.DEBatchConfig()
    cfg.struct_size = C.sizeof(_capi.DEBatchConfig)
    cfg.objective, cfg.minimize, cfg.strategy = _capi.OBJ_CUSTOM, 1, 1
    cfg.batch, cfg.pop, cfg.dim = 3, 40, 2
    cfg.CR, cfg.F, cfg.eps = 0.9, 0.8, 10e-4
    cfg.max_iter, cfg.best_val_no_change = 1000, 50
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def pso_config(**kw):
    cfg = _capi.PSOBatchConfig()
    cfg.struct_size = C.sizeof(_capi.PSOBatchConfig)
    cfg.objective, cfg.minimize, cfg.type, cfg.bounded = _capi.OBJ_CUSTOM, 1, 0, 0
    cfg.batch, cfg.n_particles, cfg.dim = 3, 10, 2
    cfg.inertia, cfg.cognitive, cfg.social, cfg.eps = 0.8, 1.8, 1.8, 10e-4
    cfg.max_iter, cfg.best_val_no_change = 5000, 50
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def create(name, cfg, n_params):
    """(code, message) of a create_custom call that must fail before the device is asked"""
    h = C.c_void_p()
    obj = custom(n_params)
    rc = getattr(_capi.lib(), name)(C.byref(cfg), C.byref(obj), C.byref(h))
    msg = _capi.lib().nlsg_last_error().decode(errors="replace")
    assert rc != 0 and not h.value, name
    return rc, msg


def largest_that_fits(fits):
    return max(n for n in range(4, 1025) if fits(n))


def test_de_batch_create_custom_checks_n_params_in_its_place():
    name = "nlsg_de_batch_create_custom"
    assert create(name, de_config(), -1)[0] == 1
    rc, msg = create(name, de_config(), 4097)
    assert rc == 2 and "4096" in msg
    assert create(name, de_config(struct_size=3), 4097)[0] == 1   # struct_size first
    assert create(name, de_config(batch=0), 4097)[0] == 1         # then batch
    rc, msg = create(name, de_config(pop=2000), -1)               # then the ranges ...
    assert rc == 2 and "1024" in msg
    rc, msg = create(name, de_config(dim=129), -1)
    assert rc == 2 and "128" in msg
    assert create(name, de_config(pop=1024, dim=128), -1)[0] == 1  # ... and n_params before the budget
    rc, msg = create(name, de_config(pop=1024, dim=128), 4097)
    assert rc == 2 and "4096" in msg and str(LDS_BUDGET) not in msg
    pop = largest_that_fits(lambda n: nlsolver_amd.DEBatchEngine.fits(n, 128))
    rc, msg = create(name, de_config(pop=pop, dim=128), 4096)      # the budget includes the row
    assert rc == 2 and "163840" in msg and "4096" in msg
    rc, msg = create(name, de_config(pop=1024, dim=128), 0)        # as before without parameters
    assert rc == 2 and "163840" in msg


def test_pso_batch_create_custom_checks_n_params_in_its_place():
    name = "nlsg_pso_batch_create_custom"
    assert create(name, pso_config(), -1)[0] == 1
    rc, msg = create(name, pso_config(), 4097)
    assert rc == 2 and "4096" in msg
    assert create(name, pso_config(struct_size=3), 4097)[0] == 1
    assert create(name, pso_config(batch=0), 4097)[0] == 1
    assert create(name, pso_config(type=7), 4097)[0] == 1
    rc, msg = create(name, pso_config(n_particles=2000), -1)
    assert rc == 2 and "1024" in msg
    rc, msg = create(name, pso_config(dim=129), -1)
    assert rc == 2 and "128" in msg
    assert create(name, pso_config(n_particles=1024, dim=128), -1)[0] == 1
    for type_ in (nlsolver_amd.PSO_VANILLA, nlsolver_amd.PSO_ACCELERATED):
        n = largest_that_fits(lambda k: nlsolver_amd.PSOBatchEngine.fits(k, 128, type_))
        rc, msg = create(name, pso_config(n_particles=n, dim=128, type=type_), 4096)
        assert rc == 2 and "163840" in msg and "4096" in msg, type_
    rc, msg = create(name, pso_config(n_particles=1024, dim=128), 0)
    assert rc == 2 and "163840" in msg


OTHERS = [("nlsg_de_create_custom", _capi.DEConfig), ("nlsg_pso_create_custom", _capi.PSOConfig),
          ("nlsg_de_ref_create_custom", _capi.DERefConfig), ("nlsg_bfgs_create_custom", _capi.BFGSConfig),
          ("nlsg_lm_create_custom", _capi.LMConfig), ("nlsg_nm_create_custom", _capi.NMConfig),
          ("nlsg_sann_create_custom", _capi.SANNConfig), ("nlsg_nmpso_create_custom", _capi.NMPSOConfig)]


@pytest.mark.parametrize("name,config", OTHERS, ids=[n for n, _ in OTHERS])
def test_engines_without_parameters_reject_them_before_the_device(name, config):
    """code 2 on a machine with or without a GPU: the check sits among the argument checks"""
    cfg = config()
    cfg.struct_size = C.sizeof(config)
    cfg.objective = _capi.OBJ_CUSTOM
    for n_params in (1, -1, 4096):
        rc, msg = create(name, cfg, n_params)
        assert rc == 2, (name, n_params, msg)
        assert "nlsg_de_batch_create_custom" in msg and "nlsg_pso_batch_create_custom" in msg


def test_custom_objective_validates_n_params():
    assert nlsolver_amd.CustomObjective("return xi;").n_params == 0
    assert nlsolver_amd.CustomObjective("return xi * p(0);", n_params=1).n_params == 1
    assert nlsolver_amd.CustomObjective("return xi * p(0);", n_params=4096).n_params == 4096
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            nlsolver_amd.CustomObjective("return xi;", n_params=bad)
    # the positional construction the engines have always used
    obj = _capi.CustomObjectiveC(b"return xi;", b"return s;", 1, 0)
    assert (obj.chain, obj.n_params) == (1, 0)
    assert C.sizeof(_capi.CustomObjectiveC) == 24 and _capi.CustomObjectiveC.n_params.offset == 20


def test_drop_ins_pair_params_with_a_parametrised_objective():
    obj = nlsolver_amd.CustomObjective("return xi * p(0);", n_params=1)
    for cls in (nlsolver_amd.DE, nlsolver_amd.PSO):
        with pytest.raises(ValueError):
            cls(obj, None)                      # the objective needs its row
        with pytest.raises(ValueError):
            cls("rosenbrock", None, params=[1.0])
        assert cls(obj, None, params=[2.0]).params.shape == (1, 1)
    with pytest.raises(ValueError):
        nlsolver_amd.DE(obj, nlsolver_amd.XorShift(), generation="reference", params=[2.0])
