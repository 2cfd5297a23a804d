"""Create / destroy cases of every engine kind at its smallest shape that still allocates every
conditional block, driven through the C-ABI only. Shared by tests/test_engine_lifecycle_gpu.py and
scripts/record_engine_cached_bytes.py, which wrote tests/golden/engine_cached_bytes.json: the test
compares what the pool parks (nlsg_cached_bytes) and what nlsg_last_error says with that record,
never with anything computed from the library under test."""
import ctypes as C
import json
import os

import numpy as np

from nlsolver_amd import _capi as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_cached_bytes.json")

GOOD = b"return xi * xi;"
BAD = b"return xi +;"  # an ordinary compile error of the run-time compiler: no kernel runs
WITH_P = b"double r = xi - p(0); return r * r;"


def _cfg(cls, **kw):
    c = cls()
    c.struct_size = C.sizeof(cls)
    c.device = 0
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _obj(body, n_params=0):
    return A.CustomObjectiveC(body, b"return s;", 0, n_params)


_DE = dict(minimize=1, strategy=A.DE_RANDOM, CR=0.9, F=0.8, eps=1e-3, max_iter=10, best_val_no_change=50)
_PSO = dict(minimize=1, type=A.PSO_VANILLA, bounded=0, inertia=0.7, cognitive=1.5, social=1.5, eps=1e-3,
            max_iter=10, best_val_no_change=50)
_LM = dict(solver=A.LM_CHOLESKY, batch=2, lambda_=1e-3, up=10.0, down=0.1, max_iter=10, f_delta=1e-8)
_NM = dict(minimize=1, bounded=0, flags=0, batch=2, step=1.0, alpha=1.0, gamma=2.0, rho=0.5, sigma=0.5,
           eps=1e-6, max_iter=10, no_change_best_tol=10, restarts=0)
_HYB = dict(minimize=1, bounded=0, batch=2, dim=2, inst_lo=0, alpha=1.0, gamma=2.0, rho=0.5, sigma=0.5,
            inertia=0.7, cognitive=1.5, social=1.5, eps=1e-6, max_iter=10, no_change_best_iter=10, seed=1)
_SANN = dict(minimize=1, batch=2, chain_lo=0, max_iter=10, temperature_iter=10, temperature_max=10.0, seed=1)
_BFGS = dict(batch=2, dim=2, max_iter=10, grad_eps=1e-6, alpha=1.0, quad_c=0.0)


def de_cfg(objective=0):  # trace: the trace and counter blocks
    return _cfg(A.DEConfig, objective=objective, trace=1, pop=8, dim=2, shard_lo=0, shard_n=8, seed=1, **_DE)


def de_ref_cfg(objective=0, dim=2, log=2):  # log: the two log blocks
    return _cfg(A.DERefConfig, objective=objective, batch=2, pop=4, dim=dim, log_capacity=log, **_DE)


def de_batch_cfg(objective=0):
    return _cfg(A.DEBatchConfig, objective=objective, batch=2, pop=4, dim=2, turns_per_launch=0, **_DE)


def pso_cfg(objective=0):  # Vanilla: velocities and personal-best rows
    return _cfg(A.PSOConfig, objective=objective, n_particles=4, dim=2, shard_lo=0, shard_n=4, seed=1, **_PSO)


def pso_batch_cfg(objective=0):
    return _cfg(A.PSOBatchConfig, objective=objective, batch=2, n_particles=4, dim=2, turns_per_launch=0, **_PSO)


def bfgs_cfg(objective=0, flags=0):
    return _cfg(A.BFGSConfig, objective=objective, flags=flags, **_BFGS)


def lm_cfg(objective=A.OBJ_TANH_REGRESSION, m=3, n=2):
    return _cfg(A.LMConfig, objective=objective, m=m, n=n, **_LM)


def nm_cfg(objective=0, dim=2):
    return _cfg(A.NMConfig, objective=objective, dim=dim, **_NM)


def nmpso_cfg(objective=0):
    return _cfg(A.NMPSOConfig, objective=objective, **_HYB)


def sann_cfg(objective=0, dim=2):
    return _cfg(A.SANNConfig, objective=objective, dim=dim, **_SANN)


# name -> (create symbol, destroy symbol, config, what goes between the config and the handle)
ENGINES = {
    "de": ("nlsg_de_create", "nlsg_de_destroy", de_cfg(), []),
    "de_ref": ("nlsg_de_ref_create", "nlsg_de_ref_destroy", de_ref_cfg(), []),
    # a population past what a workgroup's LDS holds: the trial rows in global memory
    "de_ref_spill": ("nlsg_de_ref_create", "nlsg_de_ref_destroy", de_ref_cfg(dim=8192, log=0), []),
    "de_batch": ("nlsg_de_batch_create", "nlsg_de_batch_destroy", de_batch_cfg(), []),
    "pso": ("nlsg_pso_create", "nlsg_pso_destroy", pso_cfg(), []),
    "pso_batch": ("nlsg_pso_batch_create", "nlsg_pso_batch_destroy", pso_batch_cfg(), []),
    "bfgs": ("nlsg_bfgs_create", "nlsg_bfgs_destroy", bfgs_cfg(), [None, None]),
    "bfgs_symmetric": ("nlsg_bfgs_create", "nlsg_bfgs_destroy", bfgs_cfg(flags=A.BFGS_SYMMETRIC), [None, None]),
    "lm": ("nlsg_lm_create", "nlsg_lm_destroy", lm_cfg(), []),
    "lm_wide": ("nlsg_lm_create", "nlsg_lm_destroy", lm_cfg(m=66, n=65), []),
    "lm_objective": ("nlsg_lm_create", "nlsg_lm_destroy", lm_cfg(objective=0, m=0), []),
    "lm_curve": ("nlsg_lm_create_curve", "nlsg_lm_destroy", lm_cfg(objective=A.OBJ_CURVE_MODEL),
                 [A.LMCurveC(b"r = y - th(0) * t(0) - th(1); J(0) = -t(0); J(1) = -1.0;", 1)]),
    "nm": ("nlsg_nm_create", "nlsg_nm_destroy", nm_cfg(), []),
    "nm_wide": ("nlsg_nm_create", "nlsg_nm_destroy", nm_cfg(dim=129), []),  # the simplexes in global memory
    "nmpso": ("nlsg_nmpso_create", "nlsg_nmpso_destroy", nmpso_cfg(), []),
    "sann": ("nlsg_sann_create", "nlsg_sann_destroy", sann_cfg(), []),
    "sann_long": ("nlsg_sann_create", "nlsg_sann_destroy", sann_cfg(dim=1025), []),  # the trial rows
    # one engine with parameters per kind that has them, n_params = 1
    "de_batch_params": ("nlsg_de_batch_create_custom", "nlsg_de_batch_destroy", de_batch_cfg(A.OBJ_CUSTOM),
                        [_obj(WITH_P, 1)]),
    "pso_batch_params": ("nlsg_pso_batch_create_custom", "nlsg_pso_batch_destroy", pso_batch_cfg(A.OBJ_CUSTOM),
                         [_obj(WITH_P, 1)]),
    "bfgs_params": ("nlsg_bfgs_create_params", "nlsg_bfgs_destroy", bfgs_cfg(A.OBJ_CUSTOM), [_obj(WITH_P, 1)]),
    "lm_params": ("nlsg_lm_create_params", "nlsg_lm_destroy", lm_cfg(A.OBJ_CUSTOM, m=0), [_obj(WITH_P, 1)]),
    "nm_params": ("nlsg_nm_create_params", "nlsg_nm_destroy", nm_cfg(A.OBJ_CUSTOM), [_obj(WITH_P, 1)]),
    "nmpso_params": ("nlsg_nmpso_create_params", "nlsg_nmpso_destroy", nmpso_cfg(A.OBJ_CUSTOM), [_obj(WITH_P, 1)]),
    "sann_params": ("nlsg_sann_create_params", "nlsg_sann_destroy", sann_cfg(A.OBJ_CUSTOM), [_obj(WITH_P, 1)]),
}

# a create that fails after its allocations, one engine of each kind that compiles at run time:
# name -> (create symbol, config, arguments, the good case whose cycle follows it)
RTC_FAILURES = {
    "de": ("nlsg_de_create_custom", de_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "de"),
    "de_ref": ("nlsg_de_ref_create_custom", de_ref_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "de_ref"),
    "de_batch": ("nlsg_de_batch_create_custom", de_batch_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "de_batch"),
    "pso": ("nlsg_pso_create_custom", pso_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "pso"),
    "pso_batch": ("nlsg_pso_batch_create_custom", pso_batch_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "pso_batch"),
    "bfgs": ("nlsg_bfgs_create_custom", bfgs_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "bfgs"),
    "lm": ("nlsg_lm_create_custom", lm_cfg(A.OBJ_CUSTOM, m=0), [_obj(BAD)], "lm_objective"),
    "lm_curve": ("nlsg_lm_create_curve", lm_cfg(A.OBJ_CURVE_MODEL), [A.LMCurveC(b"r = y +;", 1)], "lm_curve"),
    "lm_link": ("nlsg_lm_create_link", lm_cfg(A.OBJ_LINK_REGRESSION), [A.LMLinkC(b"return z +;", b"return 1.0;")],
                "lm"),
    "nm": ("nlsg_nm_create_custom", nm_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "nm"),
    "nmpso": ("nlsg_nmpso_create_custom", nmpso_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "nmpso"),
    "sann": ("nlsg_sann_create_custom", sann_cfg(A.OBJ_CUSTOM), [_obj(BAD)], "sann"),
}

# kind -> (engine with parameters, engine of the kind without, set_params symbol)
PARAM_KINDS = {
    "de_batch": ("de_batch_params", "de_batch", "nlsg_de_batch_set_params"),
    "pso_batch": ("pso_batch_params", "pso_batch", "nlsg_pso_batch_set_params"),
    "bfgs": ("bfgs_params", "bfgs", "nlsg_bfgs_set_params"),
    "lm": ("lm_params", "lm_objective", "nlsg_lm_set_params"),
    "nm": ("nm_params", "nm", "nlsg_nm_set_params"),
    "nmpso": ("nmpso_params", "nmpso", "nlsg_nmpso_set_params"),
    "sann": ("sann_params", "sann", "nlsg_sann_set_params"),
}


def _call_create(lib, symbol, cfg, args):
    h = C.c_void_p()
    rc = A.require(symbol)(C.byref(cfg), *[C.byref(a) if isinstance(a, C.Structure) else a for a in args],
                           C.byref(h))
    return rc, h


def create(lib, name):
    symbol, _, cfg, args = ENGINES[name]
    rc, h = _call_create(lib, symbol, cfg, args)
    assert rc == 0 and h.value, (name, rc, last_error(lib))
    return h


def destroy(lib, name, h):
    assert A.require(ENGINES[name][1])(h) == 0


def last_error(lib):
    return lib.nlsg_last_error().decode(errors="replace")


def emptied(lib):
    lib.nlsg_release_cached()
    assert lib.nlsg_cached_bytes() == 0


def cycle(lib, name):
    """one create and destroy; the bytes the pool parks afterwards"""
    destroy(lib, name, create(lib, name))
    return int(lib.nlsg_cached_bytes())


def failed_create(lib, name):
    """(error code, bytes parked) of a create whose run-time compilation fails"""
    symbol, cfg, args, _ = RTC_FAILURES[name]
    rc, h = _call_create(lib, symbol, cfg, args)
    assert not h.value
    return int(rc), int(lib.nlsg_cached_bytes())


def nm_phase_cycle(lib):
    """an NM engine that ran nlsg_nm_phase_cycles (its phase buffer exists from then on), destroyed"""
    h = create(lib, "nm")
    x0 = np.full((2, 2), 0.5)
    out = np.zeros((2, 8), dtype=np.uint64)
    rc = lib.nlsg_nm_phase_cycles(h, x0.ctypes.data_as(A.pd), out.ctypes.data_as(A.pu))
    assert rc == 0, last_error(lib)
    destroy(lib, "nm", h)
    return int(lib.nlsg_cached_bytes())


def tinyqr_calls(lib):
    """nlsg_tinyqr_lm and nlsg_tinyqr_qr (every output asked for) on two 3 x 2 systems: (bytes, bytes)"""
    X = np.array([[[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]] * 2)
    y = np.array([[1.0, 2.0, 3.0]] * 2)
    beta, Q, R = np.zeros((2, 2)), np.zeros((2, 3, 2)), np.zeros((2, 2, 2))
    p = lambda a: a.ctypes.data_as(A.pd)
    rc = lib.nlsg_tinyqr_lm(p(X), p(y), 2, 3, 2, 1e-7, 0, p(beta), None)
    assert rc == 0, last_error(lib)
    first = int(lib.nlsg_cached_bytes())
    emptied(lib)
    rc = lib.nlsg_tinyqr_qr(p(X), p(y), 2, 3, 2, 1e-7, 0, p(Q), p(R), p(beta))
    assert rc == 0, last_error(lib)
    return first, int(lib.nlsg_cached_bytes())


def _solve(lib, name, h):
    """the engine's solve entry point on valid buffers; returns its code"""
    x = np.full((2, 2), 0.5)
    seeds = np.arange(1, 3, dtype=np.uint64)
    lo, up = np.full((2, 2), -1.0), np.full((2, 2), 1.0)
    p = lambda a: a.ctypes.data_as(A.pd)
    kind = name.rsplit("_params", 1)[0]
    if kind == "de_batch":
        return lib.nlsg_de_batch_minimize(h, p(x), seeds.ctypes.data_as(A.pu), None)
    if kind == "pso_batch":
        return lib.nlsg_pso_batch_minimize(h, p(x), p(lo), p(up), seeds.ctypes.data_as(A.pu), None)
    if kind == "bfgs":
        return lib.nlsg_bfgs_minimize(h, p(x), None)
    if kind == "lm":
        return lib.nlsg_lm_minimize(h, p(x), None, None)
    if kind == "nm":
        return lib.nlsg_nm_minimize(h, p(x), None, None, None, None)
    if kind == "nmpso":
        return lib.nlsg_nmpso_minimize(h, p(x), None, None, None)
    return lib.nlsg_sann_minimize(h, p(x), None)


def param_messages(lib, kind):
    """nlsg_last_error after "solve before set_params" and after "set_params on an engine without
    parameters", with the two codes"""
    with_p, without, set_params = PARAM_KINDS[kind]
    h = create(lib, with_p)
    rc_solve = _solve(lib, with_p, h)
    solve_text = last_error(lib)
    destroy(lib, with_p, h)
    h = create(lib, without)
    row = np.zeros((2, 1))
    rc_set = A.require(set_params)(h, row.ctypes.data_as(A.pd))
    set_text = last_error(lib)
    destroy(lib, without, h)
    return {"solve_before_set_params": [int(rc_solve), solve_text],
            "set_params_without_parameters": [int(rc_set), set_text]}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
