"""C-ABI calls that every engine kind rejects before a device is touched, and the pure size functions
at their boundary values. Each rejected call is a valid smallest-shape call (the config builders of
tests/_engine_lifecycle.py) with exactly ONE thing wrong: the order of two checks is deliberately not
pinned. Shared by scripts/record_engine_doors.py, which wrote tests/golden/engine_doors.json at the
commit named inside, and tests/test_engine_doors_cpu.py, which replays the table and compares: an
expectation is never computed from the library under test."""
import ctypes as C
import json
import os
import re

import numpy as np

from nlsolver_amd import _capi as A
from tests import _engine_lifecycle as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_doors.json")

VECTOR = 2  # NLSG_CUSTOM_VECTOR
TOO_MANY = A.CUSTOM_MAX_PARAMS + 1
LINK = (b"return det_tanh(z);", b"return 1.0 - v * v;")
CURVE_BODY = b"r = y - th(0) * t(0) - th(1); J(0) = -t(0); J(1) = -1.0;"
GRAD_BODY = b"return 2.0 * xi;"


def _obj(n_params=0, chain=0):
    return A.CustomObjectiveC(L.GOOD, b"return s;", chain, n_params)


def _link(value=LINK[0], slope=LINK[1]):
    return A.LMLinkC(value, slope)


def _curve(body=CURVE_BODY, k=1):
    return A.LMCurveC(body, k)


def _grad(body=GRAD_BODY, size=None):
    return A.BFGSGradientC(C.sizeof(A.BFGSGradientC) if size is None else size, 0, body)


def _with(cfg, **kw):
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _vec(n=2):
    return np.full(n, 1.0)


class Door:
    """One create entry point: its symbol, the config of a valid call, and what goes between the config
    and the handle as (name, maker) pairs; a maker returning None stands for a legitimately null argument."""

    def __init__(self, symbol, cfg, extras=()):
        self.symbol, self.cfg, self.extras = symbol, cfg, tuple(extras)

    def call(self, lib, cfg_edit=None, null=None, **replace):
        """the door on its valid arguments, but: cfg_edit(cfg) applied, the argument `null` passed as NULL,
        an extra replaced by name"""
        keep = []  # (what the pointers point to lives until the call returns)
        cfg = self.cfg()
        if cfg_edit:
            cfg_edit(cfg)
        args = [None if null == "cfg" else C.byref(cfg)]
        for name, make in self.extras:
            v = replace[name] if name in replace else make()
            keep.append(v)
            if v is None or null == name:
                args.append(None)
            elif isinstance(v, np.ndarray):
                args.append(v.ctypes.data_as(A.pd))
            else:
                args.append(C.byref(v))
        h = C.c_void_p()
        args.append(None if null == "out" else C.byref(h))
        rc = A.require(self.symbol)(*args)
        assert not h.value, f"{self.symbol}: a rejected create returned a handle"
        return int(rc), (L.last_error(lib) if rc else "")

    def pointer_names(self):
        return ["cfg"] + [name for name, make in self.extras if make() is not None] + ["out"]


OBJ = ("obj", _obj)
CUSTOM = A.OBJ_CUSTOM

# kind -> {door name: Door}. "plain" is the built-in door; the others take NLSG_OBJ_CUSTOM (LM's link and
# curve doors their own objective constant).
DOORS = {
    "de": {"plain": Door("nlsg_de_create", L.de_cfg),
           "custom": Door("nlsg_de_create_custom", lambda: L.de_cfg(CUSTOM), [OBJ])},
    "de_ref": {"plain": Door("nlsg_de_ref_create", L.de_ref_cfg),
               "custom": Door("nlsg_de_ref_create_custom", lambda: L.de_ref_cfg(CUSTOM), [OBJ])},
    "de_batch": {"plain": Door("nlsg_de_batch_create", L.de_batch_cfg),
                 "custom": Door("nlsg_de_batch_create_custom", lambda: L.de_batch_cfg(CUSTOM), [OBJ])},
    "pso": {"plain": Door("nlsg_pso_create", L.pso_cfg),
            "custom": Door("nlsg_pso_create_custom", lambda: L.pso_cfg(CUSTOM), [OBJ])},
    "pso_batch": {"plain": Door("nlsg_pso_batch_create", L.pso_batch_cfg),
                  "custom": Door("nlsg_pso_batch_create_custom", lambda: L.pso_batch_cfg(CUSTOM), [OBJ])},
    "bfgs": {"plain": Door("nlsg_bfgs_create", L.bfgs_cfg, [("diag", lambda: None), ("lin", lambda: None)]),
             "quad": Door("nlsg_bfgs_create", lambda: L.bfgs_cfg(A.OBJ_QUAD_DIAG_RANK1),
                          [("diag", _vec), ("lin", _vec)]),
             "custom": Door("nlsg_bfgs_create_custom", lambda: L.bfgs_cfg(CUSTOM), [OBJ]),
             "params": Door("nlsg_bfgs_create_params", lambda: L.bfgs_cfg(CUSTOM), [("obj", lambda: _obj(1))]),
             "gradient": Door("nlsg_bfgs_create_gradient", lambda: L.bfgs_cfg(CUSTOM), [OBJ, ("grad", _grad)])},
    "lm": {"plain": Door("nlsg_lm_create", L.lm_cfg),
           "objective": Door("nlsg_lm_create", lambda: L.lm_cfg(objective=0, m=0)),
           "custom": Door("nlsg_lm_create_custom", lambda: L.lm_cfg(CUSTOM, m=0), [OBJ]),
           "params": Door("nlsg_lm_create_params", lambda: L.lm_cfg(CUSTOM, m=0), [("obj", lambda: _obj(1))]),
           "link": Door("nlsg_lm_create_link", lambda: L.lm_cfg(A.OBJ_LINK_REGRESSION), [("link", _link)]),
           "curve": Door("nlsg_lm_create_curve", lambda: L.lm_cfg(A.OBJ_CURVE_MODEL), [("curve", _curve)])},
    "nm": {"plain": Door("nlsg_nm_create", L.nm_cfg),
           "custom": Door("nlsg_nm_create_custom", lambda: L.nm_cfg(CUSTOM), [OBJ]),
           "params": Door("nlsg_nm_create_params", lambda: L.nm_cfg(CUSTOM), [("obj", lambda: _obj(1))])},
    "nmpso": {"plain": Door("nlsg_nmpso_create", L.nmpso_cfg),
              "custom": Door("nlsg_nmpso_create_custom", lambda: L.nmpso_cfg(CUSTOM), [OBJ]),
              "params": Door("nlsg_nmpso_create_params", lambda: L.nmpso_cfg(CUSTOM), [("obj", lambda: _obj(1))])},
    "sann": {"plain": Door("nlsg_sann_create", L.sann_cfg),
             "custom": Door("nlsg_sann_create_custom", lambda: L.sann_cfg(CUSTOM), [OBJ]),
             "params": Door("nlsg_sann_create_params", lambda: L.sann_cfg(CUSTOM), [("obj", lambda: _obj(1))])},
}
# the engines whose plain _create_custom takes no run-time parameters (the resident pair's does)
NO_PARAMS_AT_CUSTOM = ("de", "de_ref", "pso", "bfgs", "lm", "nm", "nmpso", "sann")

_2_31, _2_32 = 1 << 31, 1 << 32


def _set(**kw):
    return lambda cfg: _with(cfg, **kw)


# kind -> [(case name, door name, keyword arguments of Door.call)]: every fail(...) of the create's shape
# validation in front of open_engine, top to bottom
SHAPES = {
    "de": [
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("vector_dim_1025", "custom", dict(cfg_edit=_set(dim=1025), obj=_obj(chain=VECTOR))),
        ("dim_2_32", "plain", dict(cfg_edit=_set(dim=_2_32))),
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("objective_minus_1", "plain", dict(cfg_edit=_set(objective=-1))),
        ("strategy_2", "plain", dict(cfg_edit=_set(strategy=2))),
        ("shard_n_3", "plain", dict(cfg_edit=_set(shard_n=3))),
        ("shard_past_pop", "plain", dict(cfg_edit=_set(shard_lo=1))),
        ("shard_n_2_32", "plain", dict(cfg_edit=_set(pop=_2_32, shard_n=_2_32))),
    ],
    "de_ref": [
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("rastrigin", "plain", dict(cfg_edit=_set(objective=3))),
        ("vector_body", "custom", dict(obj=_obj(chain=VECTOR))),
        ("strategy_2", "plain", dict(cfg_edit=_set(strategy=2))),
        ("pop_3", "plain", dict(cfg_edit=_set(pop=3))),
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("batch_2_31", "plain", dict(cfg_edit=_set(batch=_2_31))),
        ("pop_2_31", "plain", dict(cfg_edit=_set(pop=_2_31))),
    ],
    "de_batch": [
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("pop_3", "plain", dict(cfg_edit=_set(pop=3))),
        ("pop_1025", "plain", dict(cfg_edit=_set(pop=1025))),
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("dim_129", "plain", dict(cfg_edit=_set(dim=129))),
        ("n_params_minus_1", "custom", dict(obj=_obj(-1))),
        ("n_params_too_many", "custom", dict(obj=_obj(TOO_MANY))),
        ("lds", "plain", dict(cfg_edit=_set(pop=128, dim=128))),  # 266432 bytes
        ("lds_with_params", "custom", dict(cfg_edit=_set(pop=64, dim=128), obj=_obj(4096))),  # 133824 + 32768
        ("batch_2_23", "plain", dict(cfg_edit=_set(batch=1 << 23))),
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("strategy_2", "plain", dict(cfg_edit=_set(strategy=2))),
    ],
    "pso": [
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("vector_dim_1025", "custom", dict(cfg_edit=_set(dim=1025), obj=_obj(chain=VECTOR))),
        ("dim_2_32", "plain", dict(cfg_edit=_set(dim=_2_32))),
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("type_2", "plain", dict(cfg_edit=_set(type=2))),
        ("shard_n_0", "plain", dict(cfg_edit=_set(shard_n=0))),
        ("shard_past_swarm", "plain", dict(cfg_edit=_set(shard_lo=1))),
        ("shard_n_past_2_32", "plain", dict(cfg_edit=_set(n_particles=_2_32 + 1, shard_n=_2_32 + 1))),
    ],
    "pso_batch": [
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("type_2", "plain", dict(cfg_edit=_set(type=2))),
        ("n_particles_0", "plain", dict(cfg_edit=_set(n_particles=0))),
        ("n_particles_1025", "plain", dict(cfg_edit=_set(n_particles=1025))),
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("dim_129", "plain", dict(cfg_edit=_set(dim=129))),
        ("n_params_minus_1", "custom", dict(obj=_obj(-1))),
        ("n_params_too_many", "custom", dict(obj=_obj(TOO_MANY))),
        ("lds", "plain", dict(cfg_edit=_set(n_particles=64, dim=128))),  # Vanilla: 200896 bytes
        ("lds_with_params", "custom",  # Accelerated: 140480 + 32768
         dict(cfg_edit=_set(type=A.PSO_ACCELERATED, n_particles=128, dim=128), obj=_obj(4096))),
        ("batch_2_23", "plain", dict(cfg_edit=_set(batch=1 << 23))),
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
    ],
    "bfgs": [
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("dim_1025", "plain", dict(cfg_edit=_set(dim=1025))),
        ("flags_8", "plain", dict(cfg_edit=_set(flags=8))),
        ("reference_order_symmetric", "plain",
         dict(cfg_edit=_set(flags=A.BFGS_REFERENCE_ORDER | A.BFGS_SYMMETRIC))),
        ("reference_order_vector_body", "custom",
         dict(cfg_edit=_set(flags=A.BFGS_REFERENCE_ORDER), obj=_obj(chain=VECTOR))),
        ("reference_order_rastrigin", "plain", dict(cfg_edit=_set(objective=3, flags=A.BFGS_REFERENCE_ORDER))),
        ("resident_symmetric", "plain", dict(cfg_edit=_set(flags=A.BFGS_RESIDENT | A.BFGS_SYMMETRIC))),
        ("resident_dim_65", "plain", dict(cfg_edit=_set(flags=A.BFGS_RESIDENT, dim=65))),
        ("gradient_n_params_minus_1", "gradient", dict(obj=_obj(-1))),
        ("gradient_n_params_too_many", "gradient", dict(obj=_obj(TOO_MANY))),
        ("gradient_struct_size", "gradient", dict(grad=_grad(size=3))),
        ("gradient_body_null", "gradient", dict(grad=_grad(body=None))),
        ("gradient_body_empty", "gradient", dict(grad=_grad(body=b""))),
        ("lds_with_params", "params",  # reference order at dim 513: 65536 + 4 * 32768
         dict(cfg_edit=_set(flags=A.BFGS_REFERENCE_ORDER, dim=513), obj=_obj(4096))),
    ],
    "lm": [
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("solver_3", "plain", dict(cfg_edit=_set(solver=3))),
        ("objective_with_qr", "objective", dict(cfg_edit=_set(solver=A.LM_QR))),
        ("reference_order_tanh", "plain", dict(cfg_edit=_set(solver=A.LM_CHOLESKY_REFERENCE_ORDER))),
        ("reference_order_rastrigin", "objective",
         dict(cfg_edit=_set(objective=3, solver=A.LM_CHOLESKY_REFERENCE_ORDER))),
        ("reference_order_vector_body", "custom",
         dict(cfg_edit=_set(solver=A.LM_CHOLESKY_REFERENCE_ORDER), obj=_obj(chain=VECTOR))),
        ("n_0", "plain", dict(cfg_edit=_set(n=0))),
        ("m_0", "plain", dict(cfg_edit=_set(m=0))),
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("curve_n_65", "curve", dict(cfg_edit=_set(n=65))),
        ("n_1025", "plain", dict(cfg_edit=_set(n=1025))),
        ("qr_n_65", "plain", dict(cfg_edit=_set(solver=A.LM_QR, n=65))),
        ("batch_2_31", "plain", dict(cfg_edit=_set(batch=_2_31))),
        ("link_value_null", "link", dict(link=_link(value=None))),
        ("link_value_empty", "link", dict(link=_link(value=b""))),
        ("link_slope_null", "link", dict(link=_link(slope=None))),
        ("link_slope_empty", "link", dict(link=_link(slope=b""))),
        ("curve_k_0", "curve", dict(curve=_curve(k=0))),
        ("curve_k_17", "curve", dict(curve=_curve(k=17))),
        ("curve_body_null", "curve", dict(curve=_curve(body=None))),
        ("curve_body_empty", "curve", dict(curve=_curve(body=b""))),
    ],
    "nm": [
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("dim_1025", "plain", dict(cfg_edit=_set(dim=1025))),
        ("batch_2_31", "plain", dict(cfg_edit=_set(batch=_2_31))),
        ("flags_2", "plain", dict(cfg_edit=_set(flags=2))),
        ("reference_order_rastrigin", "plain", dict(cfg_edit=_set(objective=3, flags=A.NM_REFERENCE_ORDER))),
        ("reference_order_vector_body", "custom",
         dict(cfg_edit=_set(flags=A.NM_REFERENCE_ORDER), obj=_obj(chain=VECTOR))),
        ("lds_with_params", "params", dict(cfg_edit=_set(dim=128), obj=_obj(4096))),  # 140504 + 32768
    ],
    "nmpso": [
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("dim_1", "plain", dict(cfg_edit=_set(dim=1))),
        ("dim_1025", "plain", dict(cfg_edit=_set(dim=1025))),
        ("batch_2_31", "plain", dict(cfg_edit=_set(batch=_2_31))),
    ],
    "sann": [
        ("objective_5", "plain", dict(cfg_edit=_set(objective=5))),
        ("dim_0", "plain", dict(cfg_edit=_set(dim=0))),
        ("batch_0", "plain", dict(cfg_edit=_set(batch=0))),
        ("vector_dim_1025", "custom", dict(cfg_edit=_set(dim=1025), obj=_obj(chain=VECTOR))),
        ("dim_2_32", "plain", dict(cfg_edit=_set(dim=_2_32))),
        ("batch_2_31", "plain", dict(cfg_edit=_set(batch=_2_31))),
    ],
}


def _door_cases():
    """(id, callable(lib) -> (code, text)) of every create door"""
    out = []

    def add(cid, door, **kw):
        out.append((cid, lambda lib: door.call(lib, **kw)))

    for kind, doors in DOORS.items():
        for dname, door in doors.items():
            pre = f"{kind}/{door.symbol}" + ("" if dname in ("plain", "custom", "params", "link", "curve",
                                                              "gradient") else f"[{dname}]")
            for arg in door.pointer_names():
                add(f"{pre}/null_{arg}", door, null=arg)
            add(f"{pre}/struct_size", door, cfg_edit=_set(struct_size=3))
            if dname == "plain":
                add(f"{pre}/objective_custom", door, cfg_edit=_set(objective=CUSTOM))
            elif dname in ("custom", "params", "gradient", "link", "curve"):
                add(f"{pre}/objective_builtin", door, cfg_edit=_set(objective=0))
            if dname == "custom" and kind in NO_PARAMS_AT_CUSTOM:
                add(f"{pre}/n_params_1", door, obj=_obj(1))
            if dname == "params":
                for n in (0, -1, TOO_MANY):
                    add(f"{pre}/n_params_{n}", door, obj=_obj(n))
        if kind == "lm":  # the built-in door names the creator of each of its three run-time kinds
            add("lm/nlsg_lm_create/objective_link", doors["plain"], cfg_edit=_set(objective=A.OBJ_LINK_REGRESSION))
            add("lm/nlsg_lm_create/objective_curve", doors["plain"], cfg_edit=_set(objective=A.OBJ_CURVE_MODEL))
        for name, dname, kw in SHAPES[kind]:
            add(f"{kind}/shape/{name}", doors[dname], **kw)
    return out


# ---- the handle-less tinyqr entries, as far as they validate on the host ----

def _tinyqr_cases():
    X, y, beta = np.ones(64), np.ones(64), np.zeros(64)
    p = lambda a: None if a is None else a.ctypes.data_as(A.pd)
    addr = lambda a: None if a is None else a.ctypes.data  # (never dereferenced: the call is rejected first)
    ms = C.c_float()

    def lm(X=X, y=y, batch=2, n=3, p_=2, beta=beta):
        return lambda lib: lib.nlsg_tinyqr_lm(p(X), p(y), batch, n, p_, 1e-7, 0, p(beta), C.byref(ms))

    def dev(X=X, y=y, batch=2, n=3, p_=2, beta=beta):
        return lambda lib: lib.nlsg_tinyqr_lm_device(addr(X), addr(y), batch, n, p_, 1e-7, 0, None, addr(beta))

    def qr(X=X, y=y, batch=2, n=3, p_=2, Q=beta, R=beta, beta=beta):
        return lambda lib: lib.nlsg_tinyqr_qr(p(X), p(y), batch, n, p_, 1e-7, 0, p(Q), p(R), p(beta))

    out = []
    for name, f in (("nlsg_tinyqr_lm", lm), ("nlsg_tinyqr_lm_device", dev)):
        out += [(f"tinyqr/{name}/null_X", f(X=None)), (f"tinyqr/{name}/null_y", f(y=None)),
                (f"tinyqr/{name}/null_beta", f(beta=None)),
                (f"tinyqr/{name}/batch_0", f(batch=0)), (f"tinyqr/{name}/n_0", f(n=0)),
                (f"tinyqr/{name}/p_0", f(p_=0)), (f"tinyqr/{name}/p_65", f(n=65, p_=65)),
                (f"tinyqr/{name}/n_below_p", f(n=2, p_=3)), (f"tinyqr/{name}/batch_2_31", f(batch=_2_31)),
                (f"tinyqr/{name}/n_2_30", f(n=1 << 30))]
    out += [("tinyqr/nlsg_tinyqr_qr/null_X", qr(X=None)),
            ("tinyqr/nlsg_tinyqr_qr/no_output", qr(Q=None, R=None, beta=None)),
            ("tinyqr/nlsg_tinyqr_qr/beta_without_y", qr(y=None)),
            ("tinyqr/nlsg_tinyqr_qr/batch_0", qr(batch=0)), ("tinyqr/nlsg_tinyqr_qr/n_0", qr(n=0)),
            ("tinyqr/nlsg_tinyqr_qr/p_0", qr(p_=0)), ("tinyqr/nlsg_tinyqr_qr/n_below_p", qr(n=2, p_=3)),
            ("tinyqr/nlsg_tinyqr_qr/n_plus_p_1281", qr(n=1217, p_=64)),
            ("tinyqr/nlsg_tinyqr_qr/beta_p_65", qr(n=65, p_=65))]
    return [(cid, (lambda f: lambda lib: _coded(lib, f(lib)))(f)) for cid, f in out]


def _coded(lib, rc):
    return int(rc), (L.last_error(lib) if rc else "")


# ---- every other exported entry point that takes a handle, on a null handle ----

def handle_symbols():
    """the nlsg_* functions of include/nlsg_c_api.h whose first parameter is an engine handle `e`"""
    text = open(os.path.join(ROOT, "include", "nlsg_c_api.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nlsg_[a-z0-9_]+)\s*\(\s*(?:const\s+)?nlsg_[a-z_]+\s*\*\s*e\b", text)))


def _default(argtype, keep):
    """a valid stand-in for one argument of a call that is rejected before it reads any of them"""
    if argtype in (A.pd, A.pu):
        a = np.zeros(64, dtype=np.float64 if argtype is A.pd else np.uint64)
        keep.append(a)
        return a.ctypes.data_as(argtype)
    if argtype is C.c_void_p:
        a = np.zeros(64)
        keep.append(a)
        return a.ctypes.data
    if isinstance(argtype, type) and issubclass(argtype, C._Pointer):
        a = (argtype._type_ * 128)()
        keep.append(a)
        return C.cast(a, argtype)
    return 0.5 if argtype is C.c_double else 1


def _is_pointer(argtype):
    return argtype is C.c_void_p or (isinstance(argtype, type) and issubclass(argtype, C._Pointer))


def _null_handle_cases():
    out = []
    for name in handle_symbols():
        res, argtypes = A.SYMBOLS[name]

        def call(lib, name=name, res=res, argtypes=argtypes, null_at=None):
            keep = []
            args = [None] + [None if i == null_at else _default(t, keep)
                             for i, t in enumerate(argtypes[1:], start=1)]
            rc = A.require(name)(*args)
            # (uint64_t and yes / no answers have no error text; a code of 0 has none either)
            return int(rc), (L.last_error(lib) if res is C.c_int and rc and "_can_" not in name else "")

        out.append((f"null_handle/{name}", call))
        for i, t in enumerate(argtypes[1:], start=1):
            if _is_pointer(t):
                out.append((f"null_handle/{name}/null_arg{i}", lambda lib, call=call, i=i: call(lib, null_at=i)))
    return out


def cases():
    """[(id, callable(lib) -> (code, text of nlsg_last_error or "" for code 0))], in a fixed order"""
    return _door_cases() + _tinyqr_cases() + _null_handle_cases()


# ---- the pure size functions at their boundary values ----

_DIMS = (0, 1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
_N_PARAMS = (-1, 0, 1, 2, 3, 100, 1000, 4096, 4097)


def pure():
    """[(id, callable(lib) -> int)]"""
    out = []

    def add(symbol, *args):
        out.append((f"{symbol}({', '.join(str(a) for a in args)})",
                    lambda lib: int(A.require(symbol)(*args))))

    for n in _N_PARAMS:
        add("nlsg_custom_params_lds_bytes", n)
    for pop in (3, 4, 1024, 1025):
        for dim in (0, 1, 128, 129):
            add("nlsg_de_batch_lds_bytes", pop, dim)
    for n in (0, 1, 1024, 1025):
        for dim in (0, 1, 128, 129):
            for t in (-1, 0, 1, 2):
                add("nlsg_pso_batch_lds_bytes", n, dim, t)
    for dim in _DIMS:
        for flags in (0, 1, 2):
            add("nlsg_nm_lds_bytes", dim, flags)
        add("nlsg_nmpso_lds_bytes", dim)
        for solver in (-1, 0, 1, 2, 3):
            add("nlsg_lm_lds_bytes", dim, solver)
        for flags in range(0, 9):
            add("nlsg_bfgs_lds_bytes", dim, flags)
    add("nlsg_nmpso_lds_bytes", 2)
    for dim in (0, 1, 8, 9, 16, 17, 32, 33, 64, 65, 1024, 1025):
        for n in _N_PARAMS:
            add("nlsg_sann_chains_per_wave", dim, n)
            add("nlsg_sann_lds_bytes", dim, n)
    return out


def replay(lib):
    """what the recorder writes and the test compares: {"cases": {id: [code, text]}, "pure": {id: value}}"""
    rec = {"cases": {}, "pure": {}}
    for cid, call in cases():
        assert cid not in rec["cases"], cid
        rec["cases"][cid] = list(call(lib))
    for cid, call in pure():
        assert cid not in rec["pure"], cid
        rec["pure"][cid] = call(lib)
    return rec


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
