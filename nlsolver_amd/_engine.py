"""What the engine classes of de.py, pso.py, bfgs.py, lm.py, nm.py, nmpso.py and sann.py share: the
objective given as source text, the base class that owns an engine's handle, config header and
parameter rows, and the small conversions between numpy and the C-ABI. One owner, so that a change to
how an engine is made is written once."""
import ctypes as C
import os

import numpy as np

from . import _capi
from ._capi import NlsgError, check, lib, require

DEFAULT_SEED = 12374563468  # rng::splitmix seed, nlsolver.h:1265
LDS_BUDGET = 160 * 1024  # bytes of LDS one gfx950 workgroup can take (DEBatchEngine's limit)


def seed_from_generator(generator):
    """Two draws of a reference-style generator (T operator()() in [0,1]) -> u64 key."""
    if generator is None:
        return DEFAULT_SEED
    if isinstance(generator, int):
        return generator & (2**64 - 1)
    hi = min(int(generator() * 2.0**32), 2**32 - 1)
    lo = min(int(generator() * 2.0**32), 2**32 - 1)
    return (hi << 32) | lo


class CustomObjective:
    """A user objective f(x) = finish(sum_i term(x_i, x_{i+1}), D) given as C++ function bodies and
    compiled for the device when the engine is created (nlsg_custom_objective).

        CustomObjective("double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;",
                        chain=True)                       # the Rosenbrock chain
        CustomObjective("return fabs(xi) * xi * xi;")     # sum |x_i|^3

    In the bodies: `xi`, `xn` (= x_{i+1}; chain objectives sum over i < D - 1) for `term`; `s`, `D`
    for `finish` (default "return s;").

    vector=True: the whole-vector form (NLSG_CUSTOM_VECTOR) for objectives that are not sums of
    such terms — `term_body` is the body of `double f(const X &x, uint64_t D)` with `x(i)`
    (coordinate i, same index in every lane), `x.size()` and `x.sum(g)` (lane-tree sum of
    g(x_i, i) over the coordinates):

        CustomObjective("double a = x(0) * x(0) + x(1) - 11, b = x(0) + x(1) * x(1) - 7;"
                        " return a * a + b * b;", vector=True)    # Himmelblau

    n_params > 0: the objective owns that many doubles of run-time data per solve, read in every
    body (and in lambdas given to x.sum) as `p(k)`, k any uint64_t below n_params. The values come
    from DEBatchEngine / PSOBatchEngine.set_params ([batch, n_params]: solve b sees row b) or from
    `params=` of the DE / PSO drop-ins; they can be replaced without recompiling. NMEngine and
    NMPSOEngine take such an objective the same way (set_params: start / instance b sees row b), and
    NelderMead / NelderMeadPSO take `params=`; no other engine does. At most CUSTOM_MAX_PARAMS.

        CustomObjective("double r = xi - p(0); return p(1) * r * r;", n_params=2)

    grad_body: the objective's analytic gradient as one more body, which BFGSEngine / BFGS evaluate
    instead of the default finite differences (nlsg_bfgs_create_gradient); every other engine ignores
    it. Terms and chain objectives: the body of
    `double grad(double xm, double xi, double xn, uint64_t i, uint64_t D, double s)`, returning
    df/dx_i, with xm = x_{i-1} (+0.0 at i = 0), xn = x_{i+1} (+0.0 at i = D - 1) and s the sum of the
    objective's terms at x, what `finish` receives; plain per-lane code. vector=True: the body of
    `double grad(const X &x, uint64_t i, uint64_t D)` with x(i), x.size(), x.sum(g); it is called for
    i = 0 .. D - 1 with the same i in every lane — D evaluations of the body per gradient, against
    4 D evaluations of the objective with finite differences. p(k) works in either.

        CustomObjective("double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;",
                        chain=True,
                        grad_body="double g = 0.0;"
                                  " if (i + 1 < D) g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi);"
                                  " if (i > 0) g = g + 200.0 * (xi - xm * xm); return g;")"""

    def __init__(self, term_body, *, chain=False, finish_body="return s;", vector=False, n_params=0,
                 grad_body=None):
        if grad_body is not None and (not isinstance(grad_body, str) or not grad_body.strip()):
            raise ValueError("grad_body must be a non-empty string of source text, or None")
        self.grad_body = grad_body
        self.term_body, self.finish_body = term_body, finish_body
        self.chain = 2 if vector else int(bool(chain))  # nlsg_custom_objective.chain
        n_params = int(n_params)
        if not 0 <= n_params <= _capi.CUSTOM_MAX_PARAMS:
            raise ValueError(f"n_params must be in 0 .. {_capi.CUSTOM_MAX_PARAMS}, not {n_params}")
        self.n_params = n_params


def rtc_library_path():
    """hiprtc of the HIP runtime this process already uses (PyTorch ships its own)."""
    try:
        import torch
        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libhiprtc.so")
        return cand if os.path.exists(cand) else ""
    except ImportError:
        return ""


# ---- numpy <-> C-ABI ---------------------------------------------------------------------------
def pd_of(a):
    """const double * of a contiguous float64 array; None stays NULL"""
    return None if a is None else a.ctypes.data_as(_capi.pd)


def pu_of(a):
    """uint64_t * of a contiguous uint64 array; None stays NULL"""
    return None if a is None else a.ctypes.data_as(_capi.pu)


def timed_ms(fn, *args):
    """the milliseconds a timing entry point stores behind its last argument"""
    ms = C.c_float()
    check(fn(*args, C.byref(ms)))
    return ms.value


def seeds_u64(seeds, batch):
    """seeds [batch] of any integers, each taken modulo 2^64"""
    return np.array([int(s) & (2**64 - 1) for s in np.asarray(seeds, dtype=object).ravel()],
                    dtype=np.uint64).reshape(batch)


def _with_params_lds(need, n_params):
    """need + nlsg_custom_params_lds_bytes(n_params); 0 when either is out of range"""
    if not n_params:
        return need
    extra = int(require("nlsg_custom_params_lds_bytes")(n_params))
    return need + extra if need and extra else 0


def _params_rows(params, batch, n_params):
    """params as a contiguous float64 [batch, n_params]"""
    return np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(batch, n_params))


# ---- the drop-ins' params= and driver= ---------------------------------------------------------
def _drop_in_rows(params, n_params):
    """params= of a drop-in: (n_params,) -> [1, n_params]; (batch, n_params) stays"""
    rows = np.ascontiguousarray(np.asarray(params, dtype=np.float64))
    if rows.ndim == 1:
        rows = rows.reshape(1, -1)
    if rows.ndim != 2 or rows.shape[1] != n_params:
        raise ValueError(f"params must be ({n_params},) or (batch, {n_params}), not {rows.shape}")
    return rows


def _rows_for_batch(rows, batch):
    """the drop-in's rows for a solve of `batch` starts: one row goes to every start"""
    if rows is None:
        return None
    if rows.shape[0] == 1:
        return np.ascontiguousarray(np.broadcast_to(rows, (batch, rows.shape[1])))
    if rows.shape[0] != batch:
        raise ValueError(f"params has {rows.shape[0]} rows and x {batch} starts")
    return rows


def pair_params(f, params, rows=_drop_in_rows):
    """(n_params of the drop-in's objective f, its params= as rows(params, n_params) or None):
    the two go together or not at all"""
    n_params = getattr(f, "n_params", 0)
    if (params is not None) != bool(n_params):
        raise ValueError("params= goes with a CustomObjective whose n_params > 0, and such an "
                         "objective needs it")
    return n_params, None if params is None else rows(params, n_params)


def check_driver(driver):
    if driver not in ("turns", "resident"):
        raise ValueError(f"driver must be 'turns' or 'resident', not {driver!r}")


# ---- the engines' base -------------------------------------------------------------------------
class Engine:
    """One handle of the C-ABI on one device and one stream, destroyed with the object. A subclass names
    its symbols and fills the fields of its config that are its own."""

    _destroy = None  # "nlsg_<engine>_destroy"
    _set_params = None  # "nlsg_<engine>_set_params"; None where the engine takes no parameter rows (and has no n_params)

    def _header(self, Config, device, stream):
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.device = device
        # None: the engine creates a private stream. An integer is a hipStream_t handle;
        # 0 is torch's default (null) stream, spelled hipStreamLegacy = 1 for the C-ABI.
        cfg.stream = None if stream is None else (stream or 1)
        self.cfg = cfg
        return cfg

    @staticmethod
    def _objective_id(objective):
        """(config's objective id, the CustomObjective or None) of a name, an id or a CustomObjective"""
        if isinstance(objective, CustomObjective):
            return _capi.OBJ_CUSTOM, objective
        return (_capi.OBJECTIVES[objective] if isinstance(objective, str) else objective), None

    def _creator(self, create, params_create=None):
        """the creator of a compiled objective: `create`, or the optional `params_create` where the
        objective declares parameters (zero stays with the creator it always had). Parameters need the
        engine's set_params as well: a library without either says so here, before anything is made."""
        if self.n_params:
            if params_create:
                create = require(params_create)
            require(self._set_params)
        return create

    def _create(self, create, cfg, *extras):
        self._h = C.c_void_p()
        check(create(C.byref(cfg), *extras, C.byref(self._h)))

    def _create_custom(self, create, cfg, custom, *more):
        """create with source text to compile: a CustomObjective, or the engine's own struct of bodies.
        `create` is resolved by the caller, so a library without it has said so before hiprtc is loaded."""
        check(lib().nlsg_rtc_load(rtc_library_path().encode()))
        if isinstance(custom, CustomObjective):
            custom = _capi.CustomObjectiveC(custom.term_body.encode(), custom.finish_body.encode(),
                                            int(custom.chain), custom.n_params)
        self._create(create, cfg, C.byref(custom), *[C.byref(m) for m in more])

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- parameter rows ---------------------------------------------------
    def set_params(self, params):
        """params [batch, n_params]: row b is what solve / start / problem b's objective reads as p(k).
        The rows hold from the next launch on and can be replaced at any time without recompiling."""
        if self._set_params is None or self.n_params == 0:
            raise NlsgError(_capi.NLSG_ERR_INVALID_ARG, "the engine's objective declares no parameters")
        rows = _params_rows(params, self.cfg.batch, self.n_params)
        check(require(self._set_params)(self._h, pd_of(rows)))

    def _apply_params(self, params):
        if params is not None:
            self.set_params(params)
