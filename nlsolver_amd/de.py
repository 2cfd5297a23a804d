"""Host-side mirror of the reference's DE class for device objectives.

Reference interface (nlsolver.h:2379-2411):
    DE<Callable, RNG, scalar_t, RecombinationStrategy>(f, generator, CR=0.9, F=0.8,
        eps=10e-4, pop_size=50, max_iter=1000, best_val_no_change=50)
    solver_status minimize(std::vector<T>& x) / maximize(std::vector<T>& x)
Same positional arguments, defaults and in/out `x` convention here; `f` is the
name of a built-in device objective (a device kernel cannot call a host functor,
DESIGN.md), `generator` supplies the 64-bit key of the counter-based RNG.
All compute happens in libnlsolver_hip.so on a gfx950 device.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (DE_BEST, DE_RANDOM, DEBatchConfig, DEConfig, DERefConfig, NlsgError, Status, check,
                    lib, require)
from .rng import XorShift

DEFAULT_SEED = 12374563468  # rng::splitmix seed, nlsolver.h:1265


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
    import os
    try:
        import torch
        cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libhiprtc.so")
        return cand if os.path.exists(cand) else ""
    except ImportError:
        return ""


class DEEngine:
    """Thin RAII wrapper over the nlsg_de_* C-ABI (one handle, one device, one stream)."""

    def __init__(self, objective, pop, dim, *, minimize=True, strategy=DE_RANDOM, CR=0.9, F=0.8,
                 eps=10e-4, max_iter=1000, best_val_no_change=50, seed=DEFAULT_SEED, device=0,
                 stream=None, shard_lo=0, shard_n=None, trace=False):
        cfg = DEConfig()
        cfg.struct_size = C.sizeof(DEConfig)
        cfg.device = device
        # None: the engine creates a private stream. An integer is a hipStream_t handle;
        # 0 is torch's default (null) stream, spelled hipStreamLegacy = 1 for the C-ABI.
        cfg.stream = None if stream is None else (stream or 1)
        custom = objective if isinstance(objective, CustomObjective) else None
        cfg.objective = (_capi.OBJ_CUSTOM if custom else
                         _capi.OBJECTIVES[objective] if isinstance(objective, str) else objective)
        cfg.minimize = int(bool(minimize))
        cfg.strategy = strategy
        cfg.trace = int(bool(trace))
        cfg.pop, cfg.dim = pop, dim
        cfg.shard_lo = shard_lo
        cfg.shard_n = pop if shard_n is None else shard_n
        cfg.CR, cfg.F, cfg.eps = CR, F, eps
        cfg.max_iter, cfg.best_val_no_change, cfg.seed = max_iter, best_val_no_change, seed
        self.cfg = cfg
        self._h = C.c_void_p()
        if custom:
            check(lib().nlsg_rtc_load(rtc_library_path().encode()))
            obj = _capi.CustomObjectiveC(custom.term_body.encode(), custom.finish_body.encode(),
                                         int(custom.chain), custom.n_params)
            check(lib().nlsg_de_create_custom(C.byref(cfg), C.byref(obj), C.byref(self._h)))
        else:
            check(lib().nlsg_de_create(C.byref(cfg), C.byref(self._h)))

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().nlsg_de_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- C-ABI calls ------------------------------------------------------
    def init(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape != (self.cfg.dim,):
            raise ValueError(f"x0 must have {self.cfg.dim} entries")
        check(lib().nlsg_de_init(self._h, x0.ctypes.data_as(_capi.pd)))

    def step(self, turns=1):
        check(lib().nlsg_de_step(self._h, turns))

    def status(self):
        st = Status()
        check(lib().nlsg_de_status(self._h, C.byref(st)))
        return st

    def best(self):
        x = np.empty(self.cfg.dim)
        f, idx = C.c_double(), C.c_uint64()
        check(lib().nlsg_de_best(self._h, x.ctypes.data_as(_capi.pd), C.byref(f), C.byref(idx)))
        return x, f.value, idx.value

    def download(self, trace=False):
        n, D = self.cfg.shard_n, self.cfg.dim
        pop, scores = np.empty((n, D)), np.empty(n)
        tr = np.empty((n, 5), dtype=np.uint64) if trace else None
        check(lib().nlsg_de_download(self._h, pop.ctypes.data_as(_capi.pd),
                                     scores.ctypes.data_as(_capi.pd),
                                     tr.ctypes.data_as(_capi.pu) if trace else None))
        return (pop, scores, tr) if trace else (pop, scores)

    def upload(self, pop, scores):
        pop = np.ascontiguousarray(pop, dtype=np.float64)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        assert pop.shape == (self.cfg.shard_n, self.cfg.dim) and scores.shape == (self.cfg.shard_n,)
        check(lib().nlsg_de_upload(self._h, pop.ctypes.data_as(_capi.pd),
                                   scores.ctypes.data_as(_capi.pd)))

    def bound_counts(self):
        """(decided, fell through and rejected, accepted): agents since init() whose trial the
        generation's lower bound rejected unread / did not decide and selection rejected / did not
        decide (or had no kept coordinate) and selection accepted. Needs trace=True; all zero in
        an engine that does not use the bound (bound_state)."""
        out = np.zeros(3, dtype=np.uint64)
        check(require("nlsg_de_bound_counts")(self._h, out.ctypes.data_as(_capi.pu)))
        return tuple(int(v) for v in out)

    def bound_state(self):
        """(enabled, retry period in generations) of the generation's lower-bound rejection"""
        on, r = C.c_int32(), C.c_uint32()
        check(require("nlsg_de_bound_state")(self._h, C.byref(on), C.byref(r)))
        return bool(on.value), r.value

    def screen_counts(self):
        """(decided, missed): agents since init() whose trial the half-row screen rejected (they
        count as decided in bound_counts too) / that tried it and went on to the one-agent path.
        Needs trace=True; both zero in an engine that does not screen (screen_state)."""
        out = np.zeros(2, dtype=np.uint64)
        check(require("nlsg_de_screen_counts")(self._h, out.ctypes.data_as(_capi.pu)))
        return tuple(int(v) for v in out)

    def screen_state(self):
        """(enabled, retry period in generations) of the generation's half-row screen"""
        on, r = C.c_int32(), C.c_uint32()
        check(require("nlsg_de_screen_state")(self._h, C.byref(on), C.byref(r)))
        return bool(on.value), r.value

    def minimize(self, x, poll_every=0):
        st = Status()
        check(lib().nlsg_de_minimize(self._h, x.ctypes.data_as(_capi.pd), poll_every, C.byref(st)))
        return st

    def time_generation_kernel(self, launches):
        ms = C.c_float()
        check(lib().nlsg_de_time_generation_kernel(self._h, launches, C.byref(ms)))
        return ms.value

    def time_turns(self, turns):
        ms = C.c_float()
        check(lib().nlsg_de_time_turns(self._h, turns, C.byref(ms)))
        return ms.value

    def record_doubles(self):
        return lib().nlsg_de_record_doubles(self._h)

    def turn_begin(self, send_dev_ptr):
        check(lib().nlsg_de_turn_begin(self._h, send_dev_ptr))

    def turn_end(self, gathered_dev_ptr, world):
        check(lib().nlsg_de_turn_end(self._h, gathered_dev_ptr, world))

    def turn_finalize(self, gathered_dev_ptr, world):
        check(lib().nlsg_de_turn_finalize(self._h, gathered_dev_ptr, world))

    def turn_generation(self):
        check(lib().nlsg_de_turn_generation(self._h))

    def can_speculate(self):
        return bool(lib().nlsg_de_can_speculate(self._h))

    def comm_attach(self, unique_id, world, rank):
        """Collective: joins the library-side RCCL communicator (see nlsolver_amd.dist)."""
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        check(lib().nlsg_de_comm_attach(self._h, buf, world, rank))

    def step_sharded(self, turns=1):
        check(lib().nlsg_de_step_sharded(self._h, turns))

    def comm_ranks(self):
        """(world, rank) as the attached RCCL communicator reports them."""
        w, r = C.c_int32(), C.c_int32()
        check(lib().nlsg_de_comm_ranks(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value


class DERefEngine:
    """Reference-order DE (nlsg_de_ref_*): `batch` independent solves of the reference's own DE
    (nlsolver.h:2414-2476) — in-place asynchronous generation, every draw from the solve's own
    xorshift state — each returning the reference's x, status and final generator state bit for bit.
    `objective`: "rosenbrock", "sphere", "styblinski_tang" or a CustomObjective given by its terms."""

    def __init__(self, objective, batch, pop, dim, *, minimize=True, strategy=DE_RANDOM, CR=0.9,
                 F=0.8, eps=10e-4, max_iter=1000, best_val_no_change=50, log_capacity=0, device=0,
                 stream=None):
        cfg = DERefConfig()
        cfg.struct_size = C.sizeof(DERefConfig)
        cfg.device = device
        cfg.stream = None if stream is None else (stream or 1)
        custom = objective if isinstance(objective, CustomObjective) else None
        cfg.objective = (_capi.OBJ_CUSTOM if custom else
                         _capi.OBJECTIVES[objective] if isinstance(objective, str) else objective)
        cfg.minimize, cfg.strategy = int(bool(minimize)), strategy
        cfg.batch, cfg.pop, cfg.dim = batch, pop, dim
        cfg.CR, cfg.F, cfg.eps = CR, F, eps
        cfg.max_iter, cfg.best_val_no_change, cfg.log_capacity = max_iter, best_val_no_change, log_capacity
        self.cfg = cfg
        self._h = C.c_void_p()
        if custom:
            create = require("nlsg_de_ref_create_custom")
            check(lib().nlsg_rtc_load(rtc_library_path().encode()))
            obj = _capi.CustomObjectiveC(custom.term_body.encode(), custom.finish_body.encode(),
                                         int(custom.chain), custom.n_params)
            check(create(C.byref(cfg), C.byref(obj), C.byref(self._h)))
        else:
            check(require("nlsg_de_ref_create")(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().nlsg_de_ref_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _inputs(self, x, states):
        B, D = self.cfg.batch, self.cfg.dim
        x = np.array(x, dtype=np.float64).reshape(B, D)
        states = np.array(states, dtype=np.uint64).reshape(B, 2)
        return x, states

    def minimize(self, x, states):
        """x [batch, dim] (x0), states [batch, 2] (xorshift x[0], x[1]) ->
        (x [batch, dim], [Status] * batch, states [batch, 2]) — new arrays, the inputs are kept"""
        x, states = self._inputs(x, states)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_de_ref_minimize(self._h, x.ctypes.data_as(_capi.pd),
                                         states.ctypes.data_as(_capi.pu), st))
        return x, list(st), states

    def log(self, b):
        """(xs [n, dim], fs [n], count) of solve b's last minimize: the evaluations in the
        reference's call order, n = min(count, log_capacity)"""
        n = C.c_uint64()
        check(lib().nlsg_de_ref_log(self._h, b, None, None, C.byref(n)))
        m = min(n.value, self.cfg.log_capacity)
        xs, fs = np.empty((m, self.cfg.dim)), np.empty(m)
        if m:
            check(lib().nlsg_de_ref_log(self._h, b, xs.ctypes.data_as(_capi.pd),
                                        fs.ctypes.data_as(_capi.pd), C.byref(n)))
        return xs, fs, n.value

    def time_solve(self, x0, states, repeats=1):
        """milliseconds of `repeats` whole solves from x0 / states (hipEvents)"""
        x0, states = self._inputs(x0, states)
        ms = C.c_float()
        check(lib().nlsg_de_ref_time_solve(self._h, x0.ctypes.data_as(_capi.pd),
                                           states.ctypes.data_as(_capi.pu), repeats, C.byref(ms)))
        return ms.value


def _with_params_lds(need, n_params):
    """need + nlsg_custom_params_lds_bytes(n_params); 0 when either is out of range"""
    if not n_params:
        return need
    extra = int(require("nlsg_custom_params_lds_bytes")(n_params))
    return need + extra if need and extra else 0


def _params_rows(params, batch, n_params):
    """params as a contiguous float64 [batch, n_params]"""
    return np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(batch, n_params))


LDS_BUDGET = 160 * 1024  # bytes of LDS one gfx950 workgroup can take (DEBatchEngine's limit)


class DEBatchEngine:
    """Resident batch DE (nlsg_de_batch_*): `batch` independent solves of the keyed engine of one
    shape, each with its own 64-bit seed and x0, one workgroup per solve with the population in LDS
    and the whole turn loop inside one kernel. Solve b is bit-identical to
    DEEngine(objective, pop, dim, seed=seeds[b], ...) driven by the same calls; it ends
    independently of its neighbours. 4 <= pop <= 1024, 1 <= dim <= 128 and lds_bytes(pop, dim)
    within LDS_BUDGET, else NlsgError (code 2): there is no global-memory fallback."""

    @staticmethod
    def lds_bytes(pop, dim, n_params=0):
        """LDS bytes a solve of this shape needs, the row of n_params objective parameters
        included; 0 outside the pop / dim / n_params ranges (host only)"""
        need = int(require("nlsg_de_batch_lds_bytes")(pop, dim))
        return _with_params_lds(need, n_params)

    @staticmethod
    def fits(pop, dim, n_params=0):
        need = DEBatchEngine.lds_bytes(pop, dim, n_params)
        return 0 < need <= LDS_BUDGET

    def __init__(self, objective, batch, pop, dim, *, minimize=True, strategy=DE_RANDOM, CR=0.9,
                 F=0.8, eps=10e-4, max_iter=1000, best_val_no_change=50, turns_per_launch=0,
                 device=0, stream=None):
        cfg = DEBatchConfig()
        cfg.struct_size = C.sizeof(DEBatchConfig)
        cfg.device = device
        cfg.stream = None if stream is None else (stream or 1)
        custom = objective if isinstance(objective, CustomObjective) else None
        cfg.objective = (_capi.OBJ_CUSTOM if custom else
                         _capi.OBJECTIVES[objective] if isinstance(objective, str) else objective)
        cfg.minimize, cfg.strategy = int(bool(minimize)), strategy
        cfg.batch, cfg.pop, cfg.dim = batch, pop, dim
        cfg.CR, cfg.F, cfg.eps = CR, F, eps
        cfg.max_iter, cfg.best_val_no_change = max_iter, best_val_no_change
        cfg.turns_per_launch = turns_per_launch
        self.cfg = cfg
        self.n_params = custom.n_params if custom else 0
        self._h = C.c_void_p()
        if custom:
            create = require("nlsg_de_batch_create_custom")
            if self.n_params:
                require("nlsg_de_batch_set_params")
            check(lib().nlsg_rtc_load(rtc_library_path().encode()))
            obj = _capi.CustomObjectiveC(custom.term_body.encode(), custom.finish_body.encode(),
                                         int(custom.chain), self.n_params)
            check(create(C.byref(cfg), C.byref(obj), C.byref(self._h)))
        else:
            check(require("nlsg_de_batch_create")(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().nlsg_de_batch_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _inputs(self, x0, seeds):
        B, D = self.cfg.batch, self.cfg.dim
        x0 = np.array(x0, dtype=np.float64).reshape(B, D)
        seeds = np.array([int(s) & (2**64 - 1) for s in np.asarray(seeds, dtype=object).ravel()],
                         dtype=np.uint64).reshape(B)
        return x0, seeds

    def set_params(self, params):
        """params [batch, n_params]: solve b's objective reads row b as p(k). The rows hold from the
        next launch on and can be replaced at any time without recompiling; scores already stored
        are not re-evaluated, so call init / minimize afterwards to solve under the new rows."""
        if self.n_params == 0:
            raise NlsgError(_capi.NLSG_ERR_INVALID_ARG, "the engine's objective declares no parameters")
        rows = _params_rows(params, self.cfg.batch, self.n_params)
        check(require("nlsg_de_batch_set_params")(self._h, rows.ctypes.data_as(_capi.pd)))

    def init(self, x0, seeds):
        """x0 [batch, dim], seeds [batch]: DEEngine.init of every solve under its own seed"""
        x0, seeds = self._inputs(x0, seeds)
        check(lib().nlsg_de_batch_init(self._h, x0.ctypes.data_as(_capi.pd), seeds.ctypes.data_as(_capi.pu)))

    def step(self, turns=1):
        check(lib().nlsg_de_batch_step(self._h, turns))

    def status(self):
        """[Status] * batch, each what DEEngine.status() returns after the same calls"""
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_de_batch_status(self._h, st))
        return list(st)

    def best(self):
        """(x [batch, dim], f [batch], index [batch]) as of every solve's last head"""
        B, D = self.cfg.batch, self.cfg.dim
        x, f, idx = np.empty((B, D)), np.empty(B), np.empty(B, dtype=np.uint64)
        check(lib().nlsg_de_batch_best(self._h, x.ctypes.data_as(_capi.pd), f.ctypes.data_as(_capi.pd),
                                       idx.ctypes.data_as(_capi.pu)))
        return x, f, idx

    def download(self, b):
        """(pop [pop, dim], scores [pop]) of solve b's current generation"""
        n, D = self.cfg.pop, self.cfg.dim
        pop, scores = np.empty((n, D)), np.empty(n)
        check(lib().nlsg_de_batch_download(self._h, b, pop.ctypes.data_as(_capi.pd),
                                           scores.ctypes.data_as(_capi.pd)))
        return pop, scores

    def upload(self, pops, scores):
        """overwrites the current generation of every solve: pops [batch, pop, dim], scores [batch, pop]"""
        B, n, D = self.cfg.batch, self.cfg.pop, self.cfg.dim
        pops = np.ascontiguousarray(pops, dtype=np.float64)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        assert pops.shape == (B, n, D) and scores.shape == (B, n)
        check(lib().nlsg_de_batch_upload(self._h, pops.ctypes.data_as(_capi.pd),
                                         scores.ctypes.data_as(_capi.pd)))

    def minimize(self, x, seeds, params=None):
        """init, then turns until every solve is done -> (x [batch, dim], [Status] * batch): new
        arrays, the inputs are kept. params: set_params(params) first."""
        if params is not None:
            self.set_params(params)
        x, seeds = self._inputs(x, seeds)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_de_batch_minimize(self._h, x.ctypes.data_as(_capi.pd),
                                           seeds.ctypes.data_as(_capi.pu), st))
        return x, list(st)

    def time_solve(self, x0, seeds, repeats=1, params=None):
        """milliseconds of `repeats` whole solves from x0 / seeds (hipEvents). params:
        set_params(params) first."""
        if params is not None:
            self.set_params(params)
        x0, seeds = self._inputs(x0, seeds)
        ms = C.c_float()
        check(lib().nlsg_de_batch_time_solve(self._h, x0.ctypes.data_as(_capi.pd),
                                             seeds.ctypes.data_as(_capi.pu), repeats, C.byref(ms)))
        return ms.value


def jump_table():
    """The nibble table of M^64 the reference-order engine advances its lanes with:
    uint64 [32, 16, 2] (entry (j, v) = xorshift128+ advanced 64 steps from the state whose nibble
    j is v; nibbles 0-15 of x[0], then 0-15 of x[1])."""
    t = np.empty((32, 16, 2), dtype=np.uint64)
    check(require("nlsg_de_ref_jump_table")(t.ctypes.data_as(_capi.pu)))
    return t


def pick_donors(draws, fixed, pop):
    """The engine's generate_indices on given draws: (ids[4], draws used, flag) with flag 0,
    1 (an index >= pop: a draw of 1.0) or 2 (the 2^20-draw cap)."""
    d = np.ascontiguousarray(draws, dtype=np.float64)
    ids, used, flag = np.zeros(4, dtype=np.uint64), C.c_uint64(), C.c_int32()
    check(require("nlsg_de_ref_pick_donors")(d.ctypes.data_as(_capi.pd), d.size, fixed, pop,
                                             ids.ctypes.data_as(_capi.pu), C.byref(used), C.byref(flag)))
    return [int(v) for v in ids], used.value, flag.value


class DE:
    """Drop-in for nlsolver::DE on a device objective (same ctor args/defaults).

    generation="reference": the reference's own generation on the caller's generator, which must
    then be an XorShift; it is advanced in place exactly as the reference advances it, and x and the
    status are the reference's bit for bit (DERefEngine, batch 1). Default: the keyed engine
    (synchronous generation, counter generator keyed by two draws of `generator`).

    driver="resident": the keyed solve runs through a batch-1 DEBatchEngine -- the whole turn loop
    in one kernel instead of a launch per generation -- when the population fits a workgroup's LDS
    (DEBatchEngine.fits), through DEEngine otherwise; the bits are the same either way.
    `driver_used` says which engine the last solve ran on. Default "turns": DEEngine.

    params: the one row of run-time parameters of a CustomObjective with n_params > 0. Such an
    objective always runs through the resident engine (the only one that takes parameters),
    whatever `driver` says; a shape that does not fit there is NlsgError code 2."""

    def __init__(self, f, generator=None, crossover_prob=0.9, differential_weight=0.8, eps=10e-4,
                 pop_size=50, max_iter=1000, best_val_no_change=50, *, strategy=DE_RANDOM,
                 device=0, generation="keyed", driver="turns", params=None):
        if generation not in ("keyed", "reference"):
            raise ValueError(f"generation must be 'keyed' or 'reference', not {generation!r}")
        if driver not in ("turns", "resident"):
            raise ValueError(f"driver must be 'turns' or 'resident', not {driver!r}")
        if driver == "resident" and generation == "reference":
            raise ValueError("driver='resident' runs the keyed generation: it cannot be combined with "
                             "generation='reference'")
        self.driver, self.driver_used = driver, None
        self.n_params = f.n_params if isinstance(f, CustomObjective) else 0
        if self.n_params and generation == "reference":
            raise ValueError("an objective with run-time parameters runs the keyed generation on the "
                             "resident engine: it cannot be combined with generation='reference'")
        if (params is not None) != bool(self.n_params):
            raise ValueError("params= goes with a CustomObjective whose n_params > 0, and such an "
                             "objective needs it")
        self.params = None if params is None else _params_rows(params, 1, self.n_params)
        if generation == "reference" and not isinstance(generator, XorShift):
            raise TypeError("generation='reference' draws from the caller's stream: generator must be an "
                            "nlsolver_amd.XorShift")
        self.f, self.generator, self.generation = f, generator, generation
        self.args = dict(CR=crossover_prob, F=differential_weight, eps=eps, max_iter=max_iter,
                         best_val_no_change=best_val_no_change, strategy=strategy, device=device)
        self.pop_size = pop_size

    def _solve(self, x, minimize):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim != 1:
            raise TypeError("x must be a 1-D float64 numpy array (it is updated in place, "
                            "like std::vector<T>& in nlsolver.h:2404)")
        if self.generation == "reference":
            with DERefEngine(self.f, 1, self.pop_size, x.size, minimize=minimize, **self.args) as eng:
                xo, st, states = eng.minimize(x[None, :], [self.generator.state])
            x[:] = xo[0]
            self.generator.state = tuple(int(v) for v in states[0])
            return st[0]
        seed = seed_from_generator(self.generator)
        if self.n_params and not DEBatchEngine.fits(self.pop_size, x.size, self.n_params):
            raise NlsgError(_capi.NLSG_ERR_UNSUPPORTED,
                            f"an objective with run-time parameters needs the resident engine, and pop "
                            f"{self.pop_size} x dim {x.size} with {self.n_params} parameters does not "
                            f"fit its {LDS_BUDGET} bytes of LDS")
        if self.n_params or (self.driver == "resident" and self._resident_fits(x.size)):
            with DEBatchEngine(self.f, 1, self.pop_size, x.size, minimize=minimize, **self.args) as eng:
                xo, st = eng.minimize(x[None, :], [seed], params=self.params)
            x[:] = xo[0]
            self.driver_used = "resident"
            return st[0]
        self.driver_used = "turns"
        with DEEngine(self.f, self.pop_size, x.size, minimize=minimize, seed=seed,
                      **self.args) as eng:
            return eng.minimize(x)

    def _resident_fits(self, dim):
        try:
            return DEBatchEngine.fits(self.pop_size, dim)
        except NlsgError:  # a library without the resident engine: the turn engine solves
            return False

    def minimize(self, x):
        return self._solve(x, True)

    def maximize(self, x):
        return self._solve(x, False)


DESolver = DE  # README.md:80 alias
