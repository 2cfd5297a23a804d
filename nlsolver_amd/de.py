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
from ._engine import (DEFAULT_SEED, LDS_BUDGET, CustomObjective, Engine, _params_rows, _with_params_lds,  # noqa: F401
                      check_driver, pair_params, pd_of, pu_of, rtc_library_path, seed_from_generator, seeds_u64,
                      timed_ms)
from .rng import XorShift


class DEEngine(Engine):
    """Thin RAII wrapper over the nlsg_de_* C-ABI (one handle, one device, one stream)."""
    _destroy = "nlsg_de_destroy"

    def __init__(self, objective, pop, dim, *, minimize=True, strategy=DE_RANDOM, CR=0.9, F=0.8,
                 eps=10e-4, max_iter=1000, best_val_no_change=50, seed=DEFAULT_SEED, device=0,
                 stream=None, shard_lo=0, shard_n=None, trace=False):
        cfg = self._header(DEConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize = int(bool(minimize))
        cfg.strategy = strategy
        cfg.trace = int(bool(trace))
        cfg.pop, cfg.dim = pop, dim
        cfg.shard_lo = shard_lo
        cfg.shard_n = pop if shard_n is None else shard_n
        cfg.CR, cfg.F, cfg.eps = CR, F, eps
        cfg.max_iter, cfg.best_val_no_change, cfg.seed = max_iter, best_val_no_change, seed
        if custom:  # (its n_params goes through: the C side refuses an objective with parameters)
            self._create_custom(lib().nlsg_de_create_custom, cfg, custom)
        else:
            self._create(lib().nlsg_de_create, cfg)

    # -- C-ABI calls ------------------------------------------------------
    def init(self, x0):
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        if x0.shape != (self.cfg.dim,):
            raise ValueError(f"x0 must have {self.cfg.dim} entries")
        check(lib().nlsg_de_init(self._h, pd_of(x0)))

    def step(self, turns=1):
        check(lib().nlsg_de_step(self._h, turns))

    def status(self):
        st = Status()
        check(lib().nlsg_de_status(self._h, C.byref(st)))
        return st

    def best(self):
        x = np.empty(self.cfg.dim)
        f, idx = C.c_double(), C.c_uint64()
        check(lib().nlsg_de_best(self._h, pd_of(x), C.byref(f), C.byref(idx)))
        return x, f.value, idx.value

    def download(self, trace=False):
        n, D = self.cfg.shard_n, self.cfg.dim
        pop, scores = np.empty((n, D)), np.empty(n)
        tr = np.empty((n, 5), dtype=np.uint64) if trace else None
        check(lib().nlsg_de_download(self._h, pd_of(pop), pd_of(scores), pu_of(tr)))
        return (pop, scores, tr) if trace else (pop, scores)

    def upload(self, pop, scores):
        pop = np.ascontiguousarray(pop, dtype=np.float64)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        assert pop.shape == (self.cfg.shard_n, self.cfg.dim) and scores.shape == (self.cfg.shard_n,)
        check(lib().nlsg_de_upload(self._h, pd_of(pop), pd_of(scores)))

    def bound_counts(self):
        """(decided, fell through and rejected, accepted): agents since init() whose trial the
        generation's lower bound rejected unread / did not decide and selection rejected / did not
        decide (or had no kept coordinate) and selection accepted. Needs trace=True; all zero in
        an engine that does not use the bound (bound_state)."""
        out = np.zeros(3, dtype=np.uint64)
        check(require("nlsg_de_bound_counts")(self._h, pu_of(out)))
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
        check(require("nlsg_de_screen_counts")(self._h, pu_of(out)))
        return tuple(int(v) for v in out)

    def screen_state(self):
        """(enabled, retry period in generations) of the generation's half-row screen"""
        on, r = C.c_int32(), C.c_uint32()
        check(require("nlsg_de_screen_state")(self._h, C.byref(on), C.byref(r)))
        return bool(on.value), r.value

    def minimize(self, x, poll_every=0):
        st = Status()
        check(lib().nlsg_de_minimize(self._h, pd_of(x), poll_every, C.byref(st)))
        return st

    def time_generation_kernel(self, launches):
        return timed_ms(lib().nlsg_de_time_generation_kernel, self._h, launches)

    def time_turns(self, turns):
        return timed_ms(lib().nlsg_de_time_turns, self._h, turns)

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


class DERefEngine(Engine):
    """Reference-order DE (nlsg_de_ref_*): `batch` independent solves of the reference's own DE
    (nlsolver.h:2414-2476) — in-place asynchronous generation, every draw from the solve's own
    xorshift state — each returning the reference's x, status and final generator state bit for bit.
    `objective`: "rosenbrock", "sphere", "styblinski_tang" or a CustomObjective given by its terms."""
    _destroy = "nlsg_de_ref_destroy"

    def __init__(self, objective, batch, pop, dim, *, minimize=True, strategy=DE_RANDOM, CR=0.9,
                 F=0.8, eps=10e-4, max_iter=1000, best_val_no_change=50, log_capacity=0, device=0,
                 stream=None):
        cfg = self._header(DERefConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize, cfg.strategy = int(bool(minimize)), strategy
        cfg.batch, cfg.pop, cfg.dim = batch, pop, dim
        cfg.CR, cfg.F, cfg.eps = CR, F, eps
        cfg.max_iter, cfg.best_val_no_change, cfg.log_capacity = max_iter, best_val_no_change, log_capacity
        if custom:
            self._create_custom(require("nlsg_de_ref_create_custom"), cfg, custom)
        else:
            self._create(require("nlsg_de_ref_create"), cfg)

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
        check(lib().nlsg_de_ref_minimize(self._h, pd_of(x), pu_of(states), st))
        return x, list(st), states

    def log(self, b):
        """(xs [n, dim], fs [n], count) of solve b's last minimize: the evaluations in the
        reference's call order, n = min(count, log_capacity)"""
        n = C.c_uint64()
        check(lib().nlsg_de_ref_log(self._h, b, None, None, C.byref(n)))
        m = min(n.value, self.cfg.log_capacity)
        xs, fs = np.empty((m, self.cfg.dim)), np.empty(m)
        if m:
            check(lib().nlsg_de_ref_log(self._h, b, pd_of(xs), pd_of(fs), C.byref(n)))
        return xs, fs, n.value

    def time_solve(self, x0, states, repeats=1):
        """milliseconds of `repeats` whole solves from x0 / states (hipEvents)"""
        x0, states = self._inputs(x0, states)
        return timed_ms(lib().nlsg_de_ref_time_solve, self._h, pd_of(x0), pu_of(states), repeats)


class DEBatchEngine(Engine):
    """Resident batch DE (nlsg_de_batch_*): `batch` independent solves of the keyed engine of one
    shape, each with its own 64-bit seed and x0, one workgroup per solve with the population in LDS
    and the whole turn loop inside one kernel. Solve b is bit-identical to
    DEEngine(objective, pop, dim, seed=seeds[b], ...) driven by the same calls; it ends
    independently of its neighbours. 4 <= pop <= 1024, 1 <= dim <= 128 and lds_bytes(pop, dim)
    within LDS_BUDGET, else NlsgError (code 2): there is no global-memory fallback.

    set_params: scores already stored are not re-evaluated, so call init / minimize afterwards to
    solve under the new rows."""
    _destroy, _set_params = "nlsg_de_batch_destroy", "nlsg_de_batch_set_params"

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
        cfg = self._header(DEBatchConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize, cfg.strategy = int(bool(minimize)), strategy
        cfg.batch, cfg.pop, cfg.dim = batch, pop, dim
        cfg.CR, cfg.F, cfg.eps = CR, F, eps
        cfg.max_iter, cfg.best_val_no_change = max_iter, best_val_no_change
        cfg.turns_per_launch = turns_per_launch
        self.n_params = custom.n_params if custom else 0
        if custom:
            self._create_custom(self._creator(require("nlsg_de_batch_create_custom")), cfg, custom)
        else:
            self._create(require("nlsg_de_batch_create"), cfg)

    def _inputs(self, x0, seeds):
        B, D = self.cfg.batch, self.cfg.dim
        return np.array(x0, dtype=np.float64).reshape(B, D), seeds_u64(seeds, B)

    def init(self, x0, seeds):
        """x0 [batch, dim], seeds [batch]: DEEngine.init of every solve under its own seed"""
        x0, seeds = self._inputs(x0, seeds)
        check(lib().nlsg_de_batch_init(self._h, pd_of(x0), pu_of(seeds)))

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
        check(lib().nlsg_de_batch_best(self._h, pd_of(x), pd_of(f), pu_of(idx)))
        return x, f, idx

    def download(self, b):
        """(pop [pop, dim], scores [pop]) of solve b's current generation"""
        n, D = self.cfg.pop, self.cfg.dim
        pop, scores = np.empty((n, D)), np.empty(n)
        check(lib().nlsg_de_batch_download(self._h, b, pd_of(pop), pd_of(scores)))
        return pop, scores

    def upload(self, pops, scores):
        """overwrites the current generation of every solve: pops [batch, pop, dim], scores [batch, pop]"""
        B, n, D = self.cfg.batch, self.cfg.pop, self.cfg.dim
        pops = np.ascontiguousarray(pops, dtype=np.float64)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        assert pops.shape == (B, n, D) and scores.shape == (B, n)
        check(lib().nlsg_de_batch_upload(self._h, pd_of(pops), pd_of(scores)))

    def minimize(self, x, seeds, params=None):
        """init, then turns until every solve is done -> (x [batch, dim], [Status] * batch): new
        arrays, the inputs are kept. params: set_params(params) first."""
        self._apply_params(params)
        x, seeds = self._inputs(x, seeds)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_de_batch_minimize(self._h, pd_of(x), pu_of(seeds), st))
        return x, list(st)

    def time_solve(self, x0, seeds, repeats=1, params=None):
        """milliseconds of `repeats` whole solves from x0 / seeds (hipEvents). params:
        set_params(params) first."""
        self._apply_params(params)
        x0, seeds = self._inputs(x0, seeds)
        return timed_ms(lib().nlsg_de_batch_time_solve, self._h, pd_of(x0), pu_of(seeds), repeats)


def jump_table():
    """The nibble table of M^64 the reference-order engine advances its lanes with:
    uint64 [32, 16, 2] (entry (j, v) = xorshift128+ advanced 64 steps from the state whose nibble
    j is v; nibbles 0-15 of x[0], then 0-15 of x[1])."""
    t = np.empty((32, 16, 2), dtype=np.uint64)
    check(require("nlsg_de_ref_jump_table")(pu_of(t)))
    return t


def pick_donors(draws, fixed, pop):
    """The engine's generate_indices on given draws: (ids[4], draws used, flag) with flag 0,
    1 (an index >= pop: a draw of 1.0) or 2 (the 2^20-draw cap)."""
    d = np.ascontiguousarray(draws, dtype=np.float64)
    ids, used, flag = np.zeros(4, dtype=np.uint64), C.c_uint64(), C.c_int32()
    check(require("nlsg_de_ref_pick_donors")(pd_of(d), d.size, fixed, pop, pu_of(ids), C.byref(used),
                                             C.byref(flag)))
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
        check_driver(driver)
        if driver == "resident" and generation == "reference":
            raise ValueError("driver='resident' runs the keyed generation: it cannot be combined with "
                             "generation='reference'")
        self.driver, self.driver_used = driver, None
        if getattr(f, "n_params", 0) and generation == "reference":
            raise ValueError("an objective with run-time parameters runs the keyed generation on the "
                             "resident engine: it cannot be combined with generation='reference'")
        self.n_params, self.params = pair_params(f, params, lambda p, n: _params_rows(p, 1, n))
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
