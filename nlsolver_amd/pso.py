"""Host-side mirror of the reference's PSO class for device objectives.

Reference interface (nlsolver.h:2498-2591):
    PSO<Callable, RNG, scalar_t, PSOType>(f, generator, inertia=0.8, cognitive_coef=1.8,
        social_coef=1.8, n_particles=10, max_iter=5000, best_val_no_change=50, eps=10e-4)
    minimize(x) / maximize(x)                       bounds = -+|x_i| (2553-2575)
    minimize(x, lower, upper) / maximize(x, lower, upper)   (note: lower first, 2577-2591)
Same positional arguments and defaults here. All compute runs in libnlsolver_hip.so.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (PSO_ACCELERATED, PSO_VANILLA, NlsgError, PSOBatchConfig, PSOConfig, Status, check, lib,
                    require)
from ._engine import (DEFAULT_SEED, LDS_BUDGET, Engine, _params_rows, _with_params_lds, check_driver, pair_params,
                      pd_of, pu_of, seed_from_generator, seeds_u64, timed_ms)


class PSOEngine(Engine):
    """RAII wrapper over the nlsg_pso_* C-ABI."""
    _destroy = "nlsg_pso_destroy"

    def __init__(self, objective, n_particles, dim, *, type=PSO_VANILLA, bounded=False,
                 minimize=True, inertia=0.8, cognitive=1.8, social=1.8, eps=10e-4, max_iter=5000,
                 best_val_no_change=50, seed=DEFAULT_SEED, device=0, stream=None, shard_lo=0,
                 shard_n=None):
        cfg = self._header(PSOConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize, cfg.type, cfg.bounded = int(bool(minimize)), type, int(bool(bounded))
        cfg.n_particles, cfg.dim = n_particles, dim
        cfg.shard_lo = shard_lo
        cfg.shard_n = n_particles if shard_n is None else shard_n
        cfg.inertia, cfg.cognitive, cfg.social, cfg.eps = inertia, cognitive, social, eps
        cfg.max_iter, cfg.best_val_no_change, cfg.seed = max_iter, best_val_no_change, seed
        if custom:  # (its n_params goes through: the C side refuses an objective with parameters)
            self._create_custom(lib().nlsg_pso_create_custom, cfg, custom)
        else:
            self._create(lib().nlsg_pso_create, cfg)

    def _bounds(self, lower, upper):
        D = self.cfg.dim
        lo = np.ascontiguousarray(np.broadcast_to(lower, (D,)), dtype=np.float64)
        hi = np.ascontiguousarray(np.broadcast_to(upper, (D,)), dtype=np.float64)
        return lo, hi

    def init(self, lower, upper):
        lo, hi = self._bounds(lower, upper)
        check(lib().nlsg_pso_init(self._h, pd_of(lo), pd_of(hi)))

    def step(self, turns=1):
        check(lib().nlsg_pso_step(self._h, turns))

    def status(self):
        st = Status()
        check(lib().nlsg_pso_status(self._h, C.byref(st)))
        return st

    def best(self):
        x = np.empty(self.cfg.dim)
        f, idx = C.c_double(), C.c_uint64()
        check(lib().nlsg_pso_best(self._h, pd_of(x), C.byref(f), C.byref(idx)))
        return x, f.value, idx.value

    def download(self):
        n, D = self.cfg.shard_n, self.cfg.dim
        vanilla = self.cfg.type == PSO_VANILLA
        pos, vel = np.empty((n, D)), (np.empty((n, D)) if vanilla else None)
        pbest, cur = np.empty(n), np.empty(n)
        check(lib().nlsg_pso_download(self._h, pd_of(pos), pd_of(vel), pd_of(pbest), pd_of(cur)))
        return pos, vel, pbest, cur

    def minimize(self, x, lower, upper, poll_every=0):
        lo, hi = self._bounds(lower, upper)
        st = Status()
        check(lib().nlsg_pso_minimize(self._h, pd_of(x), pd_of(lo), pd_of(hi), poll_every, C.byref(st)))
        return st

    def time_move_kernel(self, launches):
        return timed_ms(lib().nlsg_pso_time_move_kernel, self._h, launches)

    def record_doubles(self):
        return lib().nlsg_pso_record_doubles(self._h)

    def turn_begin(self, send_dev_ptr):
        check(lib().nlsg_pso_turn_begin(self._h, send_dev_ptr))

    def turn_end(self, gathered_dev_ptr, world):
        check(lib().nlsg_pso_turn_end(self._h, gathered_dev_ptr, world))

    def comm_attach(self, unique_id, world, rank):
        """Collective: joins the library-side RCCL communicator (see nlsolver_amd.dist)."""
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        check(lib().nlsg_pso_comm_attach(self._h, buf, world, rank))

    def step_sharded(self, turns=1):
        check(lib().nlsg_pso_step_sharded(self._h, turns))

    def comm_ranks(self):
        """(world, rank) as the attached RCCL communicator reports them."""
        w, r = C.c_int32(), C.c_int32()
        check(lib().nlsg_pso_comm_ranks(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value


class PSOBatchEngine(Engine):
    """Resident batch PSO (nlsg_pso_batch_*): `batch` independent solves of the keyed engine of one
    shape, each with its own 64-bit seed and its own bounds, one workgroup per solve with the swarm
    in LDS and the whole turn loop inside one kernel. Solve b is bit-identical to
    PSOEngine(objective, n_particles, dim, seed=seeds[b], ...) driven by the same calls with
    lower[b], upper[b]; it ends independently of its neighbours. 1 <= n_particles <= 1024,
    1 <= dim <= 128 and lds_bytes(n_particles, dim, type) within LDS_BUDGET, else NlsgError
    (code 2): there is no global-memory fallback.

    set_params: values already stored are not re-evaluated, so call init / minimize afterwards to
    solve under the new rows."""
    _destroy, _set_params = "nlsg_pso_batch_destroy", "nlsg_pso_batch_set_params"

    @staticmethod
    def lds_bytes(n_particles, dim, type=PSO_VANILLA, n_params=0):
        """LDS bytes a solve of this shape needs, the row of n_params objective parameters
        included; 0 outside the ranges (host only)"""
        need = int(require("nlsg_pso_batch_lds_bytes")(n_particles, dim, type))
        return _with_params_lds(need, n_params)

    @staticmethod
    def fits(n_particles, dim, type=PSO_VANILLA, n_params=0):
        need = PSOBatchEngine.lds_bytes(n_particles, dim, type, n_params)
        return 0 < need <= LDS_BUDGET

    def __init__(self, objective, batch, n_particles, dim, *, type=PSO_VANILLA, bounded=False,
                 minimize=True, inertia=0.8, cognitive=1.8, social=1.8, eps=10e-4, max_iter=5000,
                 best_val_no_change=50, turns_per_launch=0, device=0, stream=None):
        cfg = self._header(PSOBatchConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize, cfg.type, cfg.bounded = int(bool(minimize)), type, int(bool(bounded))
        cfg.batch, cfg.n_particles, cfg.dim = batch, n_particles, dim
        cfg.inertia, cfg.cognitive, cfg.social, cfg.eps = inertia, cognitive, social, eps
        cfg.max_iter, cfg.best_val_no_change = max_iter, best_val_no_change
        cfg.turns_per_launch = turns_per_launch
        self.n_params = custom.n_params if custom else 0
        if custom:
            self._create_custom(self._creator(require("nlsg_pso_batch_create_custom")), cfg, custom)
        else:
            self._create(require("nlsg_pso_batch_create"), cfg)

    def _inputs(self, lower, upper, seeds):
        """lower / upper: anything that broadcasts to [batch, dim]; seeds [batch]"""
        B, D = self.cfg.batch, self.cfg.dim
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), (B, D)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (B, D)))
        return lo, hi, seeds_u64(seeds, B)

    def init(self, lower, upper, seeds):
        """PSOEngine.init of every solve under its own seed and bounds"""
        lo, hi, seeds = self._inputs(lower, upper, seeds)
        check(lib().nlsg_pso_batch_init(self._h, pd_of(lo), pd_of(hi), pu_of(seeds)))

    def step(self, turns=1):
        check(lib().nlsg_pso_batch_step(self._h, turns))

    def status(self):
        """[Status] * batch, each what PSOEngine.status() returns after the same calls"""
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_pso_batch_status(self._h, st))
        return list(st)

    def best(self):
        """(x [batch, dim], f [batch], index [batch]): every solve's swarm best"""
        B, D = self.cfg.batch, self.cfg.dim
        x, f, idx = np.empty((B, D)), np.empty(B), np.empty(B, dtype=np.uint64)
        check(lib().nlsg_pso_batch_best(self._h, pd_of(x), pd_of(f), pu_of(idx)))
        return x, f, idx

    def download(self, b):
        """(pos, vel or None, pbest_val, cur_val) of solve b, as PSOEngine.download()"""
        n, D = self.cfg.n_particles, self.cfg.dim
        vanilla = self.cfg.type == PSO_VANILLA
        pos, vel = np.empty((n, D)), (np.empty((n, D)) if vanilla else None)
        pbest, cur = np.empty(n), np.empty(n)
        check(lib().nlsg_pso_batch_download(self._h, b, pd_of(pos), pd_of(vel), pd_of(pbest), pd_of(cur)))
        return pos, vel, pbest, cur

    def minimize(self, lower, upper, seeds, params=None):
        """init, then turns until every solve is done -> (x [batch, dim], [Status] * batch).
        params: set_params(params) first."""
        self._apply_params(params)
        lo, hi, seeds = self._inputs(lower, upper, seeds)
        x = np.empty((self.cfg.batch, self.cfg.dim))
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_pso_batch_minimize(self._h, pd_of(x), pd_of(lo), pd_of(hi), pu_of(seeds), st))
        return x, list(st)

    def time_solve(self, lower, upper, seeds, repeats=1, params=None):
        """milliseconds of `repeats` whole solves (hipEvents). params: set_params(params) first."""
        self._apply_params(params)
        lo, hi, seeds = self._inputs(lower, upper, seeds)
        return timed_ms(lib().nlsg_pso_batch_time_solve, self._h, pd_of(lo), pd_of(hi), pu_of(seeds), repeats)


class PSO:
    """Drop-in for nlsolver::PSO on a device objective (same ctor args/defaults/overloads).

    driver="resident": the solve runs through a batch-1 PSOBatchEngine -- the whole turn loop in one
    kernel instead of up to seven launches per turn -- when the swarm fits a workgroup's LDS
    (PSOBatchEngine.fits), through PSOEngine otherwise; the bits are the same either way.
    `driver_used` says which engine the last solve ran on. Default "turns": PSOEngine.

    params: the one row of run-time parameters of a CustomObjective with n_params > 0. Such an
    objective always runs through the resident engine (the only one that takes parameters),
    whatever `driver` says; a shape that does not fit there is NlsgError code 2."""

    def __init__(self, f, generator=None, inertia=0.8, cognitive_coef=1.8, social_coef=1.8,
                 n_particles=10, max_iter=5000, best_val_no_change=50, eps=10e-4, *,
                 type=PSO_VANILLA, device=0, driver="turns", params=None):
        check_driver(driver)
        self.driver, self.driver_used = driver, None
        self.n_params, self.params = pair_params(f, params, lambda p, n: _params_rows(p, 1, n))
        self.f, self.generator, self.n_particles = f, generator, n_particles
        self.args = dict(inertia=inertia, cognitive=cognitive_coef, social=social_coef, eps=eps,
                         max_iter=max_iter, best_val_no_change=best_val_no_change, type=type,
                         device=device)

    def _solve(self, x, lower, upper, minimize):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim != 1:
            raise TypeError("x must be a 1-D float64 numpy array (updated in place)")
        bounded = lower is not None
        if not bounded:  # nlsolver.h:2553-2560: lower = -|x|, upper = |x|
            lower, upper = -np.abs(x), np.abs(x)
        seed = seed_from_generator(self.generator)
        if self.n_params and not PSOBatchEngine.fits(self.n_particles, x.size, self.args["type"],
                                                     self.n_params):
            raise NlsgError(_capi.NLSG_ERR_UNSUPPORTED,
                            f"an objective with run-time parameters needs the resident engine, and "
                            f"{self.n_particles} particles x dim {x.size} with {self.n_params} parameters "
                            f"do not fit its {LDS_BUDGET} bytes of LDS")
        if self.n_params or (self.driver == "resident" and self._resident_fits(x.size)):
            with PSOBatchEngine(self.f, 1, self.n_particles, x.size, bounded=bounded, minimize=minimize,
                                **self.args) as eng:
                xo, st = eng.minimize(lower, upper, [seed], params=self.params)
            x[:] = xo[0]
            self.driver_used = "resident"
            return st[0]
        self.driver_used = "turns"
        with PSOEngine(self.f, self.n_particles, x.size, bounded=bounded, minimize=minimize,
                       seed=seed, **self.args) as eng:
            return eng.minimize(x, lower, upper)

    def _resident_fits(self, dim):
        try:
            return PSOBatchEngine.fits(self.n_particles, dim, self.args["type"])
        except NlsgError:  # a library without the resident engine: the turn engine solves
            return False

    def minimize(self, x, lower=None, upper=None):
        return self._solve(x, lower, upper, True)

    def maximize(self, x, lower=None, upper=None):
        return self._solve(x, lower, upper, False)


PSOSolver = PSO  # README.md:99 alias
