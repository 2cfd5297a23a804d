"""Host-side mirror of the reference's SANN class for device objectives, batched.

Reference interface (nlsolver.h:2744-2775):
    SANN<Callable, RNG, scalar_t>(f, generator, max_iter = 5000, temperature_iter = 10,
        temperature_max = 10.0)
    minimize(x) / maximize(x)
x may be (n,) or (batch, n): independent chains, one per GPU wave. The generator only seeds the
chains: draws are keyed by (seed, chain, step, slot) on the device (oracle: orc_sann_sync).

A CustomObjective with n_params > 0 (nlsg_sann_create_params): chain b anneals the objective under
row b of set_params(rows) ([batch, n_params], read as p(k)); rows are replaced without recompiling.
"""
import ctypes as C  # noqa: F401 - names the module had before _engine.py stay importable from it

import numpy as np

from ._capi import NlsgError, SANNConfig, Status, check, lib, require  # noqa: F401
from ._engine import DEFAULT_SEED, Engine, _rows_for_batch, pair_params, pd_of, seed_from_generator, timed_ms


class SANNEngine(Engine):
    _destroy, _set_params = "nlsg_sann_destroy", "nlsg_sann_set_params"

    @staticmethod
    def chains_per_wave(dim, n_params=0):
        """chains that share a wave at this shape: 64 / G for dim <= 64 while the parameter rows of the
        block's lane groups fit in LDS, else 1 (the results do not depend on it; host only)"""
        return int(require("nlsg_sann_chains_per_wave")(dim, n_params))

    @staticmethod
    def lds_bytes(dim, n_params=0):
        """dynamic LDS bytes of a launch: the parameter rows (host only)"""
        return int(require("nlsg_sann_lds_bytes")(dim, n_params))

    def __init__(self, objective, batch, dim, *, minimize=True, max_iter=5000, temperature_iter=10,
                 temperature_max=10.0, seed=DEFAULT_SEED, chain_lo=0, device=0, stream=None):
        cfg = self._header(SANNConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize = int(bool(minimize))
        cfg.batch, cfg.dim, cfg.chain_lo = batch, dim, chain_lo
        cfg.max_iter, cfg.temperature_iter = max_iter, temperature_iter
        cfg.temperature_max, cfg.seed = temperature_max, seed
        self.n_params = custom.n_params if custom else 0
        if custom:
            self._create_custom(self._creator(lib().nlsg_sann_create_custom, "nlsg_sann_create_params"), cfg, custom)
        else:
            self._create(lib().nlsg_sann_create, cfg)

    def minimize(self, x, params=None):
        """x: (batch, dim) starts; returns (best points, [Status]). params: set_params(params) first."""
        self._apply_params(params)
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        assert x.shape == (self.cfg.batch, self.cfg.dim)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_sann_minimize(self._h, pd_of(x), st))
        return x, list(st)

    def time_solve(self, x0, repeats=1, params=None):
        self._apply_params(params)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        return timed_ms(lib().nlsg_sann_time_solve, self._h, pd_of(x0), repeats)


class SANN:
    """Drop-in for nlsolver::SANN on a device objective (same ctor args and defaults).

    params: the run-time parameters of a CustomObjective with n_params > 0: one row (n_params,) shown
    to every chain, or (batch, n_params) with a 2-D x, a row per chain."""

    def __init__(self, f, generator=None, max_iter=5000, temperature_iter=10, temperature_max=10.0,
                 *, device=0, params=None):
        self.n_params, self.params = pair_params(f, params)
        self.f, self.generator = f, generator
        self.args = dict(max_iter=max_iter, temperature_iter=temperature_iter,
                         temperature_max=temperature_max, device=device)

    def _solve(self, x, minimize):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim not in (1, 2):
            raise TypeError("x must be a float64 numpy array of shape (n,) or (batch, n)")
        xb = x.reshape(1, -1) if x.ndim == 1 else x
        rows = _rows_for_batch(self.params, xb.shape[0])
        with SANNEngine(self.f, xb.shape[0], xb.shape[1], minimize=minimize,
                        seed=seed_from_generator(self.generator), **self.args) as eng:
            out, st = eng.minimize(xb, params=rows)
        xb[...] = out
        return st[0] if x.ndim == 1 else st

    def minimize(self, x):
        return self._solve(x, True)

    def maximize(self, x):
        return self._solve(x, False)
