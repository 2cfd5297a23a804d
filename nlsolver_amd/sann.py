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
import ctypes as C

import numpy as np

from . import _capi
from ._capi import NlsgError, SANNConfig, Status, check, lib, require
from .de import DEFAULT_SEED, seed_from_generator


class SANNEngine:
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
        cfg = SANNConfig()
        cfg.struct_size = C.sizeof(SANNConfig)
        cfg.device = device
        cfg.stream = None if stream is None else (stream or 1)
        from .de import CustomObjective, rtc_library_path
        custom = objective if isinstance(objective, CustomObjective) else None
        cfg.objective = (_capi.OBJ_CUSTOM if custom else
                         _capi.OBJECTIVES[objective] if isinstance(objective, str) else objective)
        cfg.minimize = int(bool(minimize))
        cfg.batch, cfg.dim, cfg.chain_lo = batch, dim, chain_lo
        cfg.max_iter, cfg.temperature_iter = max_iter, temperature_iter
        cfg.temperature_max, cfg.seed = temperature_max, seed
        self.cfg = cfg
        self.n_params = custom.n_params if custom else 0
        self._h = C.c_void_p()
        if custom:
            create = lib().nlsg_sann_create_custom
            if self.n_params:  # (zero stays with the creator it always had)
                create = require("nlsg_sann_create_params")
                require("nlsg_sann_set_params")
            check(lib().nlsg_rtc_load(rtc_library_path().encode()))
            obj = _capi.CustomObjectiveC(custom.term_body.encode(), custom.finish_body.encode(),
                                         int(custom.chain), self.n_params)
            check(create(C.byref(cfg), C.byref(obj), C.byref(self._h)))
        else:
            check(lib().nlsg_sann_create(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().nlsg_sann_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_params(self, params):
        """params [batch, n_params]: chain b's objective reads row b as p(k). The rows hold from the
        next solve on and can be replaced at any time without recompiling."""
        if self.n_params == 0:
            raise NlsgError(_capi.NLSG_ERR_INVALID_ARG, "the engine's objective declares no parameters")
        from .de import _params_rows
        rows = _params_rows(params, self.cfg.batch, self.n_params)
        check(require("nlsg_sann_set_params")(self._h, rows.ctypes.data_as(_capi.pd)))

    def minimize(self, x, params=None):
        """x: (batch, dim) starts; returns (best points, [Status]). params: set_params(params) first."""
        if params is not None:
            self.set_params(params)
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        assert x.shape == (self.cfg.batch, self.cfg.dim)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_sann_minimize(self._h, x.ctypes.data_as(_capi.pd), st))
        return x, list(st)

    def time_solve(self, x0, repeats=1, params=None):
        if params is not None:
            self.set_params(params)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        ms = C.c_float()
        check(lib().nlsg_sann_time_solve(self._h, x0.ctypes.data_as(_capi.pd), repeats, C.byref(ms)))
        return ms.value


class SANN:
    """Drop-in for nlsolver::SANN on a device objective (same ctor args and defaults).

    params: the run-time parameters of a CustomObjective with n_params > 0: one row (n_params,) shown
    to every chain, or (batch, n_params) with a 2-D x, a row per chain."""

    def __init__(self, f, generator=None, max_iter=5000, temperature_iter=10, temperature_max=10.0,
                 *, device=0, params=None):
        from .nm import _drop_in_rows
        self.n_params = getattr(f, "n_params", 0)
        if (params is not None) != bool(self.n_params):
            raise ValueError("params= goes with a CustomObjective whose n_params > 0, and such an "
                             "objective needs it")
        self.params = None if params is None else _drop_in_rows(params, self.n_params)
        self.f, self.generator = f, generator
        self.args = dict(max_iter=max_iter, temperature_iter=temperature_iter,
                         temperature_max=temperature_max, device=device)

    def _solve(self, x, minimize):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim not in (1, 2):
            raise TypeError("x must be a float64 numpy array of shape (n,) or (batch, n)")
        xb = x.reshape(1, -1) if x.ndim == 1 else x
        from .nm import _rows_for_batch
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
