"""Host-side mirror of the reference's NelderMeadPSO class for device objectives, batched.

Reference interface (nlsolver.h:3546-3620):
    NelderMeadPSO<Callable, RNG, scalar_t>(f, generator, alpha = 1, gamma = 2, rho = 0.5,
        sigma = 0.5, inertia = 0.8, cognitive_coef = 1.8, social_coef = 1.8, eps = 1e-6,
        max_iter = 1000, no_change_best_iter = 20)
    minimize(x) / maximize(x) / minimize(x, lower, upper) / maximize(x, lower, upper)
(lower before upper, like PSO). x may be (n,) or (batch, n): independent instances, one GPU
workgroup each. The generator only seeds the instances (draws are keyed on the device).
"""
import ctypes as C  # noqa: F401 - names the module had before _engine.py stay importable from it

import numpy as np

from ._capi import NMPSOConfig, NlsgError, Status, check, lib, require  # noqa: F401
from ._engine import (DEFAULT_SEED, LDS_BUDGET, Engine, _rows_for_batch, _with_params_lds, pair_params, pd_of,
                      seed_from_generator, timed_ms)


class NMPSOEngine(Engine):
    """A CustomObjective with n_params > 0 (nlsg_nmpso_create_params): instance b minimises the
    objective under row b of set_params(rows) ([batch, n_params], read as p(k)); rows are replaced
    without recompiling. The row lives in the workgroup's LDS: fits() says whether a shape has room."""
    _destroy, _set_params = "nlsg_nmpso_destroy", "nlsg_nmpso_set_params"

    @staticmethod
    def lds_bytes(dim, n_params=0):
        """LDS bytes of an instance's workgroup, the row of n_params objective parameters included;
        0 outside the ranges (host only)"""
        return _with_params_lds(int(require("nlsg_nmpso_lds_bytes")(dim)), n_params)

    @staticmethod
    def fits(dim, n_params=0):
        return 0 < NMPSOEngine.lds_bytes(dim, n_params) <= LDS_BUDGET

    def __init__(self, objective, batch, dim, *, minimize=True, bounded=False, alpha=1.0, gamma=2.0,
                 rho=0.5, sigma=0.5, inertia=0.8, cognitive=1.8, social=1.8, eps=1e-6, max_iter=1000,
                 no_change_best_iter=20, seed=DEFAULT_SEED, inst_lo=0, device=0, stream=None):
        cfg = self._header(NMPSOConfig, device, stream)
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize, cfg.bounded = int(bool(minimize)), int(bool(bounded))
        cfg.batch, cfg.dim, cfg.inst_lo = batch, dim, inst_lo
        cfg.alpha, cfg.gamma, cfg.rho, cfg.sigma = alpha, gamma, rho, sigma
        cfg.inertia, cfg.cognitive, cfg.social, cfg.eps = inertia, cognitive, social, eps
        cfg.max_iter, cfg.no_change_best_iter, cfg.seed = max_iter, no_change_best_iter, seed
        self.n_params = custom.n_params if custom else 0
        if custom:
            self._create_custom(self._creator(lib().nlsg_nmpso_create_custom, "nlsg_nmpso_create_params"), cfg,
                                custom)
        else:
            self._create(lib().nlsg_nmpso_create, cfg)

    def minimize(self, x, lower=None, upper=None, params=None):
        """x: (batch, dim) starts; returns (best particles, [Status]). params: set_params(params) first."""
        self._apply_params(params)
        n = self.cfg.dim
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        assert x.shape == (self.cfg.batch, n)
        lo = up = None
        if self.cfg.bounded:
            lo = np.ascontiguousarray(np.broadcast_to(lower, (n,)), dtype=np.float64)
            up = np.ascontiguousarray(np.broadcast_to(upper, (n,)), dtype=np.float64)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_nmpso_minimize(self._h, pd_of(x), pd_of(lo), pd_of(up), st))
        return x, list(st)

    def time_solve(self, x0, repeats=1, params=None):
        self._apply_params(params)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        return timed_ms(lib().nlsg_nmpso_time_solve, self._h, pd_of(x0), repeats)


class NelderMeadPSO:
    """Drop-in for nlsolver::NelderMeadPSO on a device objective (same ctor args and defaults).

    params: the run-time parameters of a CustomObjective with n_params > 0: one row (n_params,) shown
    to every instance, or (batch, n_params) with a 2-D x, a row per instance."""

    def __init__(self, f, generator=None, alpha=1.0, gamma=2.0, rho=0.5, sigma=0.5, inertia=0.8,
                 cognitive_coef=1.8, social_coef=1.8, eps=1e-6, max_iter=1000,
                 no_change_best_iter=20, *, device=0, params=None):
        self.n_params, self.params = pair_params(f, params)
        self.f, self.generator = f, generator
        self.args = dict(alpha=alpha, gamma=gamma, rho=rho, sigma=sigma, inertia=inertia,
                         cognitive=cognitive_coef, social=social_coef, eps=eps, max_iter=max_iter,
                         no_change_best_iter=no_change_best_iter, device=device)

    def _solve(self, x, lower, upper, minimize):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim not in (1, 2):
            raise TypeError("x must be a float64 numpy array of shape (n,) or (batch, n)")
        xb = x.reshape(1, -1) if x.ndim == 1 else x
        if xb.shape[1] < 2:  # nlsolver.h:3627-3637: refused, "some invalid solver state"
            st = Status()
            st.f_value = 999999
            return st if x.ndim == 1 else [st] * xb.shape[0]
        rows = _rows_for_batch(self.params, xb.shape[0])
        with NMPSOEngine(self.f, xb.shape[0], xb.shape[1], minimize=minimize,
                         bounded=lower is not None, seed=seed_from_generator(self.generator),
                         **self.args) as eng:
            out, st = eng.minimize(xb, lower, upper, params=rows)
        xb[...] = out
        return st[0] if x.ndim == 1 else st

    def minimize(self, x, lower=None, upper=None):
        return self._solve(x, lower, upper, True)

    def maximize(self, x, lower=None, upper=None):
        return self._solve(x, lower, upper, False)
