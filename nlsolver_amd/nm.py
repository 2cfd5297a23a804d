"""Host-side mirror of the reference's NelderMead class for device objectives, batched.

Reference interface (nlsolver.h:2099-2165):
    NelderMead<Callable, scalar_t>(f, step = -1, alpha = 1, gamma = 2, rho = 0.5, sigma = 0.5,
        eps = 1e-6, max_iter = 500, no_change_best_tol = 20, restarts = 0)
    minimize(x) / maximize(x) / minimize(x, upper, lower) / maximize(x, upper, lower)
(upper before lower — the opposite of PSO). x may be (n,) or (batch, n): independent starts,
one simplex per GPU workgroup.
"""
import ctypes as C  # noqa: F401 - names the module had before _engine.py stay importable from it

import numpy as np

from . import _capi
from ._capi import NMConfig, NlsgError, Status, check, lib, require  # noqa: F401
from ._engine import (LDS_BUDGET, CustomObjective, Engine, _drop_in_rows, _rows_for_batch, _with_params_lds,  # noqa: F401
                      pair_params, pd_of, pu_of, timed_ms)


class NMEngine(Engine):
    """reference_order=True (NLSG_NM_REFERENCE_ORDER): the objective's terms and std_err's sums in index
    order, as the reference adds them — its own runs bit for bit at every dimension (the lane-tree sums
    can break a tie between two vertices the other way: same algorithm, another branch).

    A CustomObjective with n_params > 0 (nlsg_nm_create_params): start b minimises the objective under
    row b of set_params(rows) ([batch, n_params], read as p(k)); rows are replaced without recompiling.
    The row lives in the workgroup's LDS in front of the simplex: fits() says whether a shape has room."""
    _destroy, _set_params = "nlsg_nm_destroy", "nlsg_nm_set_params"

    @staticmethod
    def lds_bytes(dim, reference_order=False, n_params=0):
        """LDS bytes a start's workgroup needs at the least (in reference order: with one term buffer),
        the row of n_params objective parameters included; 0 outside the ranges (host only)"""
        need = int(require("nlsg_nm_lds_bytes")(dim, _capi.NM_REFERENCE_ORDER if reference_order else 0))
        return _with_params_lds(need, n_params)

    @staticmethod
    def fits(dim, reference_order=False, n_params=0):
        return 0 < NMEngine.lds_bytes(dim, reference_order, n_params) <= LDS_BUDGET

    def __init__(self, objective, batch, dim, *, minimize=True, bounded=False, step=-1.0, alpha=1.0,
                 gamma=2.0, rho=0.5, sigma=0.5, eps=1e-6, max_iter=500, no_change_best_tol=20,
                 restarts=0, device=0, stream=None, reference_order=False):
        cfg = self._header(NMConfig, device, stream)
        cfg.flags = _capi.NM_REFERENCE_ORDER if reference_order else 0
        cfg.objective, custom = self._objective_id(objective)
        cfg.minimize, cfg.bounded = int(bool(minimize)), int(bool(bounded))
        cfg.batch, cfg.dim = batch, dim
        cfg.step, cfg.alpha, cfg.gamma, cfg.rho, cfg.sigma, cfg.eps = step, alpha, gamma, rho, sigma, eps
        cfg.max_iter, cfg.no_change_best_tol, cfg.restarts = max_iter, no_change_best_tol, restarts
        self.n_params = custom.n_params if custom else 0
        if custom:
            self._create_custom(self._creator(lib().nlsg_nm_create_custom, "nlsg_nm_create_params"), cfg, custom)
        else:
            self._create(lib().nlsg_nm_create, cfg)

    def minimize(self, x, upper=None, lower=None, params=None):
        """params: set_params(params) first."""
        self._apply_params(params)
        B, n = self.cfg.batch, self.cfg.dim
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (B, n)
        up = lo = None
        if self.cfg.bounded:
            up = np.ascontiguousarray(np.broadcast_to(upper, (n,)), dtype=np.float64)
            lo = np.ascontiguousarray(np.broadcast_to(lower, (n,)), dtype=np.float64)
        st = (Status * B)()
        eps = np.empty(B)
        check(lib().nlsg_nm_minimize(self._h, pd_of(x), pd_of(up), pd_of(lo), st, pd_of(eps)))
        return x, list(st), eps

    def phase_cycles(self, x0):
        """One solve with the kernel's phase counters on: (batch, 8) shader-clock cycles per phase
        (scan, centroid, reflection, expansion / contraction, shrink, -, iterations, shrinks)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        out = np.zeros((self.cfg.batch, 8), dtype=np.uint64)
        check(lib().nlsg_nm_phase_cycles(self._h, pd_of(x0), pu_of(out)))
        return out

    def time_solve(self, x0, repeats=1, params=None):
        self._apply_params(params)
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        return timed_ms(lib().nlsg_nm_time_solve, self._h, pd_of(x0), repeats)


class NelderMead:
    """Drop-in for nlsolver::NelderMead on a device objective (same ctor args/defaults).
    reference_order=None: reference order (NMEngine) wherever the reference's arithmetic exists on the
    device — Rosenbrock / Sphere / Styblinski-Tang, a custom objective given by its terms —: the
    reference's runs bit for bit. True / False force it.

    params: the run-time parameters of a CustomObjective with n_params > 0: one row (n_params,) shown
    to every start, or (batch, n_params) with a 2-D x, a row per start."""

    def __init__(self, f, step=-1.0, alpha=1.0, gamma=2.0, rho=0.5, sigma=0.5, eps=1e-6,
                 max_iter=500, no_change_best_tol=20, restarts=0, *, device=0, reference_order=None,
                 params=None):
        self.n_params, self.params = pair_params(f, params)
        if reference_order is None:
            reference_order = (isinstance(f, str) and f in ("rosenbrock", "sphere", "styblinski_tang")) or \
                (isinstance(f, CustomObjective) and f.chain != 2)
        self.reference_order = bool(reference_order)
        self.f = f
        self.eps = eps  # mutated by every solve like the reference's member (nlsolver.h:2189)
        self.args = dict(step=step, alpha=alpha, gamma=gamma, rho=rho, sigma=sigma,
                         max_iter=max_iter, no_change_best_tol=no_change_best_tol,
                         restarts=restarts, device=device)

    def _solve(self, x, upper, lower, minimize):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim not in (1, 2):
            raise TypeError("x must be a float64 numpy array of shape (n,) or (batch, n)")
        xb = x.reshape(1, -1) if x.ndim == 1 else x
        bounded = upper is not None
        rows = _rows_for_batch(self.params, xb.shape[0])
        with NMEngine(self.f, xb.shape[0], xb.shape[1], minimize=minimize, bounded=bounded,
                      eps=self.eps, reference_order=self.reference_order, **self.args) as eng:
            out, st, eps = eng.minimize(xb, upper, lower, params=rows)
        xb[...] = out
        if x.ndim == 1:
            self.eps = float(eps[0])
            return st[0]
        return st

    def minimize(self, x, upper=None, lower=None):
        return self._solve(x, upper, lower, True)

    def maximize(self, x, upper=None, lower=None):
        return self._solve(x, upper, lower, False)
