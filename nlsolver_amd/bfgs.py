"""Host-side mirror of the reference's BFGS class for device objectives, batched.

Reference interface (nlsolver.h:3169-3196):
    BFGS<Callable, scalar_t, Grad>(f, g = fin_diff, max_iter = 100, grad_eps = 5e-3, alpha = 1)
    solver_status minimize(std::vector<T>& x)          (one start per call)
Here `f` is a device objective: QuadDiagRank1 with its analytic gradient, or the name of a
built-in objective ("rosenbrock", "sphere", "styblinski_tang", "rastrigin"), for which the
reference's DEFAULT gradient runs on the device (fin_diff = finite_difference_gradient<.,.,1>,
nlsolver.h:1385-1413: four probes per coordinate, each counted as a function call). minimize()
accepts one start (n,) or a batch of independent starts (batch, n) — BASELINE config 3 — solved
in lock step on the GPU, and returns one status per start.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import BFGSConfig, NlsgError, Status, check, lib, require
from ._engine import LDS_BUDGET, CustomObjective, Engine, _rows_for_batch, check_driver, pair_params, pd_of


class QuadDiagRank1:
    """f(x) = 1/2 sum d_i x_i^2 + 1/2 c (sum x)^2 - sum b_i x_i with its analytic gradient."""
    nlsg_objective = _capi.OBJ_QUAD_DIAG_RANK1

    def __init__(self, d, b, c):
        self.d = np.ascontiguousarray(d, dtype=np.float64)
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.c = float(c)
        assert self.d.shape == self.b.shape and self.d.ndim == 1

    def __call__(self, x):
        x = np.asarray(x, dtype=np.float64)
        return 0.5 * np.sum(self.d * x * x) + 0.5 * self.c * np.sum(x) ** 2 - np.sum(self.b * x)


class BFGSEngine(Engine):
    """symmetric=True: the rank-2 update restated so that H stays bitwise symmetric and only its
    upper 128 x 128 blocks are kept and streamed (NLSG_BFGS_SYMMETRIC, include/nlsg_c_api.h):
    56 % of the memory and traffic at dim = 1024; results agree with the literal update to rounding.
    reference_order=True: every sum in index order, as the reference's sequential loops take it
    (NLSG_BFGS_REFERENCE_ORDER): the reference's own runs bit for bit, default gradient included —
    with the default gradient also the faster kernels (a probe per lane); with a gradient functor
    1.5 x the tree kernels' time at dim = 1024.

    A CustomObjective with n_params > 0 (nlsg_bfgs_create_params): problem b minimises the objective
    under row b of set_params(rows) ([batch, n_params], read as p(k)); rows are replaced without
    recompiling. The search kernel runs four problems per workgroup, a wave each, so four rows share
    the workgroup's LDS: fits() says whether a shape has room.

    gradient: None — a CustomObjective's grad_body when it has one (nlsg_bfgs_create_gradient: the
    kernels evaluate that body, about one objective evaluation per gradient instead of 4 dim, and a
    gradient counts in gradient_evals_used only, as a Grad functor does in the reference), else the
    objective's own path; "finite_difference" forces the default gradient whatever the objective
    carries; "analytic" insists and raises ValueError when there is no gradient to evaluate.
    gradient_used says which ran: "analytic" or "finite_difference". In reference order a gradient of the
    terms form costs one index-order sum of the D terms (the body's `s`) beside the body, read or not.

    resident=True (NLSG_BFGS_RESIDENT, dim <= 64, not with symmetric): the whole loop of a solve in one
    kernel, a 64-lane workgroup per problem with its inverse Hessian in LDS; step(k) is one launch per 256
    turns instead of three or four per turn, and a problem neither waits for the batch's slowest line
    search nor keeps its wave once it has stopped. Every call returns what the lock-step engine returns,
    bit for bit, download_state() included; time_steps() is NlsgError code 2. fits_resident() says
    whether a shape is taken."""

    GRADIENTS = (None, "analytic", "finite_difference")
    _destroy, _set_params = "nlsg_bfgs_destroy", "nlsg_bfgs_set_params"

    @staticmethod
    def lds_bytes(dim, reference_order=False, n_params=0, resident=False):
        """LDS bytes of a search / init launch: the reference-order buffers of its four waves (none in
        tree order) and four rows of n_params objective parameters (host only). resident=True: the
        resident workgroup's block — H, its vectors, one wave's buffers — and ONE row; 0 where the library
        or the shape has no resident mode."""
        flags = _capi.BFGS_REFERENCE_ORDER if reference_order else 0
        # (not _with_params_lds: that answers 0 where the row's size is 0, n_params past the range; this
        # one keeps `need` there, and the lock-step launch takes four rows)
        if resident:
            need = int(require("nlsg_bfgs_lds_bytes")(dim, flags | _capi.BFGS_RESIDENT))
            if need == 0:
                return 0
            return need + (int(require("nlsg_custom_params_lds_bytes")(n_params)) if n_params else 0)
        need = int(require("nlsg_bfgs_lds_bytes")(dim, flags))
        return need + (4 * int(require("nlsg_custom_params_lds_bytes")(n_params)) if n_params else 0)

    @staticmethod
    def has_resident():
        """whether the loaded library has the resident mode (one older than the flag answers 0 to it)"""
        try:
            return int(require("nlsg_bfgs_lds_bytes")(2, _capi.BFGS_RESIDENT)) != 0
        except NlsgError:
            return False

    @staticmethod
    def fits_resident(dim, symmetric=False, n_params=0):
        """whether an engine with resident=True takes the shape: 1 <= dim <= 64, the literal update,
        0 <= n_params <= 4096 (either summation order: the workgroup's block stays below 75 KiB)"""
        if symmetric or not (1 <= dim <= 64 and 0 <= n_params <= _capi.CUSTOM_MAX_PARAMS):
            return False
        if not BFGSEngine.has_resident():
            return False
        need = BFGSEngine.lds_bytes(dim, True, n_params, resident=True)
        return 0 < need <= LDS_BUDGET

    @staticmethod
    def fits(dim, reference_order=False, n_params=0):
        """whether nlsg_bfgs_create_params takes the shape: 1 <= dim <= 1024, 0 <= n_params <= 4096
        and lds_bytes within the workgroup's 160 KiB"""
        if not (1 <= dim <= 1024 and 0 <= n_params <= _capi.CUSTOM_MAX_PARAMS):
            return False
        return BFGSEngine.lds_bytes(dim, reference_order, n_params) <= LDS_BUDGET

    def __init__(self, objective, batch, *, dim=None, max_iter=100, grad_eps=5e-3, alpha=1.0,
                 device=0, stream=None, symmetric=False, reference_order=False, gradient=None,
                 resident=False):
        if gradient not in self.GRADIENTS:
            raise ValueError(f"gradient must be one of {self.GRADIENTS}, not {gradient!r}")
        custom = isinstance(objective, CustomObjective)
        has_analytic = bool(objective.grad_body) if custom else not isinstance(objective, str)
        if gradient == "analytic" and not has_analytic:
            raise ValueError("gradient='analytic' needs an objective that carries its gradient: a "
                             "CustomObjective with grad_body=, or QuadDiagRank1")
        if gradient == "finite_difference" and not custom and not isinstance(objective, str):
            raise ValueError("QuadDiagRank1 is minimised with its analytic gradient only")
        self.gradient_used = "analytic" if has_analytic and gradient != "finite_difference" else "finite_difference"
        cfg = self._header(BFGSConfig, device, stream)
        cfg.flags = (_capi.BFGS_SYMMETRIC if symmetric else 0) | \
            (_capi.BFGS_REFERENCE_ORDER if reference_order else 0) | \
            (_capi.BFGS_RESIDENT if resident else 0)
        self.symmetric = bool(symmetric)
        self.resident = bool(resident)
        cfg.batch = batch
        cfg.max_iter, cfg.grad_eps, cfg.alpha = max_iter, grad_eps, alpha
        self.n_params = objective.n_params if custom else 0
        if custom:  # user objective + its gradient body or the finite-difference gradient
            if dim is None:
                raise TypeError("a custom objective needs dim=")
            cfg.objective, cfg.dim, cfg.quad_c = _capi.OBJ_CUSTOM, dim, 0.0
            if self.gradient_used == "analytic":  # (with or without parameters)
                create = self._creator(require("nlsg_bfgs_create_gradient"))
                grad = [_capi.BFGSGradientC(C.sizeof(_capi.BFGSGradientC), 0, objective.grad_body.encode())]
            else:
                create, grad = self._creator(lib().nlsg_bfgs_create_custom, "nlsg_bfgs_create_params"), []
            self._create_custom(create, cfg, objective, *grad)
        elif isinstance(objective, str):  # built-in objective + finite-difference gradient
            if dim is None:
                raise TypeError("a built-in objective needs dim=")
            cfg.objective, cfg.dim, cfg.quad_c = _capi.OBJECTIVES[objective], dim, 0.0
            self._create(lib().nlsg_bfgs_create, cfg, None, None)
        else:
            cfg.objective = objective.nlsg_objective
            cfg.dim, cfg.quad_c = objective.d.size, objective.c
            self._create(lib().nlsg_bfgs_create, cfg, pd_of(objective.d), pd_of(objective.b))

    def _x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.cfg.batch, self.cfg.dim)
        return x

    def init(self, x0):
        check(lib().nlsg_bfgs_init(self._h, pd_of(self._x(x0))))

    def step(self, iters=1):
        check(lib().nlsg_bfgs_step(self._h, iters))

    def unfinished(self):
        c = C.c_uint64()
        check(lib().nlsg_bfgs_unfinished(self._h, C.byref(c)))
        return c.value

    def identity_count(self):
        """Unfinished problems whose inverse Hessian is the identity right now (start / reset guard):
        the H passes skip their reads for those."""
        c = C.c_uint64()
        check(lib().nlsg_bfgs_identity_count(self._h, C.byref(c)))
        return c.value

    def download(self):
        B, n = self.cfg.batch, self.cfg.dim
        x = np.empty((B, n))
        st = (Status * B)()
        check(lib().nlsg_bfgs_download(self._h, pd_of(x), st))
        return x, list(st)

    def download_state(self, hessian=True):
        B, n = self.cfg.batch, self.cfg.dim
        g = np.empty((B, n))
        H = np.empty((B, n, n)) if hessian else None
        check(lib().nlsg_bfgs_download_state(self._h, pd_of(g), pd_of(H)))
        return g, H

    def minimize(self, x, params=None):
        """params: set_params(params) first."""
        self._apply_params(params)
        x = self._x(x)
        st = (Status * self.cfg.batch)()
        check(lib().nlsg_bfgs_minimize(self._h, pd_of(x), st))
        return x, list(st)

    def hessian_bytes_per_iteration(self):
        """Algorithmic HBM bytes of the H passes per iteration and problem: read H (t = H y), read
        and write H (update + next direction) — the whole matrix, or its upper 128 x 128 blocks."""
        n = self.cfg.dim
        if not self.symmetric:
            return 3 * n * n * 8
        nb = (n + 127) // 128
        return 3 * (nb * (nb + 1) // 2) * 128 * 128 * 8

    def time_steps(self, iters):
        total, hess = C.c_float(), C.c_float()
        check(lib().nlsg_bfgs_time_steps(self._h, iters, C.byref(total), C.byref(hess)))
        return total.value, hess.value


class BFGS:
    """Drop-in for nlsolver::BFGS on a device objective; x may be (n,) or (batch, n).
    reference_order=None (as include/nlsolver_mi/nlsolver.h's device::summation() default): reference
    order wherever the reference's arithmetic exists on the device — the quadratic, the default
    gradient on Rosenbrock / Sphere / Styblinski-Tang or a custom objective given by its terms; literal
    update — i.e. the reference's runs bit for bit. With the default gradient those are also the
    faster kernels; the quadratic pays 1.18 x on large batches. True / False force it.

    params: the run-time parameters of a CustomObjective with n_params > 0: one row (n_params,) shown
    to every start, or (batch, n_params) with a 2-D x, a row per start.

    A CustomObjective that carries grad_body is minimised with that gradient (BFGSEngine gradient=None);
    gradient_used says which path the last minimize() took. g stays None: the gradient of a device
    objective is part of the objective.

    driver="resident": the solve runs in the resident kernel (BFGSEngine resident=True) whenever
    BFGSEngine.fits_resident holds — dim <= 64, not symmetric, a library that has the mode — and through
    the lock-step engine otherwise: the same x and status bit for bit either way. `driver_used` says
    which engine the last minimize() ran on. Default "turns": the lock-step engine."""

    def __init__(self, f, g=None, max_iter=100, grad_eps=5e-3, alpha=1.0, *, device=0,
                 symmetric=False, reference_order=None, params=None, driver="turns"):
        check_driver(driver)
        self.driver, self.driver_used = driver, None
        self.n_params, self.params = pair_params(f, params)
        if g is not None:
            raise TypeError("device objectives carry their analytic gradient or use the default "
                            "finite-difference one; pass g=None")
        self.f = f
        self.gradient_used = "analytic" if getattr(f, "grad_body", None) or isinstance(f, QuadDiagRank1) \
            else "finite_difference"
        self.args = dict(max_iter=max_iter, grad_eps=grad_eps, alpha=alpha, device=device,
                         symmetric=symmetric, reference_order=reference_order)

    def minimize(self, x):
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim not in (1, 2):
            raise TypeError("x must be a float64 numpy array of shape (n,) or (batch, n); "
                            "it is updated in place")
        xb = x.reshape(1, -1) if x.ndim == 1 else x
        extra = dict(dim=xb.shape[1]) if isinstance(self.f, (str, CustomObjective)) else {}
        args = dict(self.args)
        if args["reference_order"] is None:
            fd = (isinstance(self.f, str) and self.f in ("rosenbrock", "sphere", "styblinski_tang")) or \
                (isinstance(self.f, CustomObjective) and self.f.chain != 2)  # (terms: index order is the body's own loop)
            quad = isinstance(self.f, QuadDiagRank1)
            args["reference_order"] = (fd or quad) and not args["symmetric"]
        rows = _rows_for_batch(self.params, xb.shape[0])
        resident = self.driver == "resident" and \
            BFGSEngine.fits_resident(xb.shape[1], bool(args["symmetric"]), self.n_params)
        if resident:
            args["resident"] = True
        self.driver_used = "resident" if resident else "turns"
        with BFGSEngine(self.f, xb.shape[0], **extra, **args) as eng:
            self.gradient_used = eng.gradient_used
            out, st = eng.minimize(xb, params=rows)
        xb[...] = out
        return st[0] if x.ndim == 1 else st

    def maximize(self, x):  # nlsolver.h:3199 static_assert(minimize, ...)
        raise NotImplementedError("BFGS currently only supports minimization (nlsolver.h:3199)")
