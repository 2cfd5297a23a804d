"""Host-side mirror of the reference's LevenbergMarquardt class, batched, for NLLS models
whose Gauss-Newton functors live on the device, and for built-in objectives minimised through the
reference's default functors (finite-difference gradient and Hessian, nlsolver.h:3494-3511).

Reference interface (nlsolver.h:3428-3463):
    LevenbergMarquardt<Callable, scalar_t, Grad, Hess>(f, lambda = 10, upward_mult = 10,
        downward_mult = 10, max_iter = 100, f_delta = 1e-12, g, h).minimize(x)
Here `f` is a TanhRegression model, a LinkRegression (the same model with another link function,
given as source text) or a CurveModel (any residual r(theta; t_i, y_i), given with its Jacobian row as
source text) (f = sum r^2, Grad = 2 J^T r, Hess = 2 J^T J evaluated by the
kernels); minimize() takes one start (n,) or a batch (batch, n) — BASELINE config 4.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import LMConfig, NlsgError, Status, check, lib, require  # noqa: F401
from ._engine import (LDS_BUDGET, CustomObjective, Engine, _rows_for_batch, check_driver, pair_params, pd_of,
                      rtc_library_path, timed_ms)


class TanhRegression:
    """r_i(theta) = y_i - tanh(sum_j A_ij theta_j); A: (batch, m, n), y: (batch, m)."""
    nlsg_nlls_objective = _capi.OBJ_TANH_REGRESSION

    def __init__(self, A, y):
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.A.ndim == 2:
            self.A, self.y = self.A[None], self.y[None]
        assert self.A.ndim == 3 and self.y.shape == self.A.shape[:2]

    def __call__(self, theta, problem=0):
        r = self.y[problem] - np.tanh(self.A[problem] @ np.asarray(theta, dtype=np.float64))
        return float(r @ r)


class LinkRegression:
    """r_i(theta) = y_i - phi(sum_j A_ij theta_j); A: (batch, m, n), y: (batch, m) as TanhRegression.

    value: the body of `double value(double z)` — phi(z); slope: the body of
    `double slope(double z, double v)` — phi'(z) with v = value(z) at hand. Both are HIP source compiled
    when an engine is made, and may call the library's deterministic device math (det_exp, det_log,
    det_tanh, ...). The engine runs the Gauss-Newton kernels of TanhRegression (J^T J on the matrix
    cores, Cholesky or QR step) instantiated on this link.

    host: an optional numpy callable phi(z) for __call__ (f at a point, on the CPU); the device never
    uses it."""
    nlsg_nlls_objective = _capi.OBJ_LINK_REGRESSION

    def __init__(self, A, y, value, slope, host=None):
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.A.ndim == 2:
            self.A, self.y = self.A[None], self.y[None]
        if self.A.ndim != 3 or self.y.shape != self.A.shape[:2]:
            raise ValueError(f"A must be (batch, m, n) or (m, n) and y its (batch, m) or (m,): got "
                             f"{self.A.shape} and {self.y.shape}")
        if not isinstance(value, str) or not isinstance(slope, str) or not value.strip() or not slope.strip():
            raise TypeError("value and slope are the source text of the link's two function bodies")
        self.value_body, self.slope_body, self.host = value, slope, host

    def __call__(self, theta, problem=0):
        if self.host is None:
            raise TypeError("this LinkRegression has no host= link: its phi exists as device source only")
        r = self.y[problem] - self.host(self.A[problem] @ np.asarray(theta, dtype=np.float64))
        return float(r @ r)

    @classmethod
    def tanh(cls, A, y):
        """TanhRegression through the link mechanism: the same bits"""
        return cls(A, y, "return det_tanh(z);", "return 1 - v * v;", host=np.tanh)

    @classmethod
    def logistic(cls, A, y):
        return cls(A, y, "return 1.0 / (1.0 + det_exp(-z));", "return v * (1.0 - v);",
                   host=lambda z: 1.0 / (1.0 + np.exp(-z)))

    @classmethod
    def exp(cls, A, y):
        return cls(A, y, "return det_exp(z);", "return v;", host=np.exp)

    @classmethod
    def identity(cls, A, y):
        """plain linear least squares, r = y - A theta"""
        return cls(A, y, "return z;", "return 1.0;", host=lambda z: z)


class CurveModel:
    """r_i(theta) = residual(theta; t_i, y_i): a model nonlinear in several parameters, fitted to each of
    `batch` series with their own (t_i, y_i). t: (batch, m, K) — K numbers per observation, 1 <= K <= 16 —
    or (batch, m) for K = 1, or one problem without the batch axis; y: (batch, m) or (m,); n parameters,
    1 <= n <= 64.

    body: HIP source compiled when an engine is made, the residual and its Jacobian row in one. It sees
    th(j) (parameter j), t(k) (the observation's k-th datum; k a constant or an unrolled loop's counter),
    y (its target) and n, and writes r (the residual) and J(j) = dr/dtheta_j — six names taken inside
    it; it may call the library's deterministic device math (det_exp, det_log, det_tanh, ...). A J(j) it does not write is 0, a J(j) with j outside [0, n) is dropped, and
    rows past m contribute nothing whatever the body makes of zero data. Per-problem constants can ride
    in extra columns of t. The engine runs the Gauss-Newton functors of TanhRegression (f = sum r^2,
    2 J^T r, 2 J^T J on the matrix cores) with either step.

    host: an optional numpy callable (theta, t, y) -> r, with t (m, K) and y (m,), for __call__ (f at a
    point, on the CPU); the device never uses it."""
    nlsg_nlls_objective = _capi.OBJ_CURVE_MODEL

    def __init__(self, t, y, body, n, host=None):
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.y.ndim == 1 and self.t.ndim in (1, 2):  # one problem
            self.t, self.y = self.t[None], self.y[None]
        if self.t.ndim == 2:  # K = 1
            self.t = self.t[:, :, None]
        if self.t.ndim != 3 or self.y.ndim != 2 or self.y.shape != self.t.shape[:2] or 0 in self.t.shape:
            raise ValueError(f"t must be (batch, m, K), (batch, m), (m, K) or (m,) and y its (batch, m) or "
                             f"(m,): got {np.shape(t)} and {np.shape(y)}")
        if not 1 <= self.t.shape[2] <= 16:
            raise ValueError(f"a curve model takes 1 .. 16 data per observation: K = {self.t.shape[2]}")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n is the number of parameters, an integer >= 1: got {n!r}")
        if not isinstance(body, str) or not body.strip():
            raise TypeError("body is the source text of the residual and its Jacobian row")
        self.n, self.body, self.host = int(n), body, host

    def __call__(self, theta, problem=0):
        if self.host is None:
            raise TypeError("this CurveModel has no host= residual: its body exists as device source only")
        r = np.asarray(self.host(np.asarray(theta, dtype=np.float64), self.t[problem], self.y[problem]),
                       dtype=np.float64)
        return float(r @ r)

    @classmethod
    def exp_decay(cls, t, y):
        """theta0 exp(-theta1 t) + theta2"""
        body = ("const double e = det_exp(-th(1) * t(0));\n"
                "r = y - (th(0) * e + th(2));\n"
                "J(0) = -e;  J(1) = th(0) * t(0) * e;  J(2) = -1.0;")
        return cls(t, y, body, 3, host=lambda th, t, y: y - (th[0] * np.exp(-th[1] * t[:, 0]) + th[2]))

    @classmethod
    def gaussian_peak(cls, t, y):
        """theta = (amplitude, centre, width, offset): a exp(-(t - c)^2 / (2 w^2)) + d"""
        body = ("const double u = (t(0) - th(1)) / th(2);\n"
                "const double e = det_exp(-0.5 * (u * u));\n"
                "r = y - (th(0) * e + th(3));\n"
                "const double ae = th(0) * e;\n"
                "J(0) = -e;  J(1) = -(ae * u / th(2));  J(2) = -(ae * (u * u) / th(2));  J(3) = -1.0;")
        return cls(t, y, body, 4, host=lambda th, t, y: y - (
            th[0] * np.exp(-0.5 * ((t[:, 0] - th[1]) / th[2]) ** 2) + th[3]))

    @classmethod
    def logistic4(cls, t, y):
        """the four-parameter dose-response curve, theta = (a, b, c, d): d + (a - d) / (1 + (t / c)^b) for
        t > 0 — a the response at t -> 0, d at t -> inf, c the inflection point, b the slope there"""
        body = ("const double L = det_log(t(0)) - det_log(th(2));\n"
                "const double u = det_exp(th(1) * L);\n"
                "const double s = 1.0 / (1.0 + u);\n"
                "const double ad = th(0) - th(3);\n"
                "r = y - (th(3) + ad * s);\n"
                "const double w = ad * (s * s) * u;\n"
                "J(0) = -s;  J(1) = w * L;  J(2) = -(w * th(1) / th(2));  J(3) = -(1.0 - s);")
        return cls(t, y, body, 4, host=lambda th, t, y: y - (
            th[3] + (th[0] - th[3]) / (1.0 + (t[:, 0] / th[2]) ** th[1])))


def _cov_scale(scale):
    """"residual" / "absolute" or LM_COV_RESIDUAL / LM_COV_ABSOLUTE -> the constant (no library call)"""
    names = {"residual": _capi.LM_COV_RESIDUAL, "absolute": _capi.LM_COV_ABSOLUTE}
    if isinstance(scale, str) and scale in names:
        return names[scale]
    if not isinstance(scale, (bool, str)) and isinstance(scale, (int, np.integer)) and int(scale) in names.values():
        return int(scale)
    raise ValueError(f'scale is "residual" or "absolute" (LM_COV_RESIDUAL / LM_COV_ABSOLUTE): got {scale!r}')


class LMEngine(Engine):
    """model: a TanhRegression, a LinkRegression or a CurveModel, or the name / id of a built-in objective ("rosenbrock", "sphere",
    "styblinski_tang") or a CustomObjective, with batch= and n= (default functors: fin_diff +
    fin_diff_h).

    A CustomObjective with n_params > 0 (nlsg_lm_create_params): problem b minimises the objective under
    row b of set_params(rows) ([batch, n_params], read as p(k)) — one fit per series; rows are replaced
    without recompiling. The row lives in the workgroup's LDS: fits() says whether a shape has room.

    solver=LM_CHOLESKY | LM_RESIDENT (NLSG_LM_RESIDENT; Gauss-Newton models, n <= 64): the whole loop of a solve in
    one kernel, a 64-lane workgroup per problem, H, g and theta in LDS and the loop's scalars in registers,
    at most ceil((max_iter + 1) / LM_RESIDENT_CUT) launches — theta, every status field and lambda are the
    lock-step engine's bit for bit. set_solver(LM_CHOLESKY | LM_RESIDENT) switches an existing engine, the
    plain value back; `.driver` says which one runs ("turns" / "resident"). fits_resident() says whether a shape is taken."""
    _destroy, _set_params = "nlsg_lm_destroy", "nlsg_lm_set_params"

    @staticmethod
    def has_resident():
        """whether the loaded library has the resident mode (one older than the flag answers 0 to it)"""
        try:
            return int(require("nlsg_lm_lds_bytes")(2, _capi.LM_CHOLESKY | _capi.LM_RESIDENT)) != 0
        except NlsgError:
            return False

    @staticmethod
    def fits_resident(model_or_n, solver=_capi.LM_CHOLESKY):
        """whether an engine with solver | LM_RESIDENT takes the model: a TanhRegression, LinkRegression or
        CurveModel (or the parameter count of one) with 1 <= n <= 64, the Cholesky solver, and a library
        that has the mode. An objective by name or a CustomObjective (the finite-difference model) never."""
        if isinstance(model_or_n, (str, CustomObjective, bool)):
            return False
        if isinstance(model_or_n, (int, np.integer)):
            n = int(model_or_n)
        elif isinstance(model_or_n, CurveModel):
            n = model_or_n.n
        elif hasattr(model_or_n, "A"):
            n = model_or_n.A.shape[2]
        else:
            return False
        if solver != _capi.LM_CHOLESKY or not 1 <= n <= 64 or not LMEngine.has_resident():
            return False
        return int(require("nlsg_lm_lds_bytes")(n, _capi.LM_CHOLESKY | _capi.LM_RESIDENT)) != 0

    @staticmethod
    def lds_bytes(n, reference_order=False, n_params=0):
        """LDS bytes of the launch that evaluates an objective of n parameters, the row of n_params
        objective parameters included (host only; tree order past 64 parameters takes none of its own)"""
        solver = _capi.LM_CHOLESKY_REFERENCE_ORDER if reference_order else _capi.LM_CHOLESKY
        need = int(require("nlsg_lm_lds_bytes")(n, solver))
        # (not _with_params_lds: need == 0 is a valid answer here, and the row is added to it)
        return need + (int(require("nlsg_custom_params_lds_bytes")(n_params)) if n_params else 0)

    @staticmethod
    def fits(n, reference_order=False, n_params=0):
        """whether nlsg_lm_create_params takes the shape: 1 <= n <= 1024, 0 <= n_params <= 4096 and
        lds_bytes within the workgroup's 160 KiB"""
        if not (1 <= n <= 1024 and 0 <= n_params <= _capi.CUSTOM_MAX_PARAMS):
            return False
        return LMEngine.lds_bytes(n, reference_order, n_params) <= LDS_BUDGET

    def __init__(self, model, *, lam=10.0, up=10.0, down=10.0, max_iter=100, f_delta=1e-12,
                 solver=_capi.LM_CHOLESKY, device=0, stream=None, batch=None, n=None):
        custom = model if isinstance(model, CustomObjective) else None
        fd = custom is not None or isinstance(model, (str, int))
        if fd:
            if batch is None or n is None:
                raise TypeError("an objective needs batch= and n=")
            B, m = batch, 0
            objective = self._objective_id(model)[0]
        elif isinstance(model, CurveModel):
            (B, m), n = model.y.shape, model.n
            objective = model.nlsg_nlls_objective
        else:
            B, m, n = model.A.shape
            objective = model.nlsg_nlls_objective
        cfg = self._header(LMConfig, device, stream)
        cfg.objective, cfg.solver = objective, solver
        cfg.batch, cfg.m, cfg.n = B, m, n
        cfg.lambda_, cfg.up, cfg.down, cfg.max_iter, cfg.f_delta = lam, up, down, max_iter, f_delta
        self.n_params = custom.n_params if custom else 0
        if custom:
            self._create_custom(self._creator(lib().nlsg_lm_create_custom, "nlsg_lm_create_params"), cfg, custom)
        elif isinstance(model, LinkRegression):
            self._create_custom(require("nlsg_lm_create_link"), cfg,
                                _capi.LMLinkC(model.value_body.encode(), model.slope_body.encode()))
        elif isinstance(model, CurveModel):
            create, set_data = require("nlsg_lm_create_curve"), require("nlsg_lm_set_curve_data")
            self._create_custom(create, cfg, _capi.LMCurveC(model.body.encode(), model.t.shape[2]))
            check(set_data(self._h, pd_of(model.t), pd_of(model.y)))
        elif self.driver == "resident":  # a TanhRegression's resident kernel is compiled at run time
            check(lib().nlsg_rtc_load(rtc_library_path().encode()))
            self._create(lib().nlsg_lm_create, cfg)
        else:
            self._create(lib().nlsg_lm_create, cfg)
        if not fd and not isinstance(model, CurveModel):
            check(lib().nlsg_lm_set_data(self._h, pd_of(model.A), pd_of(model.y)))

    @property
    def driver(self):
        """"resident" or "turns": which driver runs the next solve (the flag in cfg.solver)"""
        flagged = self.cfg.solver >= _capi.LM_RESIDENT and self.cfg.solver & _capi.LM_RESIDENT
        return "resident" if flagged else "turns"

    def set_solver(self, solver):
        """LM_CHOLESKY / LM_QR for the next solves, LM_CHOLESKY | LM_RESIDENT for the resident driver (the
        plain value switches back); the model data stays on the device."""
        flagged = solver >= _capi.LM_RESIDENT
        if flagged:  # (the resident kernel of a TanhRegression engine is compiled here)
            check(lib().nlsg_rtc_load(rtc_library_path().encode()))
        check(lib().nlsg_lm_set_solver(self._h, solver))
        self.cfg.solver = solver

    def minimize(self, theta, params=None):
        """params: set_params(params) first."""
        self._apply_params(params)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        assert theta.shape == (self.cfg.batch, self.cfg.n)
        st = (Status * self.cfg.batch)()
        lam = np.empty(self.cfg.batch)
        check(lib().nlsg_lm_minimize(self._h, pd_of(theta), st, pd_of(lam)))
        return theta, list(st), lam

    def covariance(self, theta, scale="residual"):
        """Parameter covariance of every problem's fit at theta (batch, n), usually minimize()'s result:
        cov = c (J^T J)^-1 with c = s2 = f / (m - n) (scale="residual", scipy's curve_fit default) or
        c = 1 (scale="absolute": the residuals are already divided by their sigma). Returns
        (cov (batch, n, n), s2 (batch,), ok (batch,) bool); where J^T J has a Cholesky pivot <= 0 — or,
        in residual mode, f is not finite — ok is False and the problem's cov is all NaN.
        Near-singularity is not diagnosed. Gauss-Newton models with n <= 64 only."""
        scale = _cov_scale(scale)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        B, n = self.cfg.batch, self.cfg.n
        if theta.shape != (B, n):
            raise ValueError(f"theta must be (batch, n) = ({B}, {n}): got {theta.shape}")
        fn = require("nlsg_lm_covariance")
        cov, s2, ok = np.empty((B, n, n)), np.empty(B), np.empty(B, dtype=np.int32)
        check(fn(self._h, pd_of(theta), scale, pd_of(cov), pd_of(s2),
                 ok.ctypes.data_as(C.POINTER(C.c_int32))))
        return cov, s2, ok.astype(bool)

    def stderr(self, theta, scale="residual"):
        """Standard errors (batch, n): the square roots of covariance()'s diagonal, NaN rows where not ok"""
        cov, _, _ = self.covariance(theta, scale)
        return np.sqrt(np.diagonal(cov, axis1=1, axis2=2))

    def time_solve(self, theta0, repeats=1, params=None):
        self._apply_params(params)
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
        return timed_ms(lib().nlsg_lm_time_solve, self._h, pd_of(theta0), repeats)

    def time_eval_kernel(self, theta0, repeats=1):
        """Total ms of `repeats` launches of the evaluation kernel (f, g, H at theta0)."""
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
        return timed_ms(lib().nlsg_lm_time_eval_kernel, self._h, pd_of(theta0), repeats)

    def time_qr_kernel(self, theta0, repeats=1):
        """Total ms of `repeats` launches of the QR step kernel (after one evaluation at theta0)."""
        theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
        return timed_ms(lib().nlsg_lm_time_qr_kernel, self._h, pd_of(theta0), repeats)


class LevenbergMarquardt:
    """Drop-in for nlsolver::LevenbergMarquardt on a device NLLS model or a built-in objective
    (by name); x: (n,) or (batch, n). solver=None (as include/nlsolver_mi/nlsolver.h's
    device::summation() default): the default-functor model on Rosenbrock / Sphere / Styblinski-Tang solves
    in reference order (LM_CHOLESKY_REFERENCE_ORDER: the reference's run bit for bit, and — a probe
    per lane — the faster evaluation); everything else with LM_CHOLESKY.

    params: the run-time parameters of a CustomObjective with n_params > 0: one row (n_params,) shown
    to every start, or (batch, n_params) with a 2-D x, a row per start.

    with_driver("resident") (or .driver = "resident"): the solve runs in the resident kernel (LMEngine with
    solver | LM_RESIDENT) whenever LMEngine.fits_resident holds — a Gauss-Newton model, n <= 64, the Cholesky solver, a library that has the
    mode — and through the lock-step engine otherwise: the same x and status bit for bit either way.
    `driver_used` says which one the last minimize() ran."""

    def __init__(self, f, lam=10.0, upward_mult=10.0, downward_mult=10.0, max_iter=100,
                 f_delta=1e-12, g=None, h=None, *, solver=None, device=0, params=None):
        self.n_params, self.params = pair_params(f, params)
        if g is not None or h is not None:
            raise TypeError("device models carry their functors (Gauss-Newton for NLLS models, "
                            "the reference's finite-difference defaults for objectives)")
        self.f = f
        self.args = dict(lam=lam, up=upward_mult, down=downward_mult, max_iter=max_iter,
                         f_delta=f_delta, solver=solver, device=device)

    driver_used = None  # "turns" / "resident": what the last minimize() ran
    _driver = "turns"

    @property
    def driver(self):
        """"turns" (default) or "resident"; anything else is a ValueError"""
        return self._driver

    @driver.setter
    def driver(self, driver):
        check_driver(driver)
        self._driver = driver

    def with_driver(self, driver):
        """sets .driver and returns the solver: LevenbergMarquardt(model).with_driver("resident").minimize(x)"""
        self.driver = driver
        return self

    def _engine(self, x):
        """x as (batch, n), the engine minimize() runs it on, and the parameter rows of that batch"""
        if not isinstance(x, np.ndarray) or x.dtype != np.float64 or x.ndim not in (1, 2):
            raise TypeError("x must be a float64 numpy array of shape (n,) or (batch, n)")
        xb = x.reshape(1, -1) if x.ndim == 1 else x
        has_data = hasattr(self.f, "A") or isinstance(self.f, CurveModel)
        shape = {} if has_data else dict(batch=xb.shape[0], n=xb.shape[1])
        args = dict(self.args)
        if args["solver"] is None:
            ref = (isinstance(self.f, str) and self.f in ("rosenbrock", "sphere", "styblinski_tang")) or \
                (isinstance(self.f, CustomObjective) and self.f.chain != 2)  # (given by its terms)
            args["solver"] = _capi.LM_CHOLESKY_REFERENCE_ORDER if ref else _capi.LM_CHOLESKY
        rows = _rows_for_batch(self.params, xb.shape[0])
        # (the resident kernels are compiled at run time: a process that cannot load hiprtc stays with the turns,
        # which need it for a TanhRegression not at all)
        resident = self.driver == "resident" and LMEngine.fits_resident(self.f, args["solver"]) and \
            lib().nlsg_rtc_load(rtc_library_path().encode()) == 0
        if resident:
            args["solver"] |= _capi.LM_RESIDENT
        self._resident = resident
        return xb, LMEngine(self.f, **args, **shape), rows

    def minimize(self, x):
        xb, engine, rows = self._engine(x)
        self.driver_used = "resident" if self._resident else "turns"
        with engine as eng:
            out, st, lam = eng.minimize(xb, params=rows)
        xb[...] = out
        self.lambdas = lam  # the reference keeps lambda as a member across calls (:3436)
        return st[0] if x.ndim == 1 else st

    def covariance(self, x, scale="residual"):
        """LMEngine.covariance at x, (n,) or (batch, n) as in minimize (usually the x it left): the
        covariance (n, n) or (batch, n, n). A problem whose J^T J does not factor is all NaN."""
        scale = _cov_scale(scale)
        xb, engine, _ = self._engine(x)
        with engine as eng:
            cov, _, _ = eng.covariance(xb, scale)
        return cov[0] if x.ndim == 1 else cov

    def stderr(self, x, scale="residual"):
        """the square roots of covariance()'s diagonal: (n,) or (batch, n)"""
        cov = self.covariance(x, scale)
        return np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1))

    def maximize(self, x):  # nlsolver.h:3468 static_assert(minimize, ...)
        raise NotImplementedError("LevenbergMarquardt currently only supports minimization")
