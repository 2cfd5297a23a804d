"""The state-order errors of the C-ABI that need a live engine: what every entry point answers when it
is called before the call it depends on, or on an engine of the wrong kind. One create per engine at the
smallest shapes of tests/_engine_lifecycle.py, the wrong-order calls, destroy; codes and texts are
literals copied from the source as it stood before the engine files shared their front doors, never
formatted by code shared with the library. The calls rejected before any device is touched are
tests/test_engine_doors_cpu.py's."""
import ctypes as C

import numpy as np
import pytest

from nlsolver_amd import _capi as A
from tests import _engine_lifecycle as L

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 6


@pytest.fixture(scope="module")
def lib():
    lib = A.lib()
    yield lib
    lib.nlsg_release_cached()


class Bufs:
    """valid arguments for any entry point at batch 2, dim 2, pop <= 8, m 3"""

    def __init__(self):
        self.x = np.full(64, 0.5)
        self.y = np.full(64, 0.25)
        self.u = np.arange(1, 65, dtype=np.uint64)
        self.status = (A.Status * 8)()
        self.ms = C.c_float()
        self.ms2 = C.c_float()
        self.ok = (C.c_int32 * 8)()

    @property
    def d(self):
        return self.x.ctypes.data_as(A.pd)

    @property
    def d2(self):
        return self.y.ctypes.data_as(A.pd)

    @property
    def q(self):
        return self.u.ctypes.data_as(A.pu)

    @property
    def dev(self):  # stands for a device pointer in a call that is rejected before it is used
        return self.x.ctypes.data


def expect(lib, rc, code, text):
    assert (int(rc), L.last_error(lib)) == (code, text)


def engine(lib, symbol, cfg, *extras):
    rc, h = L._call_create(lib, symbol, cfg, list(extras))
    assert rc == 0 and h.value, (symbol, rc, L.last_error(lib))
    return h


def params_obj():
    return L._obj(L.WITH_P, 1)


def test_de_before_init(lib):
    b, text = Bufs(), "nlsg_de_init has not been called"
    h = engine(lib, "nlsg_de_create", L.de_cfg())
    try:
        expect(lib, lib.nlsg_de_step(h, 1), STATE, text)
        expect(lib, lib.nlsg_de_status(h, b.status), STATE, text)
        expect(lib, lib.nlsg_de_best(h, b.d, b.d2, b.q), STATE, text)
        expect(lib, lib.nlsg_de_download(h, b.d, b.d2, b.q), STATE, text)
        expect(lib, lib.nlsg_de_upload(h, b.d, b.d2), STATE, text)
        expect(lib, lib.nlsg_de_bound_counts(h, b.q), STATE, text)
        expect(lib, lib.nlsg_de_screen_counts(h, b.q), STATE, text)
        expect(lib, lib.nlsg_de_time_generation_kernel(h, 1, C.byref(b.ms)), STATE, text)
        expect(lib, lib.nlsg_de_time_turns(h, 1, C.byref(b.ms)), STATE, text)
        expect(lib, lib.nlsg_de_turn_begin(h, b.dev), STATE, text)
        expect(lib, lib.nlsg_de_turn_end(h, b.dev, 1), STATE, text)
        expect(lib, lib.nlsg_de_turn_finalize(h, b.dev, 1), STATE, text)
        expect(lib, lib.nlsg_de_turn_generation(h), STATE, text)
        expect(lib, lib.nlsg_de_step_sharded(h, 1), STATE, text)
    finally:
        assert lib.nlsg_de_destroy(h) == 0


def test_pso_before_init(lib):
    b, text = Bufs(), "nlsg_pso_init has not been called"
    h = engine(lib, "nlsg_pso_create", L.pso_cfg())
    try:
        expect(lib, lib.nlsg_pso_step(h, 1), STATE, text)
        expect(lib, lib.nlsg_pso_status(h, b.status), STATE, text)
        expect(lib, lib.nlsg_pso_best(h, b.d, b.d2, b.q), STATE, text)
        expect(lib, lib.nlsg_pso_download(h, b.d, b.d, b.d2, b.d2), STATE, text)
        expect(lib, lib.nlsg_pso_time_move_kernel(h, 1, C.byref(b.ms)), STATE, text)
        expect(lib, lib.nlsg_pso_turn_begin(h, b.dev), STATE, text)
        expect(lib, lib.nlsg_pso_turn_end(h, b.dev, 1), STATE, text)
        expect(lib, lib.nlsg_pso_step_sharded(h, 1), STATE, text)
    finally:
        assert lib.nlsg_pso_destroy(h) == 0


def test_bfgs_before_init(lib):
    b, text = Bufs(), "nlsg_bfgs_init has not been called"
    h = engine(lib, "nlsg_bfgs_create", L.bfgs_cfg(), None, None)
    try:
        expect(lib, lib.nlsg_bfgs_step(h, 1), STATE, text)
        expect(lib, lib.nlsg_bfgs_unfinished(h, b.q), STATE, text)
        expect(lib, lib.nlsg_bfgs_identity_count(h, b.q), STATE, text)
        expect(lib, lib.nlsg_bfgs_download(h, b.d, b.status), STATE, text)
        expect(lib, lib.nlsg_bfgs_download_state(h, b.d, b.d2), STATE, text)
        expect(lib, lib.nlsg_bfgs_time_steps(h, 1, C.byref(b.ms), C.byref(b.ms2)), STATE, text)
    finally:
        assert lib.nlsg_bfgs_destroy(h) == 0


def test_bfgs_time_steps_on_a_resident_engine(lib):
    b = Bufs()
    h = engine(lib, "nlsg_bfgs_create", L.bfgs_cfg(flags=A.BFGS_RESIDENT), None, None)
    try:
        assert lib.nlsg_bfgs_init(h, b.d) == 0, L.last_error(lib)
        expect(lib, lib.nlsg_bfgs_time_steps(h, 1, C.byref(b.ms), C.byref(b.ms2)), UNSUPPORTED,
               "a resident engine has no separate H kernels to bracket: time nlsg_bfgs_step")
    finally:
        assert lib.nlsg_bfgs_destroy(h) == 0


def test_de_batch_before_init(lib):
    b, text = Bufs(), "nlsg_de_batch_init has not been called"
    h = engine(lib, "nlsg_de_batch_create", L.de_batch_cfg())
    try:
        expect(lib, lib.nlsg_de_batch_step(h, 1), STATE, text)
        expect(lib, lib.nlsg_de_batch_status(h, b.status), STATE, text)
        expect(lib, lib.nlsg_de_batch_best(h, b.d, b.d2, b.q), STATE, text)
        expect(lib, lib.nlsg_de_batch_download(h, 0, b.d, b.d2), STATE, text)
        expect(lib, lib.nlsg_de_batch_upload(h, b.d, b.d2), STATE, text)
    finally:
        assert lib.nlsg_de_batch_destroy(h) == 0


def test_pso_batch_before_init(lib):
    b, text = Bufs(), "nlsg_pso_batch_init has not been called"
    h = engine(lib, "nlsg_pso_batch_create", L.pso_batch_cfg())
    try:
        expect(lib, lib.nlsg_pso_batch_step(h, 1), STATE, text)
        expect(lib, lib.nlsg_pso_batch_status(h, b.status), STATE, text)
        expect(lib, lib.nlsg_pso_batch_best(h, b.d, b.d2, b.q), STATE, text)
        expect(lib, lib.nlsg_pso_batch_download(h, 0, b.d, b.d, b.d2, b.d2), STATE, text)
    finally:
        assert lib.nlsg_pso_batch_destroy(h) == 0


def _lm_before_data(lib, h, text):
    b = Bufs()
    expect(lib, lib.nlsg_lm_minimize(h, b.d, b.status, b.d2), STATE, text)
    expect(lib, lib.nlsg_lm_time_solve(h, b.d, 1, C.byref(b.ms)), STATE, text)
    expect(lib, lib.nlsg_lm_covariance(h, b.d, A.LM_COV_RESIDUAL, b.d2, None, b.ok), STATE, text)
    expect(lib, lib.nlsg_lm_time_eval_kernel(h, b.d, 1, C.byref(b.ms)), STATE, text)
    expect(lib, lib.nlsg_lm_time_qr_kernel(h, b.d, 1, C.byref(b.ms)), STATE, text)


def test_lm_before_set_data(lib):
    b = Bufs()
    h = engine(lib, "nlsg_lm_create", L.lm_cfg())
    try:
        _lm_before_data(lib, h, "nlsg_lm_set_data has not been called")
        expect(lib, lib.nlsg_lm_set_curve_data(h, b.d, b.d2), INVALID_ARG,
               "not a curve engine (nlsg_lm_create_curve): its data go by nlsg_lm_set_data")
        expect(lib, lib.nlsg_lm_set_params(h, b.d), INVALID_ARG,
               "the engine's objective declares no parameters (nlsg_lm_create_params)")
    finally:
        assert lib.nlsg_lm_destroy(h) == 0


def test_lm_curve_before_set_curve_data(lib):
    b = Bufs()
    symbol, _, cfg, extras = L.ENGINES["lm_curve"]
    h = engine(lib, symbol, cfg, *extras)
    try:
        _lm_before_data(lib, h, "nlsg_lm_set_curve_data has not been called")
        expect(lib, lib.nlsg_lm_set_data(h, b.d, b.d2), INVALID_ARG,
               "a curve model's data are t and y: nlsg_lm_set_curve_data")
        expect(lib, lib.nlsg_lm_set_params(h, b.d), INVALID_ARG,
               "a curve model has no p(k): per-problem constants ride in columns of t (nlsg_lm_set_curve_data)")
    finally:
        assert lib.nlsg_lm_destroy(h) == 0


def test_lm_objective_engine_takes_no_data(lib):
    b = Bufs()
    h = engine(lib, "nlsg_lm_create", L.lm_cfg(objective=0, m=0))
    try:
        expect(lib, lib.nlsg_lm_set_data(h, b.d, b.d2), STATE, "this engine minimises a built-in objective: no data")
    finally:
        assert lib.nlsg_lm_destroy(h) == 0


# kind -> (create_params symbol, config, destroy symbol, the text before set_params,
#          [(entry point that launches, its arguments behind the handle)])
FIRST = "the objective has 1 parameters: call %s first"
NOT_CALLED = "the objective has 1 parameters: %s has not been called"


def _launching(b):
    ms = C.byref(b.ms)
    return {
        "de_batch": ("nlsg_de_batch_create_custom", L.de_batch_cfg(A.OBJ_CUSTOM), "nlsg_de_batch_destroy",
                     NOT_CALLED % "nlsg_de_batch_set_params",
                     [("nlsg_de_batch_init", (b.d, b.q)), ("nlsg_de_batch_minimize", (b.d, b.q, b.status)),
                      ("nlsg_de_batch_time_solve", (b.d, b.q, 1, ms))]),
        "pso_batch": ("nlsg_pso_batch_create_custom", L.pso_batch_cfg(A.OBJ_CUSTOM), "nlsg_pso_batch_destroy",
                      NOT_CALLED % "nlsg_pso_batch_set_params",
                      [("nlsg_pso_batch_init", (b.d, b.d2, b.q)),
                       ("nlsg_pso_batch_minimize", (b.d, b.d, b.d2, b.q, b.status)),
                       ("nlsg_pso_batch_time_solve", (b.d, b.d2, b.q, 1, ms))]),
        "bfgs": ("nlsg_bfgs_create_params", L.bfgs_cfg(A.OBJ_CUSTOM), "nlsg_bfgs_destroy",
                 FIRST % "nlsg_bfgs_set_params",
                 [("nlsg_bfgs_init", (b.d,)), ("nlsg_bfgs_step", (1,)), ("nlsg_bfgs_minimize", (b.d, b.status)),
                  ("nlsg_bfgs_time_steps", (1, ms, C.byref(b.ms2)))]),
        "lm": ("nlsg_lm_create_params", L.lm_cfg(A.OBJ_CUSTOM, m=0), "nlsg_lm_destroy",
               FIRST % "nlsg_lm_set_params",
               [("nlsg_lm_minimize", (b.d, b.status, b.d2)), ("nlsg_lm_time_solve", (b.d, 1, ms)),
                ("nlsg_lm_time_eval_kernel", (b.d, 1, ms)), ("nlsg_lm_time_qr_kernel", (b.d, 1, ms))]),
        "nm": ("nlsg_nm_create_params", L.nm_cfg(A.OBJ_CUSTOM), "nlsg_nm_destroy", FIRST % "nlsg_nm_set_params",
               [("nlsg_nm_minimize", (b.d, None, None, b.status, b.d2)), ("nlsg_nm_phase_cycles", (b.d, b.q)),
                ("nlsg_nm_time_solve", (b.d, 1, ms))]),
        "nmpso": ("nlsg_nmpso_create_params", L.nmpso_cfg(A.OBJ_CUSTOM), "nlsg_nmpso_destroy",
                  FIRST % "nlsg_nmpso_set_params",
                  [("nlsg_nmpso_minimize", (b.d, None, None, b.status)), ("nlsg_nmpso_time_solve", (b.d, 1, ms))]),
        "sann": ("nlsg_sann_create_params", L.sann_cfg(A.OBJ_CUSTOM), "nlsg_sann_destroy",
                 FIRST % "nlsg_sann_set_params",
                 [("nlsg_sann_minimize", (b.d, b.status)), ("nlsg_sann_time_solve", (b.d, 1, ms))]),
    }


@pytest.mark.parametrize("kind", ["de_batch", "pso_batch", "bfgs", "lm", "nm", "nmpso", "sann"])
def test_nothing_launches_before_set_params(lib, kind):
    create, cfg, destroy, text, calls = _launching(Bufs())[kind]
    h = engine(lib, create, cfg, params_obj())
    try:
        for symbol, args in calls:
            rc = A.require(symbol)(h, *args)
            assert (symbol, int(rc), L.last_error(lib)) == (symbol, STATE, text)
    finally:
        assert A.require(destroy)(h) == 0


NO_PARAMETERS = {
    "de_batch": "the engine's objective declares no parameters (n_params == 0)",
    "pso_batch": "the engine's objective declares no parameters (n_params == 0)",
    "bfgs": "the engine's objective declares no parameters (nlsg_bfgs_create_params)",
    "lm": "the engine's objective declares no parameters (nlsg_lm_create_params)",
    "nm": "the engine's objective declares no parameters (nlsg_nm_create_params)",
    "nmpso": "the engine's objective declares no parameters (nlsg_nmpso_create_params)",
    "sann": "the engine's objective declares no parameters (nlsg_sann_create_params)",
}


@pytest.mark.parametrize("kind", sorted(NO_PARAMETERS))
def test_set_params_on_an_engine_without_parameters(lib, kind):
    _, without, set_params = L.PARAM_KINDS[kind]
    h = L.create(lib, without)
    try:
        expect(lib, A.require(set_params)(h, Bufs().d), INVALID_ARG, NO_PARAMETERS[kind])
    finally:
        L.destroy(lib, without, h)


def test_nm_phase_cycles_on_a_bounded_engine(lib):
    b = Bufs()
    cfg = L.nm_cfg()
    cfg.bounded = 1
    h = engine(lib, "nlsg_nm_create", cfg)
    try:
        expect(lib, lib.nlsg_nm_phase_cycles(h, b.d, b.q), UNSUPPORTED,
               "nlsg_nm_phase_cycles profiles unbounded engines")
        expect(lib, lib.nlsg_nm_minimize(h, b.d, None, None, b.status, None), INVALID_ARG,
               "bounded solver needs upper and lower")
    finally:
        assert lib.nlsg_nm_destroy(h) == 0


def test_nmpso_time_solve_on_a_bounded_engine(lib):
    b = Bufs()
    cfg = L.nmpso_cfg()
    cfg.bounded = 1
    h = engine(lib, "nlsg_nmpso_create", cfg)
    try:
        expect(lib, lib.nlsg_nmpso_time_solve(h, b.d, 1, C.byref(b.ms)), UNSUPPORTED,
               "timing aid of the unbounded overloads")
        expect(lib, lib.nlsg_nmpso_minimize(h, b.d, None, None, b.status), INVALID_ARG,
               "a bounded engine needs lower and upper")
    finally:
        assert lib.nlsg_nmpso_destroy(h) == 0


POISON = 0xAB


def _poisoned_status(n=2):
    st = (A.Status * n)()
    C.memset(st, POISON, C.sizeof(st))
    return st


def _check_one_launch_rows(st, tracks_std_err):
    """all ten fields written; the ones a one-launch engine does not track hold exactly what they always held"""
    poison_u64 = int.from_bytes(bytes([POISON]) * 8, "little")
    poison_f64 = np.frombuffer(bytes([POISON]) * 8, dtype=np.float64)[0]
    for b in range(2):
        s = st[b]
        assert np.isfinite(s.f_value) and s.f_value != poison_f64
        assert s.iteration <= 10  # (max_iter of the lifecycle configs)
        assert 1 <= s.function_calls_used < poison_u64
        assert s.gradient_evals_used == 0
        assert s.hessian_evals_used == 0
        assert s.best_index == b
        assert s.val_no_change == 0
        if tracks_std_err:
            assert np.isfinite(s.std_err) and s.std_err != poison_f64
        else:
            assert s.std_err == 0.0 and not np.signbit(s.std_err)
        assert s.done == 1
        assert s.reserved == 0


def test_nm_minimize_fills_every_status_field(lib):
    x, eps = np.array([[0.5, -0.5], [1.5, 0.25]]), np.full(2, np.nan)
    st = _poisoned_status()
    h = L.create(lib, "nm")
    try:
        rc = lib.nlsg_nm_minimize(h, x.ctypes.data_as(A.pd), None, None, st, eps.ctypes.data_as(A.pd))
        assert rc == 0, L.last_error(lib)
    finally:
        L.destroy(lib, "nm", h)
    _check_one_launch_rows(st, tracks_std_err=True)
    assert [st[0].std_err, st[1].std_err] == list(eps)  # the simplex's last std_err, in both places


def test_nmpso_minimize_fills_every_status_field(lib):
    x = np.array([[0.5, -0.5], [1.5, 0.25]])
    st = _poisoned_status()
    h = L.create(lib, "nmpso")
    try:
        rc = lib.nlsg_nmpso_minimize(h, x.ctypes.data_as(A.pd), None, None, st)
        assert rc == 0, L.last_error(lib)
    finally:
        L.destroy(lib, "nmpso", h)
    _check_one_launch_rows(st, tracks_std_err=False)


def test_sann_minimize_fills_every_status_field(lib):
    x = np.array([[0.5, -0.5], [1.5, 0.25]])
    st = _poisoned_status()
    h = L.create(lib, "sann")
    try:
        rc = lib.nlsg_sann_minimize(h, x.ctypes.data_as(A.pd), st)
        assert rc == 0, L.last_error(lib)
    finally:
        L.destroy(lib, "sann", h)
    _check_one_launch_rows(st, tracks_std_err=False)
