"""An engine made and released through the Python classes gives the device pool back what the same
create / destroy cycle gives back through the C-ABI (nlsolver_amd/_engine.py owns close, `with` and
__del__ for all ten classes): the bytes parked afterwards are those of tests/golden/
engine_cached_bytes.json, whichever way the object goes, and a constructor whose run-time compilation
fails leaves the recorded bytes and no handle. Shapes and cases are tests/_engine_lifecycle.py's."""
import gc
import sys

import numpy as np
import pytest

import nlsolver_amd as N
from nlsolver_amd import _capi
from tests import _engine_lifecycle as L

pytestmark = pytest.mark.gpu

GOLD = L.golden()
_PSO = dict(inertia=0.7, cognitive=1.5, social=1.5, eps=1e-3, max_iter=10)
# ENGINES entry -> (class, arguments after the objective, keywords): the config of that entry, field for field
KINDS = {
    "de": (N.DEEngine, (8, 2), dict(trace=True, seed=1, eps=1e-3, max_iter=10)),
    "de_ref": (N.DERefEngine, (2, 4, 2), dict(log_capacity=2, eps=1e-3, max_iter=10)),
    "de_batch": (N.DEBatchEngine, (2, 4, 2), dict(eps=1e-3, max_iter=10)),
    "pso": (N.PSOEngine, (4, 2), dict(seed=1, **_PSO)),
    "pso_batch": (N.PSOBatchEngine, (2, 4, 2), _PSO),
    "bfgs": (N.BFGSEngine, (2,), dict(dim=2, max_iter=10, grad_eps=1e-6)),
    "lm_objective": (N.LMEngine, (), dict(batch=2, n=2, lam=1e-3, up=10.0, down=0.1, max_iter=10, f_delta=1e-8)),
    "nm": (N.NMEngine, (2, 2), dict(step=1.0, max_iter=10, no_change_best_tol=10)),
    "nmpso": (N.NMPSOEngine, (2, 2), dict(inertia=0.7, cognitive=1.5, social=1.5, max_iter=10,
                                          no_change_best_iter=10, seed=1)),
    "sann": (N.SANNEngine, (2, 2), dict(max_iter=10, seed=1)),
}
WITH_PARAMS = {with_p: without for with_p, without, _ in L.PARAM_KINDS.values()}  # "nm_params" -> "nm", ...
CASES = sorted(KINDS) + sorted(WITH_PARAMS)


def _parts(name):
    """(class, objective, arguments, keywords) of the ENGINES entry `name`"""
    cls, args, kw = KINDS[WITH_PARAMS.get(name, name)]
    if name in WITH_PARAMS:
        return cls, N.CustomObjective(L.WITH_P.decode(), n_params=1), args, kw
    return cls, "rosenbrock", args, kw  # (objective 0; BFGSEngine takes built-ins by name only)


@pytest.fixture(scope="module")
def lib():
    lib = _capi.lib()
    yield lib
    lib.nlsg_release_cached()


@pytest.fixture
def unraisable():
    seen, hook = [], sys.unraisablehook
    sys.unraisablehook = lambda u: seen.append(repr(u.exc_value))
    yield seen
    sys.unraisablehook = hook


def _with(make):
    with make() as eng:
        assert eng._h.value
    assert not eng._h.value


def _close_twice(make):
    eng = make()
    eng.close()
    eng.close()
    assert not eng._h.value


def _collected(make):
    eng = make()
    assert eng._h.value
    del eng
    gc.collect()


@pytest.mark.parametrize("name", CASES)
def test_released_engine_parks_the_recorded_bytes(lib, unraisable, name):
    cls, objective, args, kw = _parts(name)
    with cls(objective, *args, **kw) as eng:  # the same create: the C-ABI case's config, byte for byte
        assert bytes(eng.cfg) == bytes(L.ENGINES[name][2])
    for release in (_with, _close_twice, _collected):
        L.emptied(lib)
        release(lambda: cls(objective, *args, **kw))
        assert int(lib.nlsg_cached_bytes()) == GOLD["cycle"][name], release.__name__
    L.emptied(lib)
    assert unraisable == []


def _failing(name):
    """(class, constructor arguments, keywords) of the RTC_FAILURES entry `name`"""
    if name == "lm_curve":
        return N.LMEngine, (N.CurveModel(np.zeros((2, 3)), np.zeros((2, 3)), "r = y +;", 2),), KINDS["lm_objective"][2]
    if name == "lm_link":
        model = N.LinkRegression(np.zeros((2, 3, 2)), np.zeros((2, 3)), "return z +;", "return 1.0;")
        return N.LMEngine, (model,), KINDS["lm_objective"][2]
    cls, args, kw = KINDS["lm_objective" if name == "lm" else name]
    return cls, (N.CustomObjective(L.BAD.decode()),) + args, kw


@pytest.mark.parametrize("name", sorted(L.RTC_FAILURES))
def test_constructor_whose_compilation_fails_leaves_no_handle(lib, unraisable, name):
    cls, args, kw = _failing(name)
    L.emptied(lib)
    eng = cls.__new__(cls)
    with pytest.raises(N.NlsgError) as e:
        eng.__init__(*args, **kw)
    assert e.value.code == GOLD["rtc_failure"][name]["code"] and "does not compile" in str(e.value)
    assert bytes(eng.cfg) == bytes(L.RTC_FAILURES[name][1])
    parked = GOLD["rtc_failure"][name]["bytes"]
    assert int(lib.nlsg_cached_bytes()) == parked
    assert not eng._h.value  # nothing to destroy: close and the collector leave the pool as it is
    eng.close()
    del eng, e
    gc.collect()
    assert int(lib.nlsg_cached_bytes()) == parked
    L.emptied(lib)
    assert unraisable == []
