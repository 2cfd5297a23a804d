"""The screening wave on the boundaries of its layout: four agents per wave (de_generation_screen),
planned eight lanes per agent and screened two at a time, four waves per block. Populations that end
inside a wave, one agent short of a block, and a block and a lone agent; odd D (loads of single
coordinates); accepting regimes, declines, back-off and retry.

The comparison is tests/test_de_screen_gpu.py's Run: the engine, its NLSG_DE_SCREEN=0 twin, the
oracle, ScreenModel and BoundModel, every generation on population, scores, trace, status counters
and both count tuples. The case list (tests/_de_octet.py) is the one tests/test_de_picks_cpu.py
checks the pick rule on."""
import numpy as np
import pytest

from tests import _oracle as O
from tests import _de_screen as M
from tests import _de_octet as X
from tests.test_de_screen_gpu import Run, eng_mod, make_engines  # noqa: F401 (eng_mod: a fixture)

pytestmark = pytest.mark.gpu

DEVICE_COUNTS = {}  # case id -> (screen_counts of the device, of the model)


@pytest.mark.parametrize("c", X.CASES, ids=M.case_id)
def test_case(eng_mod, oracle, monkeypatch, c):
    r = Run(eng_mod, oracle, monkeypatch, c)
    try:
        r.step(c[6])
        DEVICE_COUNTS[r.tag] = (r.eng.screen_counts(), tuple(r.model.screen_counts))
        # one more turn: its head scans the last generation and copies the best row through the selector
        Pk, Sk = r.ref.population.copy(), r.ref.scores.copy()
        r.eng.step(1)
        r.ref.step(1)
        bx, bf, bi = r.eng.best()
        assert bi == r.ref.s.best_id and bf == Sk[bi] and np.array_equal(bx, Pk[bi]), f"{r.tag}: best"
    finally:
        r.close()
    print(f"{r.tag}: {dict(zip(M.NAMES, r.model.seen.tolist()))}")


@pytest.mark.parametrize("mode", ["fused", "serial"])
def test_turn_modes_without_trace_at_pop_17(eng_mod, oracle, monkeypatch, mode):
    """trace=False: the fused turn (screening waves behind the head's blocks; NLSG_DE_FUSED_TURN
    default) and head then generation (=0), a full block and a lone agent"""
    monkeypatch.delenv("NLSG_DE_FUSED_TURN", raising=False)
    monkeypatch.delenv("NLSG_DE_OVERLAP", raising=False)
    if mode == "serial":
        monkeypatch.setenv("NLSG_DE_FUSED_TURN", "0")
    for obj, pop, D, F, x0v, gens in (("rosenbrock", 17, 128, 0.8, 4.096, 12), ("rosenbrock", 17, 127, 0.5, 1.2, 16)):
        kw = dict(strategy=1, CR=0.9, F=F, eps=0.0, best_val_no_change=10**6)
        x0 = np.full(D, x0v)
        ref = O.DESyncRun(oracle, obj, pop, D, x0, **kw)
        eng, off = make_engines(eng_mod, monkeypatch, obj, pop, D, kw, 4, trace=False)
        try:
            assert eng.screen_state() == (True, 4)
            for e in (eng, off):
                e.init(x0)
            for g in range(gens):
                ref.step(1)
                eng.step(1)
                off.step(1)
                P, S = eng.download()
                assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), f"{mode} D {D}: generation {g + 1}"
                Po, So = off.download()
                assert np.array_equal(Po, P) and np.array_equal(So, S)
                st = eng.status()
                assert (st.iteration, st.best_index, st.val_no_change) == (ref.s.iter, ref.s.best_id, ref.s.val_no_change)
        finally:
            eng.close()
            off.close()


def test_zz_case_list_reaches_every_path(oracle):
    """From the model (fed with the oracle): the list holds what tests/_de_octet.py says it does, every
    path of the wave among it; from the counters, the device agreed with the model on every case it ran."""
    got, bad_ok, bad_picks = X.coverage(O, oracle)
    assert (bad_ok, bad_picks) == (0, 0)
    assert got == X.WANT
    for name, n in got.items():
        assert n >= 1, name
    for tag, (dev, mod) in DEVICE_COUNTS.items():
        assert dev == mod, tag
