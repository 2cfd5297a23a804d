"""The DE generation's half-row reject screen (kDeBoundScreen) on the device: two agents per wave,
each half-wave rejecting its trial on the bound's lane tree over coordinates 0..63 alone; what the
screen does not decide goes through the one-agent path.

Every generation's population, scores and trace are compared bit for bit with the oracle and with a
twin engine created under NLSG_DE_SCREEN=0 (rows are downloaded through the selectors, so bit 0 of
every selector is compared with them), bound_counts() with the bound's model (tests/_de_bound.py) on
both engines, and screen_counts() with the numpy restatement of tests/_de_screen.py fed with the
oracle's generations. The case list is the one tests/test_de_screen_cpu.py checks for coverage; the
last test repeats that check beside the device's counters."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle as O
from tests import _de_screen as M
from tests._de_bound import BoundModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_COUNTS = {}  # case id -> (screen_counts of the device, of the model)


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def make_engines(eng_mod, monkeypatch, obj, pop, D, kw, sr, trace=True, **more):
    """(engine, its twin created under NLSG_DE_SCREEN=0)"""
    for name in ("NLSG_DE_SCREEN", "NLSG_DE_SCREEN_RETRY", "NLSG_DE_BOUND", "NLSG_DE_BOUND_RETRY",
                 "NLSG_DE_BOUND_CR"):
        monkeypatch.delenv(name, raising=False)
    if sr is not None:
        monkeypatch.setenv("NLSG_DE_SCREEN_RETRY", str(sr))
    # the pair wave stays on whatever it decides: the model restates the screen, not the engine's
    # switching between its two launches (test_engine_drops_and_retries_the_pair_wave)
    monkeypatch.setenv("NLSG_DE_SCREEN_ADAPT", "0")
    eng = eng_mod.DEEngine(obj, pop, D, trace=trace, **kw, **more)
    monkeypatch.delenv("NLSG_DE_SCREEN_ADAPT")
    monkeypatch.setenv("NLSG_DE_SCREEN", "0")
    off = eng_mod.DEEngine(obj, pop, D, trace=trace, **kw, **more)
    monkeypatch.delenv("NLSG_DE_SCREEN")
    monkeypatch.delenv("NLSG_DE_SCREEN_RETRY", raising=False)
    assert off.screen_state()[0] is False
    return eng, off


class Run:
    """An engine, its NLSG_DE_SCREEN=0 twin, the oracle and the two models, stepped together."""

    def __init__(self, eng_mod, oracle, monkeypatch, c, expect_screen=True):
        obj, pop, D, CR, F, x0v, gens, seed, sr = c
        self.c, self.tag = c, M.case_id(c)
        self.kw = M.case_kw(c)
        self.x0 = np.full(D, x0v)
        self.ref = O.DESyncRun(oracle, obj, pop, D, self.x0, trace=True, **self.kw)
        self.eng, self.off = make_engines(eng_mod, monkeypatch, obj, pop, D, self.kw, sr)
        on, period = self.eng.screen_state()
        assert on is expect_screen and period == (sr or M.SCREEN_RETRY), self.tag
        assert self.eng.bound_state() == (True, M.BOUND_RETRY) == self.off.bound_state()
        self.model = M.ScreenModel(obj, pop, D, CR, F, seed, M.BOUND_RETRY, period, screen=on)
        self.bm = BoundModel(obj, pop, D, CR, F, seed, M.BOUND_RETRY)
        self.g = 0
        for e in (self.eng, self.off):
            e.init(self.x0)
        P, S = self.eng.download()
        assert same(P, self.ref.population) and same(S, self.ref.scores), f"{self.tag}: init"
        assert self.eng.screen_counts() == (0, 0) and self.eng.bound_counts() == (0, 0, 0)

    def close(self):
        self.eng.close()
        self.off.close()

    def step(self, gens):
        ref = self.ref
        for _ in range(gens):
            self.g += 1
            tag = f"{self.tag}: generation {self.g}"
            P0, S0 = ref.population.copy(), ref.scores.copy()
            ref.step(1)
            self.eng.step(1)
            self.off.step(1)
            self.model.generation(self.g, P0, S0, ref.trace)
            self.bm.generation(self.g, P0, S0, ref.trace)
            P, S, T = self.eng.download(trace=True)
            assert np.array_equal(T, ref.trace), f"{tag}: trace"
            assert same(P, ref.population), f"{tag}: population"
            assert same(S, ref.scores), f"{tag}: scores"
            st = self.eng.status()
            assert (st.iteration, st.function_calls_used, st.best_index, st.val_no_change) == \
                (ref.s.iter, ref.s.fcalls, ref.s.best_id, ref.s.val_no_change), f"{tag}: counters"
            assert self.eng.bound_counts() == tuple(self.bm.counts), f"{tag}: the bound's paths"
            assert self.eng.screen_counts() == tuple(self.model.screen_counts), f"{tag}: the screen's paths"
            Po, So, To = self.off.download(trace=True)
            assert np.array_equal(Po.view(np.uint64), P.view(np.uint64)) and \
                np.array_equal(So.view(np.uint64), S.view(np.uint64)) and np.array_equal(To, T), \
                f"{tag}: NLSG_DE_SCREEN=0"
            assert self.off.bound_counts() == tuple(self.bm.counts) and self.off.screen_counts() == (0, 0)

    def upload(self, P, S):
        for e in (self.eng, self.off):
            e.upload(P, S)
        self.ref.population[:] = P
        self.ref.scores[:] = S
        self.model.clear_bits()
        self.bm.clear_hints()


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_case(eng_mod, oracle, monkeypatch, c):
    r = Run(eng_mod, oracle, monkeypatch, c)
    try:
        r.step(c[6])
        DEVICE_COUNTS[r.tag] = (r.eng.screen_counts()[0], r.model.screen_counts[0])
        # one more turn: its head scans the last generation and copies the best row through the selector
        Pk, Sk = r.ref.population.copy(), r.ref.scores.copy()
        r.eng.step(1)
        r.ref.step(1)
        bx, bf, bi = r.eng.best()
        assert bi == r.ref.s.best_id and bf == Sk[bi] and np.array_equal(bx, Pk[bi]), f"{r.tag}: best"
    finally:
        r.close()
    print(f"{r.tag}: {dict(zip(M.NAMES, r.model.seen.tolist()))}")


@pytest.mark.parametrize("mode", ["fused", "serial", "overlap"])
def test_turn_modes_without_trace(eng_mod, oracle, monkeypatch, mode):
    """trace=False on one GPU: the fused turn (pair waves behind the head's blocks), head then
    generation, and the head on a side stream. A lone last agent at pop 33; pop 1000 in the bench regime."""
    monkeypatch.delenv("NLSG_DE_FUSED_TURN", raising=False)
    monkeypatch.delenv("NLSG_DE_OVERLAP", raising=False)
    if mode == "serial":
        monkeypatch.setenv("NLSG_DE_FUSED_TURN", "0")
    if mode == "overlap":
        monkeypatch.setenv("NLSG_DE_OVERLAP", "1")
    for obj, pop, D, F, x0v, gens in (("rosenbrock", 33, 127, 0.5, 1.2, 16), ("rosenbrock", 1000, 128, 0.8, 4.096, 6)):
        kw = dict(strategy=1, CR=0.9, F=F, eps=0.0, best_val_no_change=10**6)
        x0 = np.full(D, x0v)
        ref = O.DESyncRun(oracle, obj, pop, D, x0, **kw)
        eng, off = make_engines(eng_mod, monkeypatch, obj, pop, D, kw, 4, trace=False)
        try:
            assert eng.screen_state() == (True, 4)
            with pytest.raises(eng_mod.NlsgError):
                eng.screen_counts()
            for e in (eng, off):
                e.init(x0)
            for g in range(gens):
                ref.step(1)
                eng.step(1)
                off.step(1)
                P, S = eng.download()
                assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), f"{mode} pop {pop}: generation {g + 1}"
                Po, So = off.download()
                assert np.array_equal(Po, P) and np.array_equal(So, S)
                st = eng.status()
                assert (st.iteration, st.best_index, st.val_no_change) == (ref.s.iter, ref.s.best_id, ref.s.val_no_change)
        finally:
            eng.close()
            off.close()


def test_stop_test_fires_inside_a_fused_turn(eng_mod, oracle, monkeypatch):
    """max_iter 5: the head of turn 5 stops the solve while generation 6 runs beside it; that
    generation went to the other buffers and is never adopted, later turns are no-ops"""
    pop, D = 41, 128
    kw = dict(strategy=1, CR=0.9, F=0.5, eps=0.0, max_iter=5, best_val_no_change=10**6)
    x0 = np.full(D, 1.2)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    ref.step(9)
    assert ref.s.done
    eng, off = make_engines(eng_mod, monkeypatch, "rosenbrock", pop, D, kw, None, trace=False)
    try:
        for e in (eng, off):
            e.init(x0)
            e.step(9)
            st = e.status()
            P, S = e.download()
            bx, bf, bi = e.best()
            assert st.done == 1 and (st.iteration, st.best_index) == (ref.s.iter, ref.s.best_id)
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores)
            assert np.array_equal(bx, ref.best_x)
    finally:
        eng.close()
        off.close()


def test_three_odd_shards_on_one_gpu(eng_mod, oracle, monkeypatch):
    """the sharded turn's generation launch: island donors, shard-local agent indices in the retry
    rule, a lone last agent in every shard"""
    import torch
    for name in ("NLSG_DE_SCREEN", "NLSG_DE_BOUND"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("NLSG_DE_SCREEN_RETRY", "4")
    monkeypatch.setenv("NLSG_DE_SCREEN_ADAPT", "0")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    shards, n, D, turns, CR, F = 3, 33, 127, 14, 0.9, 0.5
    pop = shards * n
    x0 = np.full(D, 1.2)
    kw = dict(strategy=1, eps=0.0, best_val_no_change=1000, CR=CR, F=F)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, n_shards=shards, trace=True, **kw)
    engs = [eng_mod.DEEngine("rosenbrock", pop, D, shard_lo=r * n, shard_n=n, stream=stream, trace=True, **kw)
            for r in range(shards)]
    models = [M.ScreenModel("rosenbrock", pop, D, CR, F, M.SEED, M.BOUND_RETRY, 4, shard_lo=r * n, shard_n=n)
              for r in range(shards)]
    try:
        assert all(e.screen_state() == (True, 4) for e in engs)
        rec = engs[0].record_doubles()
        gathered = torch.zeros(shards * rec, dtype=torch.float64, device=dev)
        for e in engs:
            e.init(x0)
        for g in range(1, turns + 1):
            P0, S0 = ref.population.copy(), ref.scores.copy()
            ref.step(1)
            for r, e in enumerate(engs):
                e.turn_begin(gathered[r * rec:(r + 1) * rec].data_ptr())
            for e in engs:
                e.turn_generation()
            for e in engs:
                e.turn_finalize(gathered.data_ptr(), shards)
            for r, e in enumerate(engs):
                models[r].generation(g, P0, S0, ref.trace)
                P, S, T = e.download(trace=True)
                tag = f"shard {r} generation {g}"
                assert np.array_equal(T, ref.trace[r * n:(r + 1) * n]), tag
                assert np.array_equal(P, ref.population[r * n:(r + 1) * n]), tag
                assert np.array_equal(S, ref.scores[r * n:(r + 1) * n]), tag
                assert e.bound_counts() == tuple(models[r].bound_counts), tag
                assert e.screen_counts() == tuple(models[r].screen_counts), tag
        assert sum(m.screen_counts[0] for m in models) > 0 and sum(m.screen_counts[1] for m in models) > 0
    finally:
        for e in engs:
            e.close()


def test_upload_mid_run_clears_the_counts(eng_mod, oracle, monkeypatch):
    """Uploaded scores need not belong to their rows: NaN never compares, +inf is reached by no finite
    screen value, a huge finite one neither; lowered scores make the screen decide. Upload stores the
    parity in every selector byte: hints and miss counts start over."""
    c = ("rosenbrock", 40, 128, 0.9, 0.5, 1.2, 8, M.SEED, 4)
    r = Run(eng_mod, oracle, monkeypatch, c)
    try:
        r.step(8)
        assert r.model.sel.max() >= 4  # some agent carries a miss count into the upload
        P = r.ref.population.copy()
        S = r.ref.scores.copy()
        P[::3] *= 0.5
        S[1::4] *= 0.05
        S[2] = np.nan
        S[6] = np.inf
        S[10] = 1e300
        S[14] = -1.0
        r.upload(P, S)
        Pu, Su = r.eng.download()
        assert np.array_equal(Pu, P) and np.array_equal(Su.view(np.uint64), S.view(np.uint64))
        before = list(r.model.screen_counts)
        r.step(8)
        assert r.model.screen_counts[0] > before[0] and r.model.screen_counts[1] > before[1]
    finally:
        r.close()


def test_time_generation_kernel_then_init_then_steps(eng_mod, oracle, monkeypatch):
    """The timing entry point (ignore_done) advances rows, selectors, hints and miss counts without
    heads; init starts over with every selector byte cleared, and the solve after it is exact."""
    pop, D = 97, 128
    x0 = np.full(D, 1.2)
    kw = dict(CR=0.9, F=0.5, eps=0.0, max_iter=12, best_val_no_change=1000)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    ref.step(20)
    assert ref.s.done
    eng, off = make_engines(eng_mod, monkeypatch, "rosenbrock", pop, D, kw, None, trace=False)
    try:
        off.close()
        assert eng.screen_state()[0] is True
        eng.init(x0)
        eng.step(2)
        assert eng.time_generation_kernel(5) > 0
        eng.init(x0)
        eng.step(20)
        st = eng.status()
        P, S = eng.download()
        assert st.done == 1 and (st.iteration, st.best_index) == (ref.s.iter, ref.s.best_id)
        assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores)
    finally:
        eng.close()


def test_gate_edges_on_the_device(eng_mod, oracle, monkeypatch):
    """D 129 (two chunks) keeps the bound and does not screen; Sphere at D 128 screens (its case is
    in the list above); an objective outside the bound's gate does neither."""
    c = ("rosenbrock", 40, 129, 0.9, 0.5, 1.2, 6, M.SEED, None)
    r = Run(eng_mod, oracle, monkeypatch, c, expect_screen=False)
    try:
        r.step(6)
        assert sum(r.bm.counts) > 0 and r.eng.screen_counts() == (0, 0)
    finally:
        r.close()
    with eng_mod.DEEngine("sphere", 40, 128, CR=0.9, F=0.5) as e:
        assert e.screen_state()[0] is True and e.bound_state()[0] is True
    with eng_mod.DEEngine("styblinski_tang", 40, 128, CR=0.9, F=0.5) as e:
        assert e.screen_state()[0] is False and e.bound_state()[0] is False
    with eng_mod.DEEngine("rosenbrock", 40, 64, CR=0.9, F=0.5) as e:
        assert e.screen_state()[0] is False


def test_engine_drops_and_retries_the_pair_wave(eng_mod, oracle, monkeypatch):
    """Where the host reads the state it judges the share of agents the sampled pair waves decided
    since its last look: below 0.9 it goes back to the one-agent launches (screen_state reports it),
    1024 generations later it tries the pair wave again. The path changes, no output does. Never
    deciding (x0 1e-3): dropped at the first look that has 8 generations, retried after 1024. Bench
    regime: kept."""
    for name in ("NLSG_DE_SCREEN", "NLSG_DE_SCREEN_RETRY", "NLSG_DE_SCREEN_ADAPT", "NLSG_DE_BOUND"):
        monkeypatch.delenv(name, raising=False)
    pop, D = 41, 128
    kw = dict(strategy=1, CR=0.9, F=0.5, eps=0.0, max_iter=10**6, best_val_no_change=10**6)
    x0 = np.full(D, 1e-3)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    with eng_mod.DEEngine("rosenbrock", pop, D, **kw) as eng:
        eng.init(x0)
        assert eng.screen_state()[0] is True
        modes = []
        for steps in (4, 8, 8, 1020, 8, 8):  # looks after 4, 12, 20, 1040, 1048, 1056 generations
            eng.step(steps)
            ref.step(steps)
            P, S = eng.download()
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), steps
            modes.append(eng.screen_state()[0])
        # too few generations to judge; dropped; stays off; probe; judged again and dropped
        assert modes == [True, False, False, True, False, False], modes
        eng.init(x0)  # a new solve starts with the pair wave
        assert eng.screen_state()[0] is True
    kw = dict(strategy=1, CR=0.9, F=0.8, eps=0.0, max_iter=10**6, best_val_no_change=10**6)
    x0 = np.full(D, 4.096)
    ref = O.DESyncRun(oracle, "rosenbrock", 1000, D, x0, **kw)
    with eng_mod.DEEngine("rosenbrock", 1000, D, **kw) as eng:
        eng.init(x0)
        for steps in (10, 10, 10):
            eng.step(steps)
            ref.step(steps)
            P, S = eng.download()
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores)
            assert eng.screen_state()[0] is True
    monkeypatch.setenv("NLSG_DE_SCREEN_ADAPT", "0")
    with eng_mod.DEEngine("rosenbrock", pop, D, **dict(kw, F=0.5)) as eng:
        eng.init(np.full(D, 1e-3))
        eng.step(20)
        eng.status()
        assert eng.screen_state()[0] is True  # pinned


POISON_CHILD = r"""
import numpy as np
import nlsolver_amd
from nlsolver_amd import _capi
from tests import _oracle as O
from tests import _de_screen as M
c = ("rosenbrock", 33, 127, 0.9, 0.5, 1.2, 10, M.SEED, None)
obj, pop, D, CR, F, x0v, gens, seed, sr = c
x0 = np.full(D, x0v)
for rnd in range(2):  # the second engine takes the first one's blocks back from the pool
    ref = O.DESyncRun(O.load(), obj, pop, D, x0, trace=True, **M.case_kw(c))
    model = M.ScreenModel(obj, pop, D, CR, F, seed, M.BOUND_RETRY, M.SCREEN_RETRY)
    with nlsolver_amd.DEEngine(obj, pop, D, trace=True, **M.case_kw(c)) as eng:
        assert eng.screen_state()[0] is True
        assert _capi.lib().nlsg_pool_poison() == 0xFF  # the byte is in force
        eng.init(x0)
        for g in range(1, gens + 1):
            P0, S0 = ref.population.copy(), ref.scores.copy()
            ref.step(1)
            eng.step(1)
            model.generation(g, P0, S0, ref.trace)
            P, S, T = eng.download(trace=True)
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores) and np.array_equal(T, ref.trace), (rnd, g)
            assert eng.screen_counts() == tuple(model.screen_counts) and eng.bound_counts() == tuple(model.bound_counts), (rnd, g)
print("poison-ok screen")
"""


def test_poisoned_pool_blocks():
    """every block the pool hands out filled with 0xFF bytes (NLSG_POOL_POISON=1), in a child process:
    the pair wave reads no selector byte, counter or row it did not write"""
    env = dict(os.environ, NLSG_POOL_POISON="1", NLSG_DE_SCREEN_ADAPT="0")
    for name in ("NLSG_DE_SCREEN", "NLSG_DE_SCREEN_RETRY", "NLSG_DE_BOUND"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, "-c", POISON_CHILD], capture_output=True, text=True, env=env,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "poison-ok screen" in r.stdout, r.stderr[-3000:]


def test_zz_case_list_reaches_every_path(oracle):
    """From the model (fed with the oracle) every path is reached at least three times by the case
    list; from the counters, the device agreed with the model on every case it ran."""
    seen, retried = np.zeros(len(M.NAMES), dtype=np.int64), 0
    for c in M.CASES:
        model, r = M.run_model(O, oracle, c)
        seen += model.seen
        retried += r
    for k in (M.DECIDED, M.MISS_BOUND, M.MISS_ACCEPT, M.MISS_REJECT, M.FEW_DONORS, M.PAST_SIX, M.BACKED_OFF):
        assert seen[k] >= 3, (M.NAMES[k], int(seen[k]))
    assert retried >= 3
    for tag, (dev, mod) in DEVICE_COUNTS.items():
        assert dev == mod, tag
