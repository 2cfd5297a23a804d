"""The DE generation's lower-bound rejection (DeParams.bound) on the device: a trial whose terms over
mutant coordinates alone already reach the agent's score is rejected without reading the agent's row;
an agent the bound did not decide carries a hint and tries it again every R-th generation.

Every generation's population, scores, trace and status counters are compared bit for bit with the
oracle, the path counters with the numpy restatement of tests/_de_bound.py fed with the oracle's
generations, and the whole run with a second engine created under NLSG_DE_BOUND=0.

The cases with expected figures run with NLSG_DE_BOUND_RETRY=1 (every agent tries the bound in every
generation), which is how the figures were taken on the oracle; each of them runs again with the
built-in retry period, where hinted agents take the plain path and are not counted."""
import numpy as np
import pytest

from tests import _oracle as O
from tests._de_bound import BoundModel

pytestmark = pytest.mark.gpu

SEED = 12374563468


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def make_engines(eng_mod, monkeypatch, obj, pop, D, kw, retry, trace=True):
    """(engine, the same engine created under NLSG_DE_BOUND=0). From CR 1 up the gate is closed
    (the plain path reads no own row there either): NLSG_DE_BOUND_CR opens it for the test."""
    monkeypatch.delenv("NLSG_DE_BOUND", raising=False)
    if kw["CR"] >= 1.0:
        monkeypatch.setenv("NLSG_DE_BOUND_CR", "0.8")
    else:
        monkeypatch.delenv("NLSG_DE_BOUND_CR", raising=False)
    if retry is None:
        monkeypatch.delenv("NLSG_DE_BOUND_RETRY", raising=False)
    else:
        monkeypatch.setenv("NLSG_DE_BOUND_RETRY", str(retry))
    eng = eng_mod.DEEngine(obj, pop, D, trace=trace, **kw)
    monkeypatch.setenv("NLSG_DE_BOUND", "0")
    off = eng_mod.DEEngine(obj, pop, D, trace=trace, **kw)
    monkeypatch.delenv("NLSG_DE_BOUND")
    monkeypatch.delenv("NLSG_DE_BOUND_RETRY", raising=False)
    monkeypatch.delenv("NLSG_DE_BOUND_CR", raising=False)
    assert off.bound_state()[0] is False
    return eng, off


def same(a, b):
    """equal, a NaN equal to a NaN (the host's and the device's default NaN differ in the sign bit)"""
    return np.array_equal(a, b, equal_nan=True)


class Run:
    """An engine, its NLSG_DE_BOUND=0 twin, the oracle and the path model, stepped together."""

    def __init__(self, eng_mod, oracle, monkeypatch, obj, pop, D, CR, F, x0v, *, retry=None,
                 minimize=True, strategy=1, expect_enabled=True):
        self.kw = dict(strategy=strategy, CR=CR, F=F, eps=0.0, best_val_no_change=10**6, minimize=minimize)
        self.tag = f"{obj} pop {pop} D {D} CR {CR} F {F} x0 {x0v} retry {retry}"
        self.x0 = np.full(D, x0v)
        self.ref = O.DESyncRun(oracle, obj, pop, D, self.x0, trace=True, **self.kw)
        self.eng, self.off = make_engines(eng_mod, monkeypatch, obj, pop, D, self.kw, retry)
        enabled, period = self.eng.bound_state()
        assert enabled is expect_enabled, self.tag
        assert period == (retry or period) and period & (period - 1) == 0
        self.period = period
        self.model = BoundModel(obj, pop, D, CR, F, SEED, period, enabled=enabled)
        self.g = 0
        for e in (self.eng, self.off):
            e.init(self.x0)
        P, S = self.eng.download()
        assert same(P, self.ref.population) and same(S, self.ref.scores), f"{self.tag}: init"
        assert self.eng.bound_counts() == (0, 0, 0)

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
            P, S, T = self.eng.download(trace=True)
            assert np.array_equal(T, ref.trace), f"{tag}: trace"
            assert same(P, ref.population), f"{tag}: population"
            assert same(S, ref.scores), f"{tag}: scores"
            st = self.eng.status()
            assert (st.iteration, st.function_calls_used, st.best_index, st.val_no_change) == \
                (ref.s.iter, ref.s.fcalls, ref.s.best_id, ref.s.val_no_change), f"{tag}: counters"
            assert self.eng.bound_counts() == tuple(self.model.counts), f"{tag}: paths"
            Po, So, To = self.off.download(trace=True)
            assert np.array_equal(Po, P) and np.array_equal(So.view(np.uint64), S.view(np.uint64)) and \
                np.array_equal(To, T), f"{tag}: NLSG_DE_BOUND=0"
            assert self.off.bound_counts() == (0, 0, 0)
        return tuple(self.model.counts)

    def upload(self, P, S):
        for e in (self.eng, self.off):
            e.upload(P, S)
        self.ref.population[:] = P
        self.ref.scores[:] = S
        self.model.clear_hints()


def run_case(eng_mod, oracle, monkeypatch, obj, pop, D, CR, F, x0v, gens, retry):
    r = Run(eng_mod, oracle, monkeypatch, obj, pop, D, CR, F, x0v, retry=retry)
    try:
        counts = r.step(gens)
        # one more turn: its head scans the last generation and copies the best row through the selector
        Pk, Sk = r.ref.population.copy(), r.ref.scores.copy()
        r.eng.step(1)
        r.ref.step(1)
        bx, bf, bi = r.eng.best()
        assert bi == r.ref.s.best_id and bf == Sk[bi] and np.array_equal(bx, Pk[bi]), f"{r.tag}: best"
    finally:
        r.close()
    print(f"{r.tag}: decided / not decided and rejected / accepted = {counts}")
    return counts


# Rosenbrock, strategy random, CR 0.9, F 0.3, x0 1.2, 10 generations: all three paths at D 128, at an
# odd D (the non-vector loads) and at a D whose last lane pair is half padding
MIXED = {128: (96, (468, 362, 130)), 129: (64, (320, 256, 64)), 130: (64, (330, 227, 83))}


@pytest.mark.parametrize("D", sorted(MIXED))
def test_mixed_paths_expected_figures(eng_mod, oracle, monkeypatch, D):
    pop, want = MIXED[D]
    counts = run_case(eng_mod, oracle, monkeypatch, "rosenbrock", pop, D, 0.9, 0.3, 1.2, 10, 1)
    assert min(counts) >= 30, counts  # no path goes untested
    assert counts == want


@pytest.mark.parametrize("D", sorted(MIXED))
def test_mixed_paths_built_in_retry_period(eng_mod, oracle, monkeypatch, D):
    counts = run_case(eng_mod, oracle, monkeypatch, "rosenbrock", MIXED[D][0], D, 0.9, 0.3, 1.2, 10, None)
    assert min(counts) > 0 and sum(counts) < 10 * MIXED[D][0], counts  # hinted agents took the plain path


def test_smallest_width(eng_mod, oracle, monkeypatch):
    counts = run_case(eng_mod, oracle, monkeypatch, "rosenbrock", 96, 66, 0.9, 0.5, 1.2, 12, 1)
    assert min(counts) >= 20, counts
    assert counts == (999, 124, 29)
    run_case(eng_mod, oracle, monkeypatch, "rosenbrock", 96, 66, 0.9, 0.5, 1.2, 12, None)


def test_eight_chunks_odd_lane_pair(eng_mod, oracle, monkeypatch):
    counts = run_case(eng_mod, oracle, monkeypatch, "rosenbrock", 32, 1000, 0.95, 0.2, 0.6, 6, 1)
    assert min(counts) >= 10, counts
    assert counts == (36, 141, 15)
    run_case(eng_mod, oracle, monkeypatch, "rosenbrock", 32, 1000, 0.95, 0.2, 0.6, 6, None)


@pytest.mark.parametrize("retry", [1, None])
def test_bound_always_decides_in_the_bench_regime(eng_mod, oracle, monkeypatch, retry):
    assert run_case(eng_mod, oracle, monkeypatch, "rosenbrock", 96, 128, 0.9, 0.8, 4.096, 4, retry) == (384, 0, 0)


@pytest.mark.parametrize("CR", [1.0, 1.5])
def test_no_kept_coordinate(eng_mod, oracle, monkeypatch, CR):
    """CR 1.0: no draw of these generations is kept; CR 1.5 sets cr_all. The bound is the score: one
    evaluation, no own-row load, accepted or rejected on it."""
    for retry in (1, None):
        counts = run_case(eng_mod, oracle, monkeypatch, "rosenbrock", 96, 128, CR, 0.5, 1.2, 8, retry)
        assert counts == (767, 0, 1)
    # without the switch an engine of this rate does not use the bound
    monkeypatch.delenv("NLSG_DE_BOUND_CR", raising=False)
    with eng_mod.DEEngine("rosenbrock", 96, 128, CR=CR, F=0.5) as eng:
        assert eng.bound_state()[0] is False


def test_sphere(eng_mod, oracle, monkeypatch):
    assert run_case(eng_mod, oracle, monkeypatch, "sphere", 96, 128, 0.9, 0.3, 1.2, 10, 1) == (645, 198, 117)
    run_case(eng_mod, oracle, monkeypatch, "sphere", 96, 128, 0.9, 0.3, 1.2, 10, None)


@pytest.mark.parametrize("which", ["styblinski_tang", "maximize", "best"])
def test_off_by_construction(eng_mod, oracle, monkeypatch, which):
    obj = "styblinski_tang" if which == "styblinski_tang" else "rosenbrock"
    r = Run(eng_mod, oracle, monkeypatch, obj, 96, 128, 0.9, 0.3, 1.2, minimize=which != "maximize",
            strategy=0 if which == "best" else 1, expect_enabled=False)
    try:
        assert r.step(5) == (0, 0, 0)
    finally:
        r.close()


@pytest.mark.parametrize("retry", [1, None])
def test_hostile_scores(eng_mod, oracle, monkeypatch, retry):
    """x0 1e200: squares overflow, inf - inf gives NaN terms and scores"""
    r = Run(eng_mod, oracle, monkeypatch, "rosenbrock", 96, 128, 0.9, 0.5, 1e200, retry=retry)
    try:
        assert not np.all(np.isfinite(r.ref.scores))
        r.step(3)
    finally:
        r.close()


@pytest.mark.parametrize("retry", [1, None])
def test_upload_mid_run(eng_mod, oracle, monkeypatch, retry):
    """Uploaded scores need not belong to their rows: lowered ones make the bound decide where the
    true score would not, raised ones the reverse; NaN never compares; -1.0 is below every bound."""
    r = Run(eng_mod, oracle, monkeypatch, "rosenbrock", 96, 128, 0.9, 0.3, 1.2, retry=retry)
    try:
        r.step(3)
        P = r.ref.population.copy()
        S = r.ref.scores.copy()
        P[::3] *= 0.5
        S[1::4] *= 0.25
        S[2::4] *= 8.0
        S[5] = np.nan
        S[7] = -1.0
        r.upload(P, S)
        Pu, Su = r.eng.download()
        assert np.array_equal(Pu, P) and np.array_equal(Su.view(np.uint64), S.view(np.uint64))
        before = list(r.model.counts)
        r.step(3)
        assert r.model.counts[0] > before[0] and sum(r.model.counts) > sum(before) + 96
    finally:
        r.close()


def test_hint_and_retry(eng_mod, oracle, monkeypatch):
    """x0 1e-3: every score is about D - 1 while the mutant-only terms of a trial sum to about
    0.8 (D - 1), so the bound never decides. After the first generation every agent is hinted and
    tries again only when (generation + a) & (R - 1) == 0."""
    pop, D = 64, 128
    r = Run(eng_mod, oracle, monkeypatch, "rosenbrock", pop, D, 0.9, 0.5, 1e-3)
    try:
        R = r.period
        gens = 2 * R + 2
        counts = r.step(gens)
        tries = pop + sum(int(np.sum(((g + np.arange(pop)) & (R - 1)) == 0)) for g in range(2, gens + 1))
        assert counts[0] == 0 and counts[1] + counts[2] == tries, (counts, tries)
        assert tries < pop * gens or R == 1
    finally:
        r.close()


def test_without_trace_fused_turn(eng_mod, oracle, monkeypatch):
    """trace=False with strategy random on one GPU runs the fused turn; no counters, no atomics"""
    pop, D = 96, 128
    kw = dict(strategy=1, CR=0.9, F=0.3, eps=0.0, best_val_no_change=10**6)
    x0 = np.full(D, 1.2)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    eng, off = make_engines(eng_mod, monkeypatch, "rosenbrock", pop, D, kw, None, trace=False)
    try:
        assert eng.bound_state()[0] is True
        with pytest.raises(eng_mod.NlsgError):
            eng.bound_counts()
        for e in (eng, off):
            e.init(x0)
        for g in range(10):
            ref.step(1)
            eng.step(1)
            off.step(1)
            P, S = eng.download()
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), f"generation {g + 1}"
            Po, So = off.download()
            assert np.array_equal(Po, P) and np.array_equal(So, S)
            st = eng.status()
            assert (st.iteration, st.best_index, st.val_no_change) == (ref.s.iter, ref.s.best_id, ref.s.val_no_change)
    finally:
        eng.close()
        off.close()


def test_without_trace_eight_shards_on_one_gpu(eng_mod, oracle):
    """the sharded turn's generation launch (island donors, shard-local agent indices)"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    shards, n, D, turns = 8, 64, 128, 8
    pop = shards * n
    x0 = np.full(D, 1.2)
    kw = dict(strategy=1, eps=0.0, best_val_no_change=1000, CR=0.9, F=0.3)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, n_shards=shards, **kw)
    ref.step(turns - 1)
    P_last_head = ref.population.copy()
    ref.step(1)
    engs = [eng_mod.DEEngine("rosenbrock", pop, D, shard_lo=r * n, shard_n=n, stream=stream, **kw)
            for r in range(shards)]
    try:
        assert all(e.bound_state()[0] for e in engs)
        rec = engs[0].record_doubles()
        gathered = torch.zeros(shards * rec, dtype=torch.float64, device=dev)
        for e in engs:
            e.init(x0)
        assert engs[0].can_speculate()
        for _ in range(turns):
            for r, e in enumerate(engs):
                e.turn_begin(gathered[r * rec:(r + 1) * rec].data_ptr())
            for e in engs:
                e.turn_generation()
            for e in engs:
                e.turn_finalize(gathered.data_ptr(), shards)
        for r, e in enumerate(engs):
            P, S = e.download()
            assert np.array_equal(P, ref.population[r * n:(r + 1) * n]), f"shard {r} population"
            assert np.array_equal(S, ref.scores[r * n:(r + 1) * n]), f"shard {r} scores"
            st = e.status()
            assert (st.best_index, st.iteration, st.function_calls_used) == (ref.s.best_id, ref.s.iter, ref.s.fcalls)
            bx, bf, bi = e.best()
            assert np.array_equal(bx, P_last_head[bi])
    finally:
        for e in engs:
            e.close()


def test_without_trace_time_generation_kernel_then_init_then_steps(eng_mod, oracle):
    """The timing entry point advances rows, selectors and hints without heads; init starts over
    with every selector and hint cleared, and the solve after it is exact."""
    pop, D = 96, 128
    x0 = np.full(D, 1.2)
    kw = dict(CR=0.9, F=0.3, eps=0.0, max_iter=12, best_val_no_change=1000)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    ref.step(20)
    assert ref.s.done
    with eng_mod.DEEngine("rosenbrock", pop, D, **kw) as eng:
        eng.init(x0)
        eng.step(2)
        eng.time_generation_kernel(5)
        eng.init(x0)
        P, S = eng.download()
        r0 = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
        assert np.array_equal(P, r0.population) and np.array_equal(S, r0.scores)
        eng.step(20)
        st = eng.status()
        P, S = eng.download()
        bx, bf, bi = eng.best()
    assert st.done == 1 and (st.iteration, st.best_index) == (ref.s.iter, ref.s.best_id)
    assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores)
    assert np.array_equal(bx, ref.best_x)
