"""The register-resident DE generation (one wave per agent, 65 <= D <= 1024) against the synchronous
oracle, bit for bit over 30 generations, at the shapes where its shortened instruction sequences
could go wrong: the lane-mask bookkeeping of the range and crossover predicates (odd D: the
non-vector loads; one and several chunks; the last lane and the last chunk of a row), the
branch-free donor selectors (pop 5: fewer than three distinct candidates among 63, the literal donor
loop; pop 9: picks past candidate 6, the selector load; pop 300: the selector lanes), the scalar
buffer select, the 32 x 64 key products and the lean wave sum. Both strategies, Rosenbrock and
Sphere, and three regimes: the bound decides (CR 0.9, F 0.8, init width 4.096), it mixes (CR 0.9,
F 0.5, width 1.2), the gate is off and trials are accepted (CR 0.2, F 0.5, width 0.6).

Every generation compares population and scores (downloaded through the selectors), the status
counters, and the trace of an engine created with trace=True; an engine without trace runs the
fused turn beside it and is compared the same way.

The shard case: the oracle states shards of an even partition only (donors of agent a come from
[a / n * n, a / n * n + n), n = pop / shards), so a shard of 300 agents starts at a multiple of 300
inside a population that is one: shard_lo = 1200, shard_n = 300 of pop 4 200."""
import ctypes as C

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

GENS = 30
DIMS = [65, 66, 127, 128, 129, 256, 1024]
POPS = [5, 9, 300]
REGIMES = {"decides": (0.9, 0.8, 4.096), "mixes": (0.9, 0.5, 1.2), "accepts": (0.2, 0.5, 0.6)}


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def counters(st):
    return (st.iteration, st.function_calls_used, st.best_index, st.val_no_change, st.done)


def ref_counters(s):
    return (s.iter, s.fcalls, s.best_id, s.val_no_change, s.done)


def check_generation(tag, ref, traced, plain):
    P, S, T = traced.download(trace=True)
    assert np.array_equal(T, ref.trace), f"{tag}: trace"
    assert np.array_equal(bits(P), bits(ref.population)), f"{tag}: population"
    assert np.array_equal(bits(S), bits(ref.scores)), f"{tag}: scores"
    assert counters(traced.status()) == ref_counters(ref.s), f"{tag}: counters"
    if plain is not None:
        Pp, Sp = plain.download()
        assert np.array_equal(bits(Pp), bits(P)) and np.array_equal(bits(Sp), bits(S)), f"{tag}: fused turn"
        assert counters(plain.status()) == ref_counters(ref.s), f"{tag}: fused turn counters"


@pytest.mark.parametrize("obj", ["rosenbrock", "sphere"])
@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("strategy", [1, 0], ids=["random", "best"])
@pytest.mark.parametrize("pop", POPS)
@pytest.mark.parametrize("D", DIMS)
def test_thirty_generations_bit_exact(eng_mod, oracle, D, pop, strategy, regime, obj):
    CR, F, width = REGIMES[regime]
    kw = dict(strategy=strategy, CR=CR, F=F, eps=0.0, best_val_no_change=10**6)
    x0 = np.full(D, width)
    tag0 = f"{obj} D {D} pop {pop} strategy {strategy} {regime}"
    ref = O.DESyncRun(oracle, obj, pop, D, x0, trace=True, **kw)
    with eng_mod.DEEngine(obj, pop, D, trace=True, **kw) as traced, eng_mod.DEEngine(obj, pop, D, **kw) as plain:
        if regime != "accepts" and strategy == 1:
            assert traced.bound_state()[0] and plain.bound_state()[0], tag0
        traced.init(x0)
        plain.init(x0)
        P, S = plain.download()
        assert np.array_equal(bits(P), bits(ref.population)) and np.array_equal(bits(S), bits(ref.scores)), f"{tag0}: init"
        for g in range(1, GENS + 1):
            ref.step(1)
            traced.step(1)
            plain.step(1)
            check_generation(f"{tag0}: generation {g}", ref, traced, plain)
        # one more turn: its head scans generation 30 and copies the best row through its selector
        Pk, Sk = ref.population.copy(), ref.scores.copy()
        ref.step(1)
        plain.step(1)
        bx, bf, bi = plain.best()
        assert bi == ref.s.best_id and bf == Sk[bi] and np.array_equal(bx, Pk[bi]), f"{tag0}: best"


@pytest.mark.parametrize("D,pop", [(128, 300), (129, 9), (1024, 64)])
def test_bound_switched_off_is_the_same_run(eng_mod, oracle, monkeypatch, D, pop):
    kw = dict(strategy=1, CR=0.9, F=0.5, eps=0.0, best_val_no_change=10**6)
    x0 = np.full(D, 1.2)
    monkeypatch.delenv("NLSG_DE_BOUND", raising=False)
    on = eng_mod.DEEngine("rosenbrock", pop, D, **kw)
    monkeypatch.setenv("NLSG_DE_BOUND", "0")
    off = eng_mod.DEEngine("rosenbrock", pop, D, **kw)
    monkeypatch.delenv("NLSG_DE_BOUND")
    try:
        assert on.bound_state()[0] is True and off.bound_state()[0] is False
        on.init(x0)
        off.init(x0)
        for g in range(1, GENS + 1):
            on.step(1)
            off.step(1)
            (P, S), (Po, So) = on.download(), off.download()
            assert np.array_equal(bits(P), bits(Po)) and np.array_equal(bits(S), bits(So)), f"generation {g}"
            assert counters(on.status()) == counters(off.status()), f"generation {g}"
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("D", [66, 129, 256])
def test_upload_mid_run_resets_the_selectors(eng_mod, oracle, D):
    """After accepted trials the rows sit in both buffers; an upload puts every row back into the
    buffer of the current parity and clears the selector bytes, hints included."""
    pop = 300
    kw = dict(strategy=1, CR=0.9, F=0.3, eps=0.0, best_val_no_change=10**6)  # (F 0.3: all three paths)
    x0 = np.full(D, 1.2)
    accepted = 0
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, trace=True, **kw)
    with eng_mod.DEEngine("rosenbrock", pop, D, trace=True, **kw) as traced, \
            eng_mod.DEEngine("rosenbrock", pop, D, **kw) as plain:
        traced.init(x0)
        plain.init(x0)
        for g in range(1, 16):  # an odd number of generations: parity 1 at the upload
            ref.step(1)
            traced.step(1)
            plain.step(1)
            check_generation(f"D {D}: generation {g}", ref, traced, plain)
            accepted += int(np.sum(ref.trace[:, 4] == 1))
        assert accepted >= 100, accepted  # (the oracle's count, 143 at D 256: rows sit in both buffers)
        P = ref.population[::-1].copy() * 0.75  # other rows than the engine holds, in another order
        S = ref.scores[::-1].copy() * 0.5       # lowered scores: the bound decides more often
        for e in (traced, plain):
            e.upload(P, S)
        ref.population[:] = P
        ref.scores[:] = S
        Pu, Su = plain.download()
        assert np.array_equal(bits(Pu), bits(P)) and np.array_equal(bits(Su), bits(S))
        for g in range(16, GENS + 1):
            ref.step(1)
            traced.step(1)
            plain.step(1)
            check_generation(f"D {D}: generation {g} (after the upload)", ref, traced, plain)


@pytest.mark.parametrize("regime", ["decides", "mixes"])
def test_shard_that_does_not_start_at_zero(eng_mod, oracle, regime):
    """shard_lo = 1200, shard_n = 300 of pop 4 200: global agent ids key the draws, shard-local ones
    address rows, scores and selectors; a turn in its three pieces with the shard's own record."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pop, lo, n, D = 4200, 1200, 300, 128
    CR, F, width = REGIMES[regime]
    kw = dict(strategy=1, CR=CR, F=F, eps=0.0, best_val_no_change=10**6)
    x0 = np.full(D, width)
    ref = O.OracleShardEngine(oracle, "rosenbrock", pop, D, lo, n, **kw)
    ref.init(x0)
    rec_host = np.zeros(ref.record_doubles())
    with eng_mod.DEEngine("rosenbrock", pop, D, shard_lo=lo, shard_n=n, stream=stream, **kw) as eng:
        assert eng.bound_state()[0] is True
        rec = torch.zeros(eng.record_doubles(), dtype=torch.float64, device=dev)
        assert rec.numel() == rec_host.size
        eng.init(x0)
        P, S = eng.download()
        Pr, Sr = ref.shard()
        assert np.array_equal(bits(P), bits(Pr)) and np.array_equal(bits(S), bits(Sr)), "init"
        for g in range(1, GENS + 1):
            ref.turn_begin(rec_host.ctypes.data_as(C.c_void_p))
            ref.turn_generation()
            ref.turn_finalize(rec_host.ctypes.data_as(C.c_void_p), 1)
            eng.turn_begin(rec.data_ptr())
            eng.turn_generation()
            eng.turn_finalize(rec.data_ptr(), 1)
            P, S = eng.download()
            Pr, Sr = ref.shard()
            assert np.array_equal(bits(P), bits(Pr)), f"generation {g}: population"
            assert np.array_equal(bits(S), bits(Sr)), f"generation {g}: scores"
            # (minimum, its global index, "valid", the best row; sum and M2 are taken for eps > 0 only)
            rd = rec.cpu().numpy()
            assert np.array_equal(bits(rd[[0, 1, 4]]), bits(rec_host[[0, 1, 4]])) and \
                np.array_equal(bits(rd[5:]), bits(rec_host[5:])), f"generation {g}: record"
            st, s = eng.status(), ref.run.s
            assert (st.iteration, st.function_calls_used, st.best_index) == (s.iter, s.fcalls, s.best_id), f"generation {g}"
