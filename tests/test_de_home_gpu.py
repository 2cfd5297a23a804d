"""DE stores only accepted trial rows: each agent's row lives in buf[0] or buf[1] as a per-agent
selector says (DeParams.home). Every path that reads or writes the population is compared bit for
bit with the oracle in regimes that accept trials, so that after a few generations the rows are
spread over both buffers: the generation kernels of every layout, the fused turn whose speculative
generation a stop test discards, upload / download, the sharded turn, the timing entry point and
recycled (poisoned) pool blocks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng_mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def x0_for(D, val=0.6):
    return val * (1.0 + 0.001 * np.arange(D))


def accepting_generations(eng_mod, oracle, pop, D, strategy, CR, *, minimize=True, trace=True, turns=6):
    """`turns` single turns from x0 0.6 with F 0.5: trace (where kept), population, scores and counters of
    every generation equal the oracle's, then one more turn whose head scans the last generation and
    copies the best row through the selector. trace=False with strategy random runs the fused turn (head k
    and generation k + 1 in one launch), which a trace buffer switches off. Returns the number of accepted
    trials."""
    x0 = x0_for(D)
    kw = dict(strategy=strategy, CR=CR, F=0.5, eps=0.0, best_val_no_change=10**6, minimize=minimize)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, trace=trace, **kw)
    accepted = 0
    tag = f"pop {pop} D {D} strategy {strategy} minimize {minimize} trace {trace}"
    with eng_mod.DEEngine("rosenbrock", pop, D, trace=trace, **kw) as eng:
        eng.init(x0)
        P, S = eng.download()
        assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), f"{tag}: init"
        for g in range(turns):
            before = ref.scores.copy()
            eng.step(1)
            ref.step(1)
            if trace:
                P, S, T = eng.download(trace=True)
                assert np.array_equal(T, ref.trace), f"{tag}: trace gen {g}"
                assert int(T[:, 4].sum()) == int(np.sum(ref.scores != before)), f"{tag}: accept mask gen {g}"
            else:
                P, S = eng.download()
            assert np.array_equal(P, ref.population), f"{tag}: population gen {g}"
            assert np.array_equal(S, ref.scores), f"{tag}: scores gen {g}"
            st = eng.status()
            assert (st.iteration, st.function_calls_used, st.best_index, st.val_no_change) == \
                (ref.s.iter, ref.s.fcalls, ref.s.best_id, ref.s.val_no_change), f"{tag}: counters gen {g}"
            accepted += int(np.sum(ref.scores != before))
        # one more turn: its head scans the last generation and copies the best row through the selector
        Pk, Sk = ref.population.copy(), ref.scores.copy()
        eng.step(1)
        ref.step(1)
        bx, bf, bi = eng.best()
        assert bi == ref.s.best_id and bf == Sk[bi] and np.array_equal(bx, Pk[bi]), f"{tag}: best"
    return accepted


# D = 16 / 64: packed groups; 128: one wave per agent; 1000: 8 chunks, odd row length per lane
# pair; 1025 / 2048: the segment-streaming kernel (odd and even rows)
@pytest.mark.parametrize("D", [16, 64, 128, 1000, 1025, 2048])
@pytest.mark.parametrize("strategy", [0, 1])
@pytest.mark.parametrize("CR", [0.2, 0.01])
def test_accepting_generations_bit_exact(eng_mod, oracle, D, strategy, CR):
    """CR 0.2, F 0.5 from x0 0.6 accepts ~10 % of the trials at D <= 128; CR 0.01 (about one
    crossed coordinate) keeps accepting at D >= 1000, where CR 0.2 accepts next to nothing."""
    accepted = accepting_generations(eng_mod, oracle, 128 if D <= 128 else 64, D, strategy, CR)
    assert accepted > 0 or CR == 0.2


@pytest.mark.parametrize("D", [16, 128, 1025])
@pytest.mark.parametrize("strategy", [0, 1])
def test_upload_mid_run_then_steps(eng_mod, oracle, D, strategy):
    """After accepting generations the rows sit in both buffers; an upload puts a changed
    population into one of them, and the generations after it must read the uploaded rows."""
    pop = 96
    x0 = x0_for(D)
    kw = dict(strategy=strategy, CR=0.2 if D <= 128 else 0.01, F=0.5, eps=0.0, best_val_no_change=10**6)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    with eng_mod.DEEngine("rosenbrock", pop, D, **kw) as eng:
        eng.init(x0)
        eng.step(3)
        ref.step(3)
        P, S = eng.download()
        assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores)
        P2 = P.copy()
        P2[::3] *= 0.5  # every third row moved: these scores no longer match, as uploads allow
        S2 = S.copy()
        S2[1::4] += 1.0
        eng.upload(P2, S2)
        ref.population[:] = P2
        ref.scores[:] = S2
        Pu, Su = eng.download()
        assert np.array_equal(Pu, P2) and np.array_equal(Su, S2)
        for g in range(3):
            eng.step(1)
            ref.step(1)
            P, S = eng.download()
            assert np.array_equal(P, ref.population), f"population gen {g} after upload"
            assert np.array_equal(S, ref.scores), f"scores gen {g} after upload"


@pytest.mark.parametrize("D", [16, 128])
@pytest.mark.parametrize("mode", ["fused", "serial"])
def test_stop_inside_a_fused_turn_with_accepted_rows(eng_mod, oracle, D, mode, monkeypatch):
    """max_iter fires in head k while the same launch's speculative generation k + 1 accepts
    trials (its rows go to the slots that home_k does not point at): the state, the population
    and best_x stay those of generation k."""
    monkeypatch.setenv("NLSG_DE_FUSED_TURN", "1" if mode == "fused" else "0")
    pop = 512
    x0 = x0_for(D)
    for max_iter in (3, 6):
        kw = dict(CR=0.2, F=0.5, eps=0.0, max_iter=max_iter, best_val_no_change=1000)
        ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, trace=True, **kw)
        ref.step(max_iter + 5)
        assert ref.s.done and ref.s.iter == max_iter
        # the generation that the stop discards accepts trials: one more oracle generation shows it
        probe = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, trace=True,
                            **dict(kw, max_iter=1000))
        probe.step(max_iter + 1)
        assert probe.trace[:, 4].sum() > 0
        with eng_mod.DEEngine("rosenbrock", pop, D, **kw) as eng:
            eng.init(x0)
            eng.step(max_iter + 5)
            st = eng.status()
            P, S = eng.download()
            bx, bf, bi = eng.best()
        assert st.done == 1 and (st.iteration, st.function_calls_used, st.best_index) == \
            (ref.s.iter, ref.s.fcalls, ref.s.best_id)
        assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores)
        assert np.array_equal(bx, ref.best_x) and bf == ref.scores[bi]


def shards_on_one_gpu(eng_mod, oracle, shards, n, D, strategy, turns=6):
    """`shards` shard engines of n agents each on one device (island donors, one record exchange per
    turn) over accepting turns: every shard's rows, scores and counters equal the oracle's, the best row
    of each shard's record is read through its selectors."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pop = shards * n
    x0 = x0_for(D)
    kw = dict(strategy=strategy, eps=0.0, best_val_no_change=1000, CR=0.2, F=0.5)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, n_shards=shards, **kw)
    ref.step(turns - 1)
    P_last_head = ref.population.copy()  # what the last turn's head scanned
    ref.step(1)
    engs = [eng_mod.DEEngine("rosenbrock", pop, D, shard_lo=r * n, shard_n=n, stream=stream, **kw)
            for r in range(shards)]
    try:
        rec = engs[0].record_doubles()
        gathered = torch.zeros(shards * rec, dtype=torch.float64, device=dev)
        for e in engs:
            e.init(x0)
        speculate = engs[0].can_speculate()
        for _ in range(turns):
            for r, e in enumerate(engs):
                e.turn_begin(gathered[r * rec:(r + 1) * rec].data_ptr())
            if speculate:
                for e in engs:
                    e.turn_generation()
                for e in engs:
                    e.turn_finalize(gathered.data_ptr(), shards)
            else:
                for e in engs:
                    e.turn_end(gathered.data_ptr(), shards)
        for r, e in enumerate(engs):
            P, S = e.download()
            assert np.array_equal(P, ref.population[r * n:(r + 1) * n]), f"shard {r} population"
            assert np.array_equal(S, ref.scores[r * n:(r + 1) * n]), f"shard {r} scores"
            st = e.status()
            assert (st.best_index, st.iteration, st.function_calls_used) == \
                (ref.s.best_id, ref.s.iter, ref.s.fcalls)
            bx, bf, bi = e.best()
            assert np.array_equal(bx, P_last_head[bi])
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("strategy", [1, 0])
def test_eight_shards_on_one_gpu_accepting_bit_exact(eng_mod, oracle, strategy):
    """Eight shard engines on one device (island donors, one record exchange per turn), the best
    row of each shard's record read through its selectors, over enough accepting turns that every
    shard's rows are spread over both buffers."""
    shards_on_one_gpu(eng_mod, oracle, 8, 1024, 128, strategy)


@pytest.mark.parametrize("D", [16, 128, 2048])
def test_time_generation_kernel_then_init_then_solve(eng_mod, oracle, D):
    """The timing entry point advances the population (and the selectors) without heads; init
    must start over from buf[0] with every selector reset, and the solve after it is exact."""
    pop = 256 if D <= 128 else 64
    x0 = x0_for(D)
    kw = dict(CR=0.2 if D <= 128 else 0.01, F=0.5, eps=0.0, max_iter=12, best_val_no_change=1000)
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, x0, **kw)
    for _ in range(20):
        ref.step()
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


POISON_SCRIPT = r"""
import numpy as np, sys
sys.path.insert(0, %r)
import nlsolver_amd
from tests import _oracle as O
lib = O.load()
# twice, so that the second round of engines runs on recycled (and poisoned) blocks; the first
# generation reads selectors of parity 0 only, the later ones those the generations wrote
for rep in range(2):
    for D, CR in ((16, 0.2), (128, 0.2), (1025, 0.01)):
        pop = 256 if D <= 128 else 64
        x0 = 0.6 * (1.0 + 0.001 * np.arange(D))
        kw = dict(CR=CR, F=0.5, eps=0.0, best_val_no_change=1000, trace=True)
        ref = O.DESyncRun(lib, "rosenbrock", pop, D, x0, **kw); ref.step(5)
        with nlsolver_amd.DEEngine("rosenbrock", pop, D, **kw) as eng:
            eng.init(x0); eng.step(5); P, S, T = eng.download(trace=True)
        assert T[:, 4].sum() > 0
        assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), (rep, D)
print("poison-ok")
"""


def test_accepting_run_on_poisoned_pool_blocks():
    """NLSG_POOL_POISON=1 hands out every block filled with 0xFF bytes: a selector read before the
    engine wrote it would send a row to the wrong buffer."""
    env = dict(os.environ, NLSG_POOL_POISON="1")
    r = subprocess.run([sys.executable, "-c", POISON_SCRIPT % ROOT], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and "poison-ok" in r.stdout, r.stderr[-2000:]
