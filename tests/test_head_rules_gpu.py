"""The head of a DE / PSO turn on the device (de_scan_head_block, de_finalize_kernel, finish_turn,
pso_finish_turn and the finalisers) against the independent references of tests/_head_ref.py on
hostile scores: ties, NaN / inf, ill-conditioned samples. tests/test_head_rules_cpu.py holds the
C restatement to the same references, so device and restatement cannot be wrong together.

DE scores are uploaded: row i of the population is filled with i, so best()'s row names the
agent. Turn 1 scans a vector whose unique minimum puts the incumbent where the case wants it,
turn 2 scans the hostile vector (an upload overwrites what the generation between them did).

std_err is held to |dev - exact| / exact <= L u (2 + 2 kappa) + (L u kappa)^2 with u = 2^-53 and
L = 32 roundings on the longest path of the two-level block tree (derivation:
tests/_head_common.py; the measured worst ratios per family: tests/test_head_rules_cpu.py),
L + world + 3 across `world` shards; it is also bit-equal to the restatement's tree.

Mutation checks run on an MI355X (each mutated library failed, by a comparison with the Python
references, not only with the restatement):
  `<` flipped to `<=` in argmin_combine     test_de_head_follows_the_reference and
      test_de_shards_decide_as_one_scan (ties/dup_around_incumbent_beaten,
      ties/two_valued_min_first_and_last, nonfinite/neg_inf_twice: a later index wins)
  the merge term n_t (dm dm) dropped        the same two tests at 1025 and 2049 (std_err outside
      the bound in every ties / conditioning vector of more than one tile)
  kTile as the ragged tile's n_t            the same two and test_de_stop_tests_fire_and_hold[2049]
      (std_err; ties/all_equal no longer gives 0 and misses the eps stop)
  incumbent branch of de_scan_head_block removed   all three (ties/all_equal,
      ties/dup_around_incumbent_tied, -0.0 against +0.0, nonfinite/nan_at_incumbent)
  the kernels before the fixes              test_de_shards_decide_as_one_scan (NaN incumbent in a
      later rank: nan_at_incumbent, nan_everywhere_but_0, ...) and nonfinite/all_1e308 (NaN
      where the literal formula gives +inf) in both"""
import math

import numpy as np
import pytest

from tests import _head_ref as R
from tests import _head_common as H

pytestmark = pytest.mark.gpu

SIZES = H.SIZES  # 263169 = 257 tiles + 1: a second trip of the last block's 256-strided loops
L_UNSHARDED, L_sharded = H.L_UNSHARDED, H.L_sharded


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    return nlsolver_amd


_ROWS = {}


def rows_for(n, D):
    if (n, D) not in _ROWS:
        _ROWS.clear()
        _ROWS[(n, D)] = np.repeat(np.arange(n, dtype=np.float64)[:, None], D, axis=1)
    return _ROWS[(n, D)]


def device_turns(eng, n, D, vectors):
    """init, then per vector: upload it under the rows 0 .. n-1 and make one turn"""
    rows = rows_for(n, D)
    eng.init(np.ones(D))
    for v in vectors:
        eng.upload(rows, v)
        eng.step(1)
    st = eng.status()
    bx, bf, bi = eng.best()
    return st, bx, bf, bi


def compare(tag, st, bx, bf, bi, want, f_value, bad):
    got = (st.best_index, st.val_no_change, st.iteration, bool(st.done))
    if got != want:
        bad.append(f"{tag}: (best, vnc, iter, done) {got} != reference {want}")
    if not R.same_double(st.f_value, f_value) or not R.same_double(bf, f_value):
        bad.append(f"{tag}: f_value {st.f_value!r} / {bf!r} != reference {f_value!r}")
    if bi != want[0] or not np.all(bx == float(want[0])):
        bad.append(f"{tag}: best() gives agent {bi} row {bx[:2]}, reference agent {want[0]}")


def check_std_err(tag, c, got, want_bits, L, bad):
    if not R.same_double(got, want_bits):
        bad.append(f"{tag}: std_err {got!r} != restatement {want_bits!r}")
    if c.judge:
        ok, _, text = R.judge_std_err(got, c.vec, L)
        if not ok:
            bad.append(f"{tag}: std_err {text}")


def tree_std_err(oracle, vec):
    v = np.ascontiguousarray(vec, dtype=np.float64)
    m2 = oracle.orc_tiled_m2_merged(H.O._ptr(v), v.size, None)
    return math.sqrt(m2 / (v.size - 1)) if m2 == m2 else math.nan


# ---- DE, one device ------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("strategy", [1, 0], ids=["random", "best"])
def test_de_head_follows_the_reference(mod, oracle, monkeypatch, n, fused, strategy):
    monkeypatch.setenv("NLSG_DE_FUSED_TURN", fused)
    bad = []
    with mod.DEEngine("sphere", n, 2, strategy=strategy, eps=R.EPS_TINY, max_iter=1000,
                      best_val_no_change=10 ** 6) as eng:
        for c in R.cases(n):
            tag = f"{c.name} inc {c.inc}"
            st, bx, bf, bi = device_turns(eng, n, 2, [c.place, c.vec])
            compare(tag, st, bx, bf, bi, c.want, c.f_value, bad)
            check_std_err(tag, c, st.std_err, tree_std_err(oracle, c.vec), L_UNSHARDED, bad)
    assert not bad, f"n {n}: {len(bad)} mismatches\n" + "\n".join(bad[:40])


def test_de_head_long_rows(mod, oracle):
    """D = 1026: the segment-streaming layout copies best_x from rows longer than a wave holds"""
    n, D = 257, 1026
    bad = []
    with mod.DEEngine("sphere", n, D, eps=R.EPS_TINY, max_iter=1000, best_val_no_change=10 ** 6) as eng:
        for c in R.cases(n):
            tag = f"{c.name} inc {c.inc}"
            st, bx, bf, bi = device_turns(eng, n, D, [c.place, c.vec])
            compare(tag, st, bx, bf, bi, c.want, c.f_value, bad)
            check_std_err(tag, c, st.std_err, tree_std_err(oracle, c.vec), L_UNSHARDED, bad)
    assert not bad, f"{len(bad)} mismatches\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("n", [5, 257, 2049])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_de_stop_tests_fire_and_hold(mod, monkeypatch, n, fused):
    """val_no_change against best_val_no_change in {1, 2}; std_err against eps a factor of 2
    below and above the exact statistic: each stop test is seen to fire and to hold."""
    monkeypatch.setenv("NLSG_DE_FUSED_TURN", fused)
    inc = n // 2
    seen = set()
    fams = R.families(n, inc, which=("ties", "conditioning"))
    fams = [f for f in fams if f[0].startswith("conditioning")] + fams[:3]
    for name, vec in fams:
        for bvnc in (1, 2):
            place = R.placement(n, inc)
            h = R.RefDEHead(best_val_no_change=bvnc)
            h.turn(place)
            h.turn(vec)
            with mod.DEEngine("sphere", n, 2, eps=0.0, best_val_no_change=bvnc) as eng:
                st, bx, bf, bi = device_turns(eng, n, 2, [place, vec])
            bad = []
            compare(f"{name} bvnc {bvnc}", st, bx, bf, bi,
                    (h.best_id, h.val_no_change, h.iter, h.done), h.f_value, bad)
            assert not bad, bad
            seen.add(("vnc", h.done))
        if not R.std_err_precondition(vec):
            continue
        exact, _ = R.exact_std_err(vec)
        if not exact > 1e-300:
            continue
        for eps, fires in ((exact / 2, False), (2 * exact, True)):
            place = R.placement(n, inc, scale=max(1.0, 4 * eps))  # the placing turn must not stop
            h = R.RefDEHead(eps=eps, best_val_no_change=10 ** 6)
            h.turn(place)
            h.turn(vec)
            assert h.done == fires
            with mod.DEEngine("sphere", n, 2, eps=eps, best_val_no_change=10 ** 6) as eng:
                st, bx, bf, bi = device_turns(eng, n, 2, [place, vec])
            bad = []
            compare(f"{name} eps {eps}", st, bx, bf, bi,
                    (h.best_id, h.val_no_change, h.iter, h.done), h.f_value, bad)
            assert not bad, bad
            seen.add(("eps", fires))
    assert seen == {("vnc", True), ("vnc", False), ("eps", True), ("eps", False)}


# ---- DE, shards on one device ----------------------------------------------------------------
@pytest.mark.parametrize("m", H.SHARD_SIZES)
@pytest.mark.parametrize("world", H.WORLDS)
@pytest.mark.parametrize("order", ["turn_end", "speculative"])
def test_de_shards_decide_as_one_scan(mod, oracle, world, m, order):
    """`world` shard engines on torch's current stream; the records are exchanged through
    adjacent slices of one tensor. Every shard's status equals RefDEHead on the GLOBAL vector:
    equal minima in several shards, all-NaN shards (valid = 0), a NaN incumbent in a later rank."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = world * m
    strategy = 1 if order == "speculative" else 0
    kw = dict(strategy=strategy, eps=R.EPS_TINY, max_iter=1000, best_val_no_change=10 ** 6)
    engs = [mod.DEEngine("sphere", n, 2, shard_lo=r * m, shard_n=m, stream=stream, **kw)
            for r in range(world)]
    rec = engs[0].record_doubles()
    gathered = torch.zeros(world * rec, dtype=torch.float64, device=dev)
    assert engs[0].can_speculate() == (strategy == 1)
    rows = rows_for(n, 2)
    run = H.make_run(oracle, n, world)
    bad = []
    for c in R.cases(n, world):
        tag = f"{c.name} inc {c.inc}"
        for e in engs:
            e.init(np.ones(2))
        for v in (c.place, c.vec):
            for r, e in enumerate(engs):
                e.upload(rows[r * m:(r + 1) * m], v[r * m:(r + 1) * m])
            for r, e in enumerate(engs):
                e.turn_begin(gathered[r * rec:(r + 1) * rec].data_ptr())
            if order == "speculative":
                for e in engs:
                    e.turn_generation()
                for e in engs:
                    e.turn_finalize(gathered.data_ptr(), world)
            else:
                for e in engs:
                    e.turn_end(gathered.data_ptr(), world)
        want_se = H.oracle_turns(run, [c.place, c.vec], eps=R.EPS_TINY)[4]
        for r, e in enumerate(engs):
            st = e.status()
            bx, bf, bi = e.best()
            compare(f"{tag} shard {r}", st, bx, bf, bi, c.want, c.f_value, bad)
            check_std_err(f"{tag} shard {r}", c, st.std_err, want_se, L_sharded(world), bad)
    for e in engs:
        e.close()
    assert not bad, f"world {world} m {m}: {len(bad)} mismatches\n" + "\n".join(bad[:40])


# ---- hostile objectives: PSO, and DE's acceptance rule ----------------------------------------
OBJECTIVES = {
    "ties": ("return floor(x(0) * 8);", lambda P: np.floor(P[:, 0] * 8)),
    "nan": ('return x(1) > 0.5 ? __builtin_nan("") : x(0);',
            lambda P: np.where(P[:, 1] > 0.5, np.nan, P[:, 0])),
    "inf": ("return x(1) > 0.5 ? __builtin_inf() : x(0);",
            lambda P: np.where(P[:, 1] > 0.5, np.inf, P[:, 0])),
}


def same_array(a, b):
    return np.array_equal(a, b, equal_nan=True)


# (shards, eps): one device with the single-launch head (eps = 0) and with the std_err kernels and
# the finaliser over its own record (eps > 0); four shards with records, std_err and the finaliser
PSO_LAYOUTS = [(1, 0.0), (1, R.EPS_TINY), (4, R.EPS_TINY)]


@pytest.mark.parametrize("m", [255, 1025, 4096])
@pytest.mark.parametrize("ptype", [0, 1], ids=["vanilla", "accelerated"])
@pytest.mark.parametrize("shards,eps", PSO_LAYOUTS, ids=["one-eps0", "one-eps", "four-eps"])
@pytest.mark.parametrize("objective", sorted(OBJECTIVES))
def test_pso_head_follows_the_reference(mod, objective, shards, eps, ptype, m):
    """`m` particles per shard (n = shards * m, so every shard has the ragged size). Three turns.
    Before each, the downloaded positions give f; RefPSOHead takes the turn on them: the
    downloaded pbest values, then (after the device's turn) gbest index, value and position,
    val_no_change, done and, where eps > 0, std_err(pbest) must be the reference's."""
    import torch
    body, f = OBJECTIVES[objective]
    obj = mod.CustomObjective(body, vector=True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = m * shards
    L = L_UNSHARDED if shards == 1 else L_sharded(shards)
    kw = dict(type=ptype, eps=eps, max_iter=5000, best_val_no_change=2, stream=stream)
    engs = [mod.PSOEngine(obj, n, 2, shard_lo=r * m, shard_n=m, **kw) for r in range(shards)]
    rec = engs[0].record_doubles()
    gathered = torch.zeros(shards * rec, dtype=torch.float64, device=dev)
    ref = R.RefPSOHead(n, max_iter=5000, best_val_no_change=2, eps=eps)
    for e in engs:
        e.init(-1.0, 1.0)
    best_pos, updates = None, 0  # swarm_best_position = positions[best] at the last update, :2736
    for turn in range(3):
        parts = [e.download() for e in engs]
        pos = np.concatenate([p[0] for p in parts])
        pbest = np.concatenate([p[2] for p in parts])
        cur = np.concatenate([p[3] for p in parts])
        vals = f(pos)
        assert same_array(cur, vals), f"turn {turn}: the device's f differs from numpy's"
        was_done, old_best = ref.done, ref.swarm_best_value
        ref.turn(vals)
        if not was_done:
            assert same_array(pbest, np.array(ref.particle_best_values)), f"turn {turn}: pbest"
            if ref.swarm_best_value < old_best:
                best_pos = pos[ref.swarm_best_index].copy()
                updates += 1
        if shards == 1:
            engs[0].step(1)
        else:
            for r, e in enumerate(engs):
                e.turn_begin(gathered[r * rec:(r + 1) * rec].data_ptr())
            for e in engs:
                e.turn_end(gathered.data_ptr(), shards)
        for r, e in enumerate(engs):
            st = e.status()
            bx, bf, bi = e.best()
            tag = f"turn {turn} shard {r}"
            assert (st.val_no_change, bool(st.done), st.iteration) == \
                (ref.val_no_change, ref.done, ref.iter), tag
            assert R.same_double(st.f_value, ref.swarm_best_value), tag
            assert R.same_double(bf, ref.swarm_best_value), tag
            if best_pos is not None:
                assert st.best_index == bi == ref.swarm_best_index, tag
                assert same_array(bx, best_pos), f"{tag}: best position {bx} != {best_pos}"
            if eps > 0 and not was_done:
                pb = np.array(ref.particle_best_values)
                ok, _, text = R.judge_std_err(st.std_err, pb, L)
                assert ok, f"{tag}: std_err {text}"
    assert updates >= 1  # the swarm best was copied at least once
    for e in engs:
        e.close()


@pytest.mark.parametrize("objective", sorted(OBJECTIVES))
@pytest.mark.parametrize("strategy", [1, 0], ids=["random", "best"])
def test_de_acceptance_on_hostile_objectives(mod, objective, strategy):
    """Five DE turns: the scores are f of the rows beside them, exactly, and `score < old` never
    lets a NaN replace a finite score; the head follows RefDEHead on the downloaded scores."""
    body, f = OBJECTIVES[objective]
    obj = mod.CustomObjective(body, vector=True)
    n = 1025
    ref = R.RefDEHead(max_iter=1000, best_val_no_change=10 ** 6)
    with mod.DEEngine(obj, n, 2, strategy=strategy, eps=0.0, max_iter=1000,
                      best_val_no_change=10 ** 6) as eng:
        eng.init(np.array([2.0, 2.0]))
        P, S = eng.download()
        assert same_array(S, f(P))
        assert objective == "ties" or (~np.isfinite(S)).sum() > n // 8  # the hostile branch is taken
        for turn in range(5):
            ref.turn(S)
            eng.step(1)
            st = eng.status()
            bx, bf, bi = eng.best()
            assert (st.best_index, st.val_no_change, st.iteration) == \
                (ref.best_id, ref.val_no_change, ref.iter), turn
            assert bi == ref.best_id and R.same_double(bf, ref.f_value) and same_array(bx, P[bi])
            P2, S2 = eng.download()
            assert same_array(S2, f(P2)), f"turn {turn}: scores are not f(population)"
            kept = np.isfinite(S)
            assert np.all(np.isfinite(S2[kept]) & (S2[kept] <= S[kept])), f"turn {turn}"
            assert np.all((S2 < S) | same_rows(P2, P)), f"turn {turn}: a row moved without a better score"
            P, S = P2, S2


def same_rows(a, b):
    return np.all((a == b) | (np.isnan(a) & np.isnan(b)), axis=1)
