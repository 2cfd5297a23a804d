"""The head of a DE turn in oracle/oracle_de.c (best scan with the incumbent and tie rules,
val_no_change, std_err, the three stop tests) against the independent references of
tests/_head_ref.py, on hostile scores: ties, NaN / inf, ill-conditioned samples. No GPU.

The device kernels are pinned bit for bit to this C restatement elsewhere; this file pins the
restatement itself to the reference's rules (nlsolver.h:2428-2447, :2037-2052), so that the two
cannot be wrong together. tests/test_head_rules_gpu.py runs the same vectors on the device.

std_err: the one-pass tile-merged form (orc_tiled_m2_merged) is held to the a-priori bound
    |got - exact| / exact <= L u (2 + 2 kappa) + (L u kappa)^2,   u = 2^-53, L = 32
(L: see tests/_head_common.py). Worst measured error as a fraction of the bound's linear term,
over the sizes 4 ... 263169 below (test_tiled_m2_accuracy prints them):
    conditioning/normal_0_1         0.0153   (kappa ~ 1)
    conditioning/normal_50_10       0.0041   (kappa ~ 5)
    conditioning/normal_10000_0.01  2.3e-05  (kappa ~ 1e6)
    conditioning/normal_-1e+08_1    4.3e-05  (kappa ~ 1e8)
    conditioning/outlier_1e12       0.0086   (kappa ~ 1)
    conditioning/denormals          squared deviations underflow: 0.0 against ~1e-312, inside
                                    the absolute underflow term 2^-536
    ties/* (two or three values)    at most 0.0113
"""
import math

import numpy as np
import pytest

from tests import _head_ref as R
from tests import _oracle as O
from tests._head_common import (L_UNSHARDED, SHARD_SIZES, SIZES, WORLDS, L_sharded, make_run,
                                 oracle_head, oracle_turns)

def ref_turns(vectors, **kw):
    h = R.RefDEHead(**kw)
    for v in vectors:
        h.turn(v)
    return h.best_id, h.val_no_change, h.iter, h.done


def check_rules(lib, n, shards):
    run = make_run(lib, n, shards)
    L = L_UNSHARDED if shards == 1 else L_sharded(shards)
    bad = []
    for c in R.cases(n, shards):
        got = oracle_turns(run, [c.place, c.vec], eps=R.EPS_TINY)
        if got[:4] != c.want:
            bad.append(f"{c.name} inc {c.inc}: (best, vnc, iter, done) {got[:4]} != reference {c.want}")
        if not R.same_double(got[5], c.f_value):  # the finaliser's own best value
            bad.append(f"{c.name} inc {c.inc}: f_value {got[5]!r} != {c.f_value!r}")
        if c.judge:
            ok, _, text = R.judge_std_err(got[4], c.vec, L)
            if not ok:
                bad.append(f"{c.name} inc {c.inc}: std_err {text}")
    assert not bad, f"n {n} shards {shards}: {len(bad)} mismatches\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("n", SIZES)
def test_unsharded_head_follows_the_reference(oracle, n):
    check_rules(oracle, n, 1)


@pytest.mark.parametrize("m", SHARD_SIZES)
@pytest.mark.parametrize("world", WORLDS)
def test_sharded_head_decides_as_one_scan(oracle, world, m):
    """N shards decide as one scan of the global vector would, NaN incumbents in a later rank
    included (the finaliser must not let an earlier rank's finite record displace it)."""
    check_rules(oracle, world * m, world)


@pytest.mark.parametrize("world", [1, 2, 4])
def test_oracle_head_is_sync_steps_head(oracle, world):
    """oracle_head (tests/_head_common.py) against orc_de_sync_step itself, turn by turn on
    fuzzed scores: same best_id, counters, stop flag and std_err."""
    n = 8 * world
    kw = dict(n_shards=world, eps=R.EPS_TINY, max_iter=40, best_val_no_change=10 ** 6)
    a = O.DESyncRun(oracle, "sphere", n, 2, np.ones(2), **kw)
    b = O.DESyncRun(oracle, "sphere", n, 2, np.ones(2), **kw)
    rng = np.random.default_rng(17 + world)
    for t in range(45):  # runs into max_iter
        v = R.fuzz_vector(n, rng) if t % 3 else rng.normal(0.0, 1.0, n)
        a.scores[:] = v
        b.scores[:] = v
        a.step(1)
        oracle_head(b)
        assert (a.s.best_id, a.s.val_no_change, a.s.iter, a.s.done) == \
            (b.s.best_id, b.s.val_no_change, b.s.iter, b.s.done), t
        assert R.same_double(a.s.std_err, b.s.std_err), t
    assert a.s.done and a.s.iter == 40


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_fuzzed_turns(oracle, world):
    """1500 consecutive turns on vectors drawn from {NaN, -inf, -0.0, 0.0, 1, +inf}: the state
    carries over, so the incumbent's score is whatever the next vector puts there."""
    n = 8 * world
    run = make_run(oracle, n, world)
    s = run.s
    s.best_id, s.iter, s.val_no_change, s.done = 0, 0, 0, 0
    s.max_iter = 10 ** 6
    ref = R.RefDEHead(max_iter=10 ** 6, best_val_no_change=10 ** 6)
    rng = np.random.default_rng(world)
    bad = nan_inc = 0
    for t in range(1500):
        v = R.fuzz_vector(n, rng)
        nan_inc += bool(np.isnan(v[ref.best_id]))
        run.scores[:] = v
        oracle_head(run)
        ref.turn(v)
        if (int(s.best_id), int(s.val_no_change), int(s.iter)) != (ref.best_id, ref.val_no_change, ref.iter):
            bad += 1
            s.best_id, s.val_no_change = ref.best_id, ref.val_no_change  # count turns, not a cascade
    assert nan_inc > 100  # the case is drawn often
    assert bad == 0, f"{bad} of 1500 turns differ ({nan_inc} with a NaN incumbent)"


@pytest.mark.parametrize("world,n", [(1, 5), (1, 257), (1, 2049), (2, 514), (4, 4100)])
def test_stop_tests_fire_and_hold(oracle, world, n):
    """val_no_change against best_val_no_change in {1, 2}; std_err against eps a factor of 2
    below and above the exact statistic."""
    run = make_run(oracle, n, world)
    inc = n // 2
    place = R.placement(n, inc)
    seen = set()
    for name, vec in R.families(n, inc, world, which=("ties", "conditioning")):
        for bvnc in (1, 2):
            got = oracle_turns(run, [place, vec], best_val_no_change=bvnc)
            want = ref_turns([place, vec], best_val_no_change=bvnc)
            assert got[:4] == want, (name, bvnc, got, want)
            seen.add(("vnc", want[3]))
        if not R.std_err_precondition(vec):
            continue
        exact, _ = R.exact_std_err(vec)
        if not exact > 1e-300:
            continue
        for eps, fires in ((exact / 2, False), (2 * exact, True)):
            far = R.placement(n, inc, scale=max(1.0, 4 * eps))  # the placing turn must not stop
            got = oracle_turns(run, [far, vec], eps=eps)
            want = ref_turns([far, vec], eps=eps)
            assert want[3] == fires and got[:4] == want, (name, eps, got, want)
            seen.add(("eps", fires))
    assert seen == {("vnc", True), ("vnc", False), ("eps", True), ("eps", False)}


def test_tiled_m2_accuracy(oracle):
    """orc_tiled_m2_merged against the exact statistic, inside the a-priori bound; prints the
    worst error per family as a fraction of the bound's linear term (module docstring)."""
    worst = {}
    for n in SIZES:
        for name, vec in R.families(n, n // 2, which=("ties", "conditioning")):
            if not R.std_err_precondition(vec):
                continue
            v = np.ascontiguousarray(vec)
            tot = O.C.c_double()
            m2 = oracle.orc_tiled_m2_merged(O._ptr(v), n, O.C.byref(tot))
            got = math.sqrt(m2 / (n - 1))
            ok, ratio, text = R.judge_std_err(got, vec, L_UNSHARDED)
            assert ok, f"{name} n {n}: {text}"
            if ratio is not None:
                worst[name] = max(worst.get(name, 0.0), ratio)
    for name in sorted(worst):
        print(f"{name:40s} worst err / linear term {worst[name]:.3g}")
    assert max(worst.values()) <= 1.0


def test_references_are_independent():
    """the references restate the rules on their own: no oracle, no package"""
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(R))
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add(node.module or "")
    assert not any("oracle" in m or "nlsolver" in m for m in mods), mods
    # and they agree with numpy's two-pass statistic where that is well conditioned
    x = np.random.default_rng(3).normal(50.0, 10.0, 999)
    exact, kappa = R.exact_std_err(x)
    assert abs(exact - np.std(x, ddof=1)) <= 1e-13 * exact and 4.5 < kappa < 6.0
    assert abs(R.literal_std_err(x) - exact) <= 1e-13 * exact
