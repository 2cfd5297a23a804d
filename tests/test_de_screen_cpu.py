"""The DE generation's half-row reject screen (kDeBoundScreen) without a device: the host's gate and
its two environment switches, the back-off rule on the selector byte as a pure function, and the
screen rule restated in numpy with the kernel's tree order (tests/_de_screen.py) run on the oracle's
synchronous DE runs: on every agent and generation, screen-decided implies bound-decided implies
rejected. The case list of tests/test_de_screen_gpu.py is checked here to reach every path."""
import ctypes as C

import numpy as np
import pytest

from tests import _oracle as O
from tests import _de_screen as M
from tests._de_bound import BoundModel, lane_tree
from tests.test_de_bound_cpu import hostile_rows


def test_host_gate():
    from nlsolver_amd import _capi
    gate, bound_gate = _capi.require("nlsg_de_screen_gate"), _capi.require("nlsg_de_bound_gate")
    ROS, SPH, ST, RAS = (_capi.OBJECTIVES[k] for k in ("rosenbrock", "sphere", "styblinski_tang", "rastrigin"))
    RANDOM, BEST = _capi.DE_RANDOM, _capi.DE_BEST
    # one chunk past its half: 65 <= D <= 128
    assert [gate(ROS, RANDOM, 1, 0.9, D) for D in (64, 65, 128, 129)] == [0, 1, 1, 0]
    assert [bound_gate(ROS, RANDOM, 1, 0.9, D) for D in (64, 65, 128, 129)] == [0, 1, 1, 1]
    # the bound's crossover window
    assert [gate(ROS, RANDOM, 1, cr, 128) for cr in (0.79, 0.8, 0.9, 1.0, 1.5)] == [0, 1, 1, 0, 0]
    assert gate(ROS, RANDOM, 1, float("nan"), 128) == 0
    assert gate(SPH, RANDOM, 1, 0.9, 128) == 1
    assert gate(ROS, BEST, 1, 0.9, 128) == 0     # strategy best
    assert gate(ROS, RANDOM, 0, 0.9, 128) == 0   # maximising
    for obj in (ST, RAS, _capi.OBJ_CUSTOM):      # terms that can be negative, user objectives
        assert gate(obj, RANDOM, 1, 0.9, 128) == 0
    # never wider than the bound's gate
    for D in (1, 64, 65, 100, 128, 129, 1024, 1025):
        for cr in (0.5, 0.8, 0.99, 1.0):
            assert gate(ROS, RANDOM, 1, cr, D) <= bound_gate(ROS, RANDOM, 1, cr, D)


def test_environment_switches(monkeypatch):
    from nlsolver_amd import _capi
    env = _capi.require("nlsg_de_screen_env")

    def read():
        on, r = C.c_int32(), C.c_uint32()
        assert env(C.byref(on), C.byref(r)) == 0
        return on.value, r.value

    monkeypatch.delenv("NLSG_DE_SCREEN", raising=False)
    monkeypatch.delenv("NLSG_DE_SCREEN_RETRY", raising=False)
    assert read() == (1, M.SCREEN_RETRY)
    monkeypatch.setenv("NLSG_DE_SCREEN", "0")
    assert read() == (0, M.SCREEN_RETRY)
    monkeypatch.setenv("NLSG_DE_SCREEN", "1")
    for text, want in (("16", 16), ("1", 1), ("256", 256), ("1073741824", 2**30), ("48", M.SCREEN_RETRY),
                       ("0", M.SCREEN_RETRY), ("-4", M.SCREEN_RETRY), ("2147483648", M.SCREEN_RETRY),
                       ("x", M.SCREEN_RETRY)):
        monkeypatch.setenv("NLSG_DE_SCREEN_RETRY", text)
        assert read() == (1, want), text


def test_back_off_rule_is_the_models():
    """nlsg_de_screen_rule (the host's copy of the kernel's rule) against the numpy one, on every
    selector byte, and the count as a state machine"""
    from nlsolver_amd import _capi
    rule = _capi.require("nlsg_de_screen_rule")
    after = C.c_uint32()
    for sel in range(16):
        for g in (1, 2, 7, 8, 63, 64, 255, 256, 2**32 - 3, 2**32 + 5):
            for a in (0, 1, 5, 63, 250):
                for br, sr in ((256, 64), (1, 1), (4, 16), (16, 4)):
                    bt, stry = M.tries_screen(np.int64(sel), g, a, br, sr)
                    for outcome in (0, 1, 2):
                        got = rule(sel, g, a, br, sr, outcome, C.byref(after))
                        assert got == int(stry), (sel, g, a, br, sr)
                        assert after.value == int(M.count_after(np.int64(sel >> 2 & 3), np.int64(outcome)))
    # the state machine: two misses in a row park the agent, a decision frees it
    cnt, seq = 0, []
    for outcome in (1, 0, 1, 1, 1, 1, 2, 0, 2):
        cnt = int(M.count_after(np.int64(cnt), np.int64(outcome)))
        seq.append(cnt)
    assert seq == [1, 0, 1, 2, 3, 3, 3, 0, 0]
    # hint clear: tries while the count is below 2, then only in its retry generations
    for cnt in range(4):
        tried = [g for g in range(1, 33) if M.tries_screen(np.int64(cnt << 2), g, 3, 256, 8)[1]]
        assert tried == (list(range(1, 33)) if cnt < 2 else [5, 13, 21, 29])
    # a hinted agent tries only where the bound would: both periods must agree
    tried = [g for g in range(1, 65) if M.tries_screen(np.int64(2 | 3 << 2), g, 0, 16, 8)[1]]
    assert tried == [16, 32, 48, 64]
    tried = [g for g in range(1, 65) if M.tries_screen(np.int64(2), g, 0, 16, 8)[1]]
    assert tried == [16, 32, 48, 64]


@pytest.mark.parametrize("obj", ["rosenbrock", "sphere"])
@pytest.mark.parametrize("D", [65, 66, 127, 128])
def test_screen_value_is_below_the_bound(obj, D):
    """screen <= bound <= full bit for bit (or NaN, which decides nothing) over hostile rows"""
    rng = np.random.default_rng(7 + D)
    n = 400
    rows = hostile_rows(rng, n, D)
    known = rng.random((n, D)) < rng.choice([0.0, 0.5, 0.9, 0.99, 1.0], size=(n, 1))
    full = lane_tree(obj, rows)
    other = np.where(known, rows, hostile_rows(rng, n, D))
    bound = lane_tree(obj, other, known)
    screen = M.screen_value(obj, other, known)
    with np.errstate(invalid="ignore"):
        assert not np.any(bound < screen) and not np.any(full < screen)
        assert np.isnan(screen).any() and (~np.isnan(screen)).any()
        for old in (-np.inf, 0.0, 1.0, 1e300, np.inf, np.nan):
            dec = screen >= old
            assert not np.any(dec & (full < old))
            assert not np.any(dec & ~(bound >= old) & ~np.isnan(bound))
    # nothing known below 64: the screen value is +0.0
    none = ~known[:, :64].any(axis=1)
    assert np.array_equal(screen[none].view(np.uint64), np.zeros(int(none.sum()), dtype=np.uint64))


def test_screen_value_is_the_half_waves_tree():
    """the kernel's order spelled out: 32 lanes, terms 2j and 2j + 1, levels 16 .. 1"""
    rng = np.random.default_rng(3)
    D, n = 128, 50
    x = rng.uniform(-2.048, 2.048, size=(n, D))
    known = rng.random((n, D)) < 0.9
    want = M.screen_value("rosenbrock", x, known)
    j = np.arange(32)
    term = lambda xi, xn: (1 - xi) * (1 - xi) + (100 * (xn - xi * xi)) * (xn - xi * xi)
    t0 = np.where(known[:, 2 * j] & known[:, 2 * j + 1], term(x[:, 2 * j], x[:, 2 * j + 1]), 0.0)
    t1 = np.where(known[:, 2 * j + 1] & known[:, 2 * j + 2] & (j != 31)[None, :],
                  term(x[:, 2 * j + 1], x[:, 2 * j + 2]), 0.0)
    acc = (0.0 + t0) + t1
    for off in (16, 8, 4, 2, 1):
        acc = acc + acc[:, j ^ off]
    assert np.array_equal(acc[:, 0].view(np.uint64), want.view(np.uint64))


@pytest.fixture(scope="module")
def models(oracle):
    return [M.run_model(O, oracle, c) for c in M.CASES]


def test_chain_holds_on_the_oracles_runs(oracle, models):
    """ScreenModel.generation asserts the chain on every agent and generation; here the bound's side
    of it against tests/_de_bound.py, and the counters' arithmetic"""
    for c, (model, _) in zip(M.CASES, models):
        obj, pop, D, CR, F, x0v, gens, seed, sr = c
        ref = O.DESyncRun(oracle, obj, pop, D, np.full(D, x0v), trace=True, **M.case_kw(c))
        bm = BoundModel(obj, pop, D, CR, F, seed, M.BOUND_RETRY)
        for g in range(1, gens + 1):
            P, S = ref.population.copy(), ref.scores.copy()
            ref.step(1)
            bm.generation(g, P, S, ref.trace)
        assert model.bound_counts == bm.counts, M.case_id(c)
        assert model.screen_counts[0] <= model.bound_counts[0]
        assert model.screen_counts[0] == model.seen[M.DECIDED]
        assert model.screen_counts[1] == model.seen[M.MISS_BOUND] + model.seen[M.MISS_ACCEPT] + model.seen[M.MISS_REJECT]


def test_case_list_reaches_every_path(models):
    seen = sum(m.seen for m, _ in models)
    retried = sum(r for _, r in models)
    for k in (M.DECIDED, M.MISS_BOUND, M.MISS_ACCEPT, M.MISS_REJECT, M.FEW_DONORS, M.PAST_SIX, M.BACKED_OFF):
        assert seen[k] >= 3, (M.NAMES[k], int(seen[k]))
    assert retried >= 3
