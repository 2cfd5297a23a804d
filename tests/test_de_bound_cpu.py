"""The DE generation rejects a trial on the terms that involve mutant coordinates alone
(DeParams.bound). The argument rests on the lane tree: with +0.0 in place of every term that reads
a kept coordinate, summed in the same per-lane order and the same butterfly, the masked value is a
lower bound of the full value bit for bit. Here the tree is restated in numpy (tests/_de_bound.py),
pinned to the oracle's, and the bound property is checked over hostile rows; the host's gate is
checked as a plain function."""
import numpy as np
import pytest

from tests import _oracle as O
from tests._de_bound import BoundModel, cross_masks, ctr_key, lane_tree, mix64, u01

OBJS = ("rosenbrock", "sphere")


def orc_tree(oracle, obj, row):
    row = np.ascontiguousarray(row, dtype=np.float64)
    return oracle.orc_objective_tree(O.OBJ[obj], row.ctypes.data_as(O.pd), row.size)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_keyed_draws_equal_the_oracles(oracle):
    rng = np.random.default_rng(1)
    z = rng.integers(0, 2**63, size=64, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for v in list(z) + [np.uint64(0), np.uint64(2**64 - 1)]:
        assert int(mix64(v)) == oracle.orc_mix64(int(v))
        assert int(ctr_key(v, np.uint64(7))) == oracle.orc_ctr_key(int(v), 7)
        assert float(u01(v)) == oracle.orc_u01(int(v))


@pytest.mark.parametrize("obj", OBJS)
@pytest.mark.parametrize("D", [66, 128, 129, 1000])
def test_full_mask_equals_the_oracle_tree_bit_for_bit(oracle, obj, D):
    rng = np.random.default_rng(D)
    rows = np.concatenate([rng.uniform(-2.048, 2.048, size=(6, D)),
                           rng.standard_normal((3, D)) * 1e3,
                           np.full((1, D), 1.0), np.zeros((1, D))])
    rows[8, D // 2] = np.inf
    rows[7, 1] = np.nan
    got = lane_tree(obj, rows)
    got_all_known = lane_tree(obj, rows, np.ones(rows.shape, dtype=bool))
    for i, row in enumerate(rows):
        want = orc_tree(oracle, obj, row)
        assert bits(got[i]) == bits(want) or (np.isnan(got[i]) and np.isnan(want)), (obj, D, i)
    # adding +0.0 where nothing is masked changes no bit
    assert np.array_equal(bits(got), bits(got_all_known))


def hostile_rows(rng, n, D):
    rows = rng.uniform(-2.048, 2.048, size=(n, D))
    kind = rng.integers(0, 6, size=(n, D))
    pick = rng.random((n, D)) < 0.08
    rows = np.where(pick & (kind == 0), rng.standard_normal((n, D)) * 1e150, rows)   # squares overflow
    rows = np.where(pick & (kind == 1), rng.standard_normal((n, D)) * 5e-324 * 1e3, rows)  # denormal
    rows = np.where(pick & (kind == 2), np.inf, rows)
    rows = np.where(pick & (kind == 3), -np.inf, rows)
    rows = np.where(pick & (kind == 4) & (rng.random((n, D)) < 0.3), np.nan, rows)
    rows = np.where(pick & (kind == 5), rng.standard_normal((n, D)) * 1e60, rows)
    rows[: n // 4] = rng.uniform(-2.048, 2.048, size=(n // 4, D))  # a quarter stays tame
    return rows


@pytest.mark.parametrize("obj", OBJS)
@pytest.mark.parametrize("D", [66, 128, 129, 300, 1000])
def test_masked_value_is_a_lower_bound(obj, D):
    """bound >= old must imply !(full < old) for every old: the masked value is NaN (never '>=')
    or not above the full value (or the full value is NaN: rejected either way)."""
    rng = np.random.default_rng(100 + D)
    n = 400 if D <= 300 else 120
    rows = hostile_rows(rng, n, D)
    cr = rng.choice([0.0, 0.2, 0.5, 0.9, 0.99, 1.0], size=(n, 1))
    known = rng.random((n, D)) < cr
    full = lane_tree(obj, rows)
    # the unknown coordinates hold something else in the mutant the bound is taken from
    other = np.where(known, rows, hostile_rows(rng, n, D))
    bound = lane_tree(obj, other, known)
    with np.errstate(invalid="ignore"):
        assert not np.any(full < bound), (obj, D)
        nan_b = np.isnan(bound)
        assert nan_b.any() and (~nan_b).any()
        for old in (-np.inf, -1.0, 0.0, 1e300, np.inf, np.nan):
            assert not np.any(bound[nan_b] >= old)           # a NaN bound decides nothing
            decided = bound >= old
            assert not np.any(decided & (full < old))
        # a NaN score is rejected by the bound as well: NaN >= x is false
        assert not np.any(np.full(3, 1.0) >= np.nan)
    all_known = known.all(axis=1)
    assert np.array_equal(bits(bound[all_known]), bits(full[all_known]))
    none_known = ~known.any(axis=1)
    assert np.array_equal(bits(bound[none_known]), bits(np.zeros(int(none_known.sum()))))


def test_model_reproduces_the_oracles_accept_flags(oracle):
    """The crossover masks recomputed from the keys rebuild the oracle's trials: rows and accept
    flags agree, and the bound never rejects what the oracle accepted (BoundModel asserts it)."""
    pop, D, CR, F, seed = 96, 128, 0.9, 0.3, 12374563468
    ref = O.DESyncRun(oracle, "rosenbrock", pop, D, np.full(D, 1.2), CR=CR, F=F, eps=0.0,
                      best_val_no_change=10**6, trace=True)
    model = BoundModel("rosenbrock", pop, D, CR, F, seed, retry=1)
    for g in range(1, 6):
        P, S = ref.population.copy(), ref.scores.copy()
        ref.step(1)
        T = ref.trace
        cross = cross_masks(seed, g, np.arange(pop), D, CR, T[:, 3])
        r = T[:, :3].astype(np.int64)
        trial = np.where(cross, P[r[:, 0]] + F * (P[r[:, 1]] - P[r[:, 2]]), P)
        score = lane_tree("rosenbrock", trial)
        accept = score < S
        assert np.array_equal(accept, T[:, 4] != 0)
        assert np.array_equal(ref.population, np.where(accept[:, None], trial, P))
        assert np.array_equal(ref.scores, np.where(accept, score, S))
        model.generation(g, P, S, T)
    assert sum(model.counts) == 5 * pop and min(model.counts) > 0


def test_host_gate():
    from nlsolver_amd import _capi
    gate = _capi.require("nlsg_de_bound_gate")
    ROS, SPH, ST, RAS = (_capi.OBJECTIVES[k] for k in ("rosenbrock", "sphere", "styblinski_tang", "rastrigin"))
    RANDOM, BEST = _capi.DE_RANDOM, _capi.DE_BEST
    assert gate(ROS, RANDOM, 1, 0.9, 128) == 1
    assert gate(SPH, RANDOM, 1, 0.9, 128) == 1
    assert gate(ROS, RANDOM, 1, 0.95, 65) == 1 and gate(ROS, RANDOM, 1, 0.99, 1024) == 1
    # from CR 1 up no coordinate is kept and the plain path reads no own row either
    assert gate(ROS, RANDOM, 1, 1.0, 128) == 0 and gate(ROS, RANDOM, 1, 1.5, 128) == 0
    # objectives whose terms can be negative, and user objectives
    for obj in (ST, RAS, _capi.OBJ_CUSTOM):
        assert gate(obj, RANDOM, 1, 0.9, 128) == 0
    assert gate(ROS, BEST, 1, 0.9, 128) == 0      # the kept coordinates are the best row's
    assert gate(ROS, RANDOM, 0, 0.9, 128) == 0    # maximising: fmul = -1
    assert gate(ROS, RANDOM, 1, 0.9, 64) == 0     # the packed kernel
    assert gate(ROS, RANDOM, 1, 0.9, 1025) == 0   # the segment kernel
    for cr in (0.0, 0.2, 0.5, float("nan"), -1.0):  # too few known terms to decide
        assert gate(ROS, RANDOM, 1, cr, 128) == 0
    # the threshold itself: on at and above it, off below
    grid = [k / 100 for k in range(0, 100)]
    on = [cr for cr in grid if gate(ROS, RANDOM, 1, cr, 128)]
    assert on and on[-1] == 0.99 and on == [cr for cr in grid if cr >= on[0]]
    assert _capi.lib().nlsg_abi_version() == 1
