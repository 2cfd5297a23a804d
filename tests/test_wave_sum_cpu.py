"""The numpy restatement of the wave sum (tests/_wave_sum.py), which tests/test_wave_sum_gpu.py pins
the device to, against the exactly rounded sum: so that the reference is checked by something other
than the code it is a reference for.

Error bound: the butterfly is a balanced tree of depth 6, every term passes through six round-to-
nearest additions (relative error <= u = 2^-53 each, none in the subnormal range, where addition is
exact), so |tree - sum| <= ((1 + u)^6 - 1) * sum |x_i|; math.fsum gives the exact sum rounded once
(u * |sum| more)."""
import math

import numpy as np

from tests import _wave_sum as W

U = 2.0 ** -53


def check(v):
    t = W.butterfly(v)
    assert (t.view(np.uint64) == t[:, :1].view(np.uint64)).all(), "lanes of a wave differ"
    for row, got in zip(v, t[:, 0]):
        exact = math.fsum(row)
        mag = math.fsum(abs(x) for x in row)
        bound = 6.0000001 * U * mag + U * abs(exact)  # (1 + u)^6 - 1 = 6 u + 15 u^2 + ...
        assert abs(got - exact) <= bound, (got, exact, bound)


def test_restatement_against_fsum_normals():
    check(W.normals(np.random.default_rng(1), 512))


def test_restatement_against_fsum_wide_and_cancelling():
    check(W.wide(np.random.default_rng(2), 512))


def test_restatement_specials():
    rng = np.random.default_rng(3)
    v = W.specials(rng, 512)
    t = W.butterfly(v)
    fin = np.isfinite(v).all(axis=1)
    check(v[fin])
    # the all -0 wave sums to -0, the all +0 one to +0, mixed zeros to +0 (round to nearest)
    assert np.signbit(t[512 // 8]).all() and (t[512 // 8] == 0).all()
    assert not np.signbit(t[512 // 8 + 1]).any()
    # one sign of infinity per wave: that infinity in every lane
    inf = ~fin
    assert inf.sum() >= 200
    want = np.where(np.isposinf(v[inf]).any(axis=1), np.inf, -np.inf)
    assert (t[inf] == want[:, None]).all()


def test_restatement_nan_reaches_every_lane():
    t = W.butterfly(W.one_nan(np.random.default_rng(4), 256))
    assert np.isnan(t).all()


def test_restatement_order_is_own_first_xor_levels():
    # integers small enough for exact sums: the butterfly is the plain total, and one level is v[l] + v[l ^ off]
    v = np.arange(64, dtype=np.float64)[None, :] * 3.0 + 1.0
    assert (W.butterfly(v) == v.sum()).all()
    assert W.all_inputs(waves_each=4).shape == (16, 64)
