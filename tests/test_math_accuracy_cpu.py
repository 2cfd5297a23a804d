"""The oracle's copies of nlsg_math.h's deterministic primitives (oracle_math.c, oracle_lm.c) against
256-bit references (tests/golden/math_ref.npz), with the bound each primitive claims.

test_math_gpu.py holds the device bit-equal to these copies; this file checks that the algorithm
both copies share is right — a changed coefficient, a dropped reduction term or a wrong threshold
passes a copy-against-copy comparison, not this one."""
import importlib.util
import os

import numpy as np
import pytest

from tests import _math_ref as M
from tests import _oracle as O


@pytest.fixture(scope="module")
def ref():
    return M.load()


@pytest.fixture(scope="module")
def probe(oracle):
    return lambda fn, bits: O.probe_math(oracle, fn, bits)


def test_fixture_size():
    assert os.path.getsize(M.FIXTURE) <= 512 * 1024


@pytest.mark.parametrize("name", M.ACCURACY)
def test_accuracy(ref, probe, name):
    M.check(name, ref, probe)


def test_special_values(probe):
    M.check_specials(probe)


def test_rnorm_special_draws(probe):
    z = np.array(M.RNORM_SPECIAL_DRAWS, dtype=np.uint64)
    got = M.f64(probe("rnorm", z))
    want = np.array([M.rnorm_special_expected(v) for v in M.RNORM_SPECIAL_DRAWS])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)


def test_exp_thresholds(probe):
    """+inf exactly from the first double above fdlibm's overflow threshold on, finite at it; 0
    exactly below the underflow threshold, the smallest subnormal at it"""
    o, u = M.O_THRESHOLD, M.U_THRESHOLD
    x = np.array([o, np.nextafter(o, np.inf), u, np.nextafter(u, -np.inf)])
    y = M.f64(probe("exp", x.view(np.uint64)))
    assert np.isfinite(y[0]) and y[0] > 1.79e308
    assert y[1] == np.inf
    assert y[2] == 5e-324
    assert y[3].view(np.uint64) == 0


def test_symmetries(ref, probe):
    """tanh is odd and cos even, bit for bit — except, for cos, within a few ulps of the quadrant
    switch points |y| = (n + 1/2) pi/2: there floor(y 2/pi + 1/2) may put y and -y into quadrants
    that are not mirror images (r ~ +pi/4 against -pi/4: the cosine kernel against the sine
    kernel), and the two results may differ by 1 ulp"""
    rng = np.random.default_rng(5)
    y = np.concatenate([M.f64(ref["cos_x"]), rng.uniform(-64.0, 64.0, 1_000_000)])
    cp, cm = probe("cos", y.view(np.uint64)), probe("cos", (-y).view(np.uint64))
    a = np.abs(y) * 6.36619772367581382433e-01
    switch = np.abs(a - np.floor(a) - 0.5) < 2.0**-40
    assert np.array_equal(cp[~switch], cm[~switch])
    assert (np.abs(cp[switch].astype(np.int64) - cm[switch].astype(np.int64)) <= 1).all()
    x = M.f64(ref["tanh_x"])
    assert np.array_equal(probe("tanh", (-x).view(np.uint64)),
                          (-M.f64(probe("tanh", x.view(np.uint64)))).view(np.uint64))


def _runs(centres, n):
    """n consecutive doubles from each centre on"""
    c = np.asarray(centres, dtype=np.float64).view(np.int64)
    return (c[:, None] + np.arange(-n, n, dtype=np.int64)[None, :]).ravel().view(np.float64)


@pytest.mark.parametrize("fn,lo,hi,centres", [
    ("log", 2.0**-60, 2.0**60, [1.0, 0.7071067811865476, 1.4142135623730951, 0.5, 2.0]),
    ("exp", M.U_THRESHOLD, M.O_THRESHOLD,
     [0.0, 0.34657359027997264, -0.34657359027997264, -708.0, -708.3964185322641, 709.0,
      709.4361393031039]),
    ("tanh", -25.0, 25.0, [0.0, 0.17328679513998632, 0.34657359027997264, 0.5198603854199589,
                           -0.17328679513998632, 3.19, 14.93, 22.0, -22.0]),
])
def test_monotone(probe, fn, lo, hi, centres):
    """non-decreasing on a sorted dense grid: random points plus runs of consecutive doubles across
    the reduction's switching points. log and exp strictly; tanh, whose error exceeds half an ulp,
    is not monotone from one double to the next: two neighbours' results, each within 2.5 ulp of
    nearly the same exact value, may step back by up to 5 ulps"""
    rng = np.random.default_rng(7)
    if fn == "log":
        x = np.exp2(rng.uniform(np.log2(lo), np.log2(hi), 1_000_000))
    else:
        x = rng.uniform(lo, hi, 1_000_000)
    x = np.sort(np.concatenate([x, _runs(centres, 2000)]))
    y = M.f64(probe(fn, x.view(np.uint64)))
    slack = 5 * np.spacing(np.abs(y[:-1])) if fn == "tanh" else 0.0
    bad = np.flatnonzero(np.diff(y) < -slack)
    assert bad.size == 0, (fn, x[bad[:5]], y[bad[:5]], y[bad[:5] + 1])


def test_generator_reproduces_fixture(ref):
    """if mpmath is here: the generator's argument sets equal the fixture's, and a seeded sample of
    200 references recomputes to the same (hi, lo)"""
    pytest.importorskip("mpmath")
    path = os.path.join(M.ROOT, "tests", "golden", "gen_math_ref.py")
    spec = importlib.util.spec_from_file_location("gen_math_ref", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    args = gen.arguments()
    for name, xs in args.items():
        assert np.array_equal(xs, M.arguments(ref, name)), name
    rng = np.random.default_rng(11)
    names = list(args)
    for _ in range(200):
        name = names[rng.integers(len(names))]
        i = int(rng.integers(ref[name + "_hi"].size))
        hi, lo = gen.to_dd(gen.exact(name, M.arguments(ref, name)[i]))
        assert (hi, lo) == (ref[name + "_hi"][i], ref[name + "_lo"][i]), (name, i)
