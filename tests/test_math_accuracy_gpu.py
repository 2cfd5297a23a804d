"""The device's deterministic math primitives (nlsg_probe_math) against 256-bit references
(tests/golden/math_ref.npz) with the bound each primitive claims — directly, not through the oracle
— and against the oracle bit for bit on every fixture argument; the square root, the Givens
rotation's 1 / sqrt(r^2 + 1) and u01 against IEEE arithmetic (numpy / Python), bit for bit."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _math_ref as M
from tests import _oracle as O
from tests.test_math_gpu import draws

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available()
    from nlsolver_amd import _capi
    return lambda fn, bits: _capi.probe_math(fn, bits)


@pytest.fixture(scope="module")
def ref():
    return M.load()


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


def _fixture_doubles(ref):
    """every double argument of the fixture, and the specials"""
    xs = [ref[k] for k in ("log_x", "log_unit_x", "exp_x", "tanh_x", "cos_x", "cos_2pi_x")]
    sp = np.array([s[1] for s in M.SPECIALS] + [2.0**-767, 2.0**-64, 1.0, -1.0, 0.5])
    return M.f64(np.unique(np.concatenate(xs + [sp.view(np.uint64)])))


def _domain(fn, x):
    if fn == "log_unit":
        return x[(x >= 2.0**-64) & (x <= 1.0)]
    if fn == "givens_t":  # r = small / large: |r| <= 1, or NaN
        return x[~(np.abs(x) > 1.0)]
    if fn == "sqrt":
        return x[(x == 0.0) | (x >= 2.0**-767) | np.isnan(x)]
    return x


@pytest.mark.parametrize("fn", sorted(O.PROBE, key=O.PROBE.get))
def test_device_equals_oracle_on_fixture(ref, probe, oracle, fn):
    """device == oracle, bit for bit (NaN: any NaN), on every argument of the fixture"""
    if fn in ("u01", "rnorm", "rnorm_cos"):
        u = np.unique(np.concatenate([ref["rnorm_x"], ref["u01_x"],
                                      np.array(M.RNORM_SPECIAL_DRAWS, dtype=np.uint64)]))
        nan_ok = np.zeros(u.size, bool)
    else:
        x = _domain(fn, _fixture_doubles(ref))
        u = x.view(np.uint64)
        nan_ok = None
    dev, orc = probe(fn, u), O.probe_math(oracle, fn, u)
    if nan_ok is None:
        nan_ok = np.isnan(M.f64(dev)) & np.isnan(M.f64(orc))
    bad = np.flatnonzero((dev != orc) & ~nan_ok)
    assert bad.size == 0, (fn, u[bad[:5]], dev[bad[:5]], orc[bad[:5]])


def test_new_probes_bit_exact(probe, oracle):
    """the four probes added with the fixture, device against oracle on millions of arguments"""
    rng = np.random.default_rng(21)
    n = 1_000_000
    x = np.ldexp(1.0 + rng.random(n), rng.integers(-64, 0, n))  # [2^-64, 1)
    x[:2] = [2.0**-64, 1.0]
    z = draws(rng, n)
    r = 2 * rng.random(n) - 1
    s = np.ldexp(1.0 + rng.random(n), rng.integers(-767, 1024, n))
    for fn, u in (("log_unit", x.view(np.uint64)), ("rnorm_cos", z), ("givens_t", r.view(np.uint64)),
                  ("sqrt", s.view(np.uint64))):
        dev, orc = probe(fn, u), O.probe_math(oracle, fn, u)
        bad = np.flatnonzero(dev != orc)
        assert bad.size == 0, (fn, u[bad[:5]], dev[bad[:5]], orc[bad[:5]])


def test_rnorm_wave_uniform_special_path(probe, oracle):
    """det_rnorm takes its special-case path for the whole wave when one lane holds z = 0 or
    z >= 2^64 - 2^10: the other 63 lanes' bits must not depend on which path the wave took"""
    rng = np.random.default_rng(22)
    base = rng.integers(1, 2**63, size=64, dtype=np.uint64)  # no special draw among them
    plain = probe("rnorm", base)
    for lane in (0, 13, 63):
        for special in (0, 2**64 - 2**10, 2**64 - 1):
            z = base.copy()
            z[lane] = special
            got = probe("rnorm", z)
            keep = np.arange(64) != lane
            assert np.array_equal(got[keep], plain[keep]), (lane, special)
            assert got[lane] == np.float64(M.rnorm_special_expected(special)).view(np.uint64)
            assert np.array_equal(got, O.probe_math(oracle, "rnorm", z))
    # two waves: the special draw in the first must leave the second's path alone too
    z = np.concatenate([base, base])
    z[5] = 0
    got = probe("rnorm", z)
    assert np.array_equal(got[64:], plain)


def _midpoint_squares(rng, n, lo, hi):
    """doubles x close to the square of a rounding midpoint of [lo, hi): sqrt(x) is a hard case"""
    out = []
    for m in rng.uniform(lo, hi, n):
        mid = Fraction(m) + Fraction(float(np.spacing(m))) / 2
        out.append(float(mid * mid))
    return np.array(out)


def test_givens_t_bit_exact(probe):
    """1 / sqrt(r^2 + 1) as the kernels write it (div_unscaled / sqrt_unscaled, without the
    compiler's scaling and fix-up) equals the IEEE expression of the reference's
    inv_sqrt(std::pow(r, 2) + 1.0) bit for bit"""
    rng = np.random.default_rng(23)
    r = 2 * rng.random(1_000_000) - 1
    # hard cases: x = r^2 + 1 next to a rounding midpoint of the square root, and of the reciprocal
    xs = list(_midpoint_squares(rng, 2000, 1.0, np.sqrt(2.0)))
    for m in rng.uniform(np.sqrt(0.5), 1.0, 2000):
        mid = Fraction(m) + Fraction(float(np.spacing(m))) / 2  # 1 / s near a midpoint
        s = float(1 / mid)
        xs.append(float(Fraction(s) * Fraction(s)))
    hard = []
    for x in xs:
        x = min(max(x, 1.0), 2.0)
        r0 = np.sqrt(x - 1.0)
        for k in range(-2, 3):
            rr = np.float64(r0).view(np.int64) + k
            rr = np.int64(max(rr, 0)).view(np.float64)
            if rr <= 1.0 and rr * rr + 1.0 == x:
                hard += [rr, -rr]
    assert len(hard) > 1000
    special = [0.0, -0.0, 5e-324, -5e-324, 2.0**-1022, 1e-160, 1.5e-154, 2.0**-26, 2.0**-27, 1.0, -1.0,
               np.nextafter(1.0, 0.0), np.nan]
    r = np.concatenate([r, np.array(hard), np.array(special)])
    got = M.f64(probe("givens_t", r.view(np.uint64)))
    want = 1.0 / np.sqrt(r * r + 1.0)
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (r[~ok][:5], got[~ok][:5], want[~ok][:5])


def test_sqrt_correctly_rounded(probe):
    """sqrt_unscaled<true> on its stated domain (0, +inf, x >= 2^-767) equals IEEE sqrt"""
    rng = np.random.default_rng(24)
    n = 1_000_000
    x = np.ldexp(1.0 + rng.random(n), rng.integers(-767, 1024, n))  # every binade of the domain
    hard = _midpoint_squares(rng, 4000, 1.0, 2.0)
    e = 2 * rng.integers(-383, 511, hard.size)  # even powers of two keep them hard
    hard = np.concatenate([np.ldexp(hard, e), hard])
    hard = np.concatenate([hard.view(np.int64) + k for k in (-1, 0, 1)]).view(np.float64)
    edge = np.array([2.0**-767, np.nextafter(2.0**-767, 1.0), 2.0**-766, 0.0, np.inf,
                     np.finfo(np.float64).max, 1.0, 2.0, 4.0, np.nan])
    x = np.concatenate([x, hard[(hard >= 2.0**-767) & np.isfinite(hard)], edge])
    got = M.f64(probe("sqrt", x.view(np.uint64)))
    want = np.sqrt(x)
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (x[~ok][:5], got[~ok][:5], want[~ok][:5])


def test_u01_correctly_rounded(probe):
    """(double)z 2^-64 is z / 2^64 rounded to nearest, ties to even"""
    rng = np.random.default_rng(25)
    z = draws(rng, 200_000)
    ties = [2**63 + (2 * int(j) + 1) * 2**10 for j in rng.integers(0, 2**51, 1000)] + \
           [2**53 + 2 * int(j) + 1 for j in rng.integers(0, 2**51, 1000)]
    z = np.concatenate([z, np.array(ties, dtype=np.uint64)])
    got = M.f64(probe("u01", z))
    want = np.array([float(Fraction(int(v), 2**64)) for v in z])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
