"""The 256-bit references of tests/golden/math_ref.npz (written by tests/golden/gen_math_ref.py) and
the accuracy bound each deterministic primitive of nlsg_math.h is held to. Shared by the oracle's
test (test_math_accuracy_cpu.py) and the device's (test_math_accuracy_gpu.py); needs no mpmath.

A probe is any callable (name, uint64 bit patterns) -> uint64 bit patterns of the results.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "math_ref.npz")

O_THRESHOLD = 7.09782712893383973096e+02   # fdlibm's: exp overflows above it
U_THRESHOLD = -7.45133219101941108420e+02  # fdlibm's: exp underflows to 0 below it
TWO_PI = 2 * 3.14159265358979323846        # det_cos_2pi's two_pi
ULP53 = 2.0**-53

# every primitive with 256-bit references, as the probes name them
ACCURACY = ("log", "log_unit", "exp", "tanh", "cos", "cos_2pi", "rnorm", "rnorm_cos", "u01")


def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def arguments(ref, name):
    return ref[("rnorm" if name == "rnorm_cos" else name) + "_x"]


def f64(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def ulp_of(hi, lo):
    """ulp of the exact value hi + lo (hi its correctly rounded double); 2^-1074 at the least"""
    m, e = np.frexp(np.abs(hi))
    below = (m == 0.5) & (np.sign(lo) == -np.sign(hi))  # hi a power of two, the exact value below it
    return np.ldexp(1.0, np.maximum(e - 53 - below.astype(np.int64), -1074))


def error(y, hi, lo):
    """y - (hi + lo), to about 106 bits (y - hi is exact wherever the bound is met)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (y - hi) - lo


def _report(name, x, y, hi, bad):
    i = np.flatnonzero(bad)[:5]
    return f"{name}: {bad.sum()} of {bad.size} out of bounds, e.g. x={x[i]!r} got={y[i]!r} exact~{hi[i]!r}"


def check(name, ref, probe):
    """probe's results for every fixture argument of `name` against the stated bound"""
    u = arguments(ref, name)
    y = f64(probe(name, u))
    hi, lo = ref[name + "_hi"], ref[name + "_lo"]
    x = u if name in ("rnorm", "rnorm_cos", "u01") else f64(u)
    if name == "u01":  # (double)z 2^-64 is one correctly rounded conversion
        bad = y.view(np.uint64) != hi.view(np.uint64)
    elif name in ("log", "log_unit"):
        # log: fdlibm's kernel on every positive finite input (subnormal ones scaled by 2^54
        # first) is within 1 ulp; log_unit: the claim of nlsg_math.h's table logarithm on [2^-64, 1]
        bound = 1.0 if name == "log" else 0.62
        bad = ~(np.abs(error(y, hi, lo)) <= bound * ulp_of(hi, lo))
    elif name == "exp":
        s = ref["exp_scale"]
        over, under = x > O_THRESHOLD, x < U_THRESHOLD
        ys = np.ldexp(y, s)  # the fixture holds exp(x) 2^s: the scaling is exact
        d = np.abs(error(ys, hi, lo))
        normal = np.abs(hi) >= np.ldexp(1.0, -1022 + s)
        bad = np.where(over, y != np.inf,          # +inf exactly above the overflow threshold
              np.where(under, y.view(np.uint64) != 0,  # +0 exactly below the underflow threshold
              np.where(normal, ~(d <= ulp_of(hi, lo)),  # normal results: <= 1 ulp
                       ~(d <= np.ldexp(1.0, -1074 + s)))))  # subnormal: one rounding of y 2^k
    elif name == "tanh":
        # numerator and denominator <= 1 ulp each, plus the rounding of the division: <= 2.5 ulp;
        # from |x| = 22 on the result is +-1 exactly
        big = np.abs(x) >= 22.0
        bad = np.where(big, y != np.copysign(1.0, x),
                       ~(np.abs(error(y, hi, lo)) <= 2.5 * ulp_of(hi, lo)))
    elif name == "cos":
        # two-term Cody-Waite: |r|'s absolute error stays ~2^-86 and the kernels add < 1 ulp of 1,
        # so <= 1.5 2^-53 absolute everywhere; <= 1.5 ulp where the value is not near a zero
        d = np.abs(error(y, hi, lo))
        bad = ~(d <= 1.5 * ULP53)
        away = np.abs(hi) >= 2.0**-5
        bad |= away & ~(d <= 1.5 * ulp_of(hi, lo))
    elif name == "cos_2pi":
        # against cos(fl(2 pi x)): det_cos's bound while fl(2 pi x) is in det_cos's range; beyond,
        # the period is taken off x before the product is rounded, which moves the argument by up
        # to the rounding of fl(2 pi x)
        t = TWO_PI * x
        d = np.abs(error(y, hi, lo))
        bad = np.where(np.abs(t) <= 64.0, ~(d <= 1.5 * ULP53), ~(d <= np.spacing(np.abs(t)) + ULP53))
    elif name == "rnorm":
        # 0.31 + 0.5 + 0.5 ulp from log, sqrt and product (relative, times R) plus the cosine's
        # 2.3e-16 (absolute, times R): <= 3.7e-16 R
        bad = ~(np.abs(error(y, hi, lo)) <= 3.7e-16 * ref["rnorm_R"])
    elif name == "rnorm_cos":
        # nlsg_math.h's claim for det_rnorm_cos: <= 2.3e-16 absolute
        bad = ~(np.abs(error(y, hi, lo)) <= 2.3e-16)
    else:
        raise ValueError(name)
    assert not bad.any(), _report(name, x, y, hi, bad)
    return u, y


# exact values: (primitive, argument, result) compared bit for bit (NaN: any NaN)
SPECIALS = [
    ("log", 0.0, -np.inf), ("log", -0.0, -np.inf), ("log", 1.0, 0.0), ("log", np.inf, np.inf),
    ("log", -1.0, np.nan), ("log", -np.inf, np.nan), ("log", np.nan, np.nan),
    ("log", -5e-324, np.nan),
    ("log_unit", 1.0, 0.0),
    ("exp", 0.0, 1.0), ("exp", -0.0, 1.0), ("exp", np.inf, np.inf), ("exp", -np.inf, 0.0),
    ("exp", np.nan, np.nan), ("exp", 709.79, np.inf), ("exp", 1e300, np.inf),
    ("exp", -745.14, 0.0), ("exp", -1e300, 0.0), ("exp", 5e-324, 1.0), ("exp", -5e-324, 1.0),
    ("tanh", 0.0, 0.0), ("tanh", -0.0, -0.0), ("tanh", np.inf, 1.0), ("tanh", -np.inf, -1.0),
    ("tanh", np.nan, np.nan), ("tanh", 22.0, 1.0), ("tanh", -22.0, -1.0), ("tanh", 1e300, 1.0),
    ("tanh", 5e-324, 5e-324), ("tanh", -5e-324, -5e-324),
    ("cos", 0.0, 1.0), ("cos", -0.0, 1.0), ("cos", 64.00000001, np.nan),
    ("cos", -64.00000001, np.nan), ("cos", np.inf, np.nan), ("cos", -np.inf, np.nan),
    ("cos", np.nan, np.nan),
    ("cos_2pi", 0.0, 1.0), ("cos_2pi", -0.0, 1.0), ("cos_2pi", 2.0**52, 1.0),
    ("cos_2pi", -(2.0**52), 1.0), ("cos_2pi", np.nan, np.nan), ("cos_2pi", np.inf, np.nan),
    ("sqrt", 0.0, 0.0), ("sqrt", -0.0, -0.0), ("sqrt", np.inf, np.inf), ("sqrt", np.nan, np.nan),
    ("sqrt", 1.0, 1.0), ("sqrt", 4.0, 2.0),
    ("givens_t", 0.0, 1.0), ("givens_t", -0.0, 1.0), ("givens_t", np.nan, np.nan),
    ("givens_t", 5e-324, 1.0),
]


def check_specials(probe):
    by_fn = {}
    for fn, x, want in SPECIALS:
        by_fn.setdefault(fn, []).append((x, want))
    for fn, cases in by_fn.items():
        x = np.array([c[0] for c in cases])
        want = np.array([c[1] for c in cases])
        got = f64(probe(fn, x.view(np.uint64)))
        ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint64) == want.view(np.uint64))
        assert ok.all(), (fn, x[~ok], got[~ok], want[~ok])


def rnorm_special_expected(z):
    """the reference's expression sqrt(-2 log u1) cos(2 pi_ u2) for z = 0 (u1 = 0: +inf times the
    cosine of 0) and z >= 2^64 - 2^10 (u1 rounds to 1: sqrt(-0) = -0 times the cosine)"""
    import math
    u1 = float(int(z)) * 2.0**-64
    y = float(int(z) & 0xFFFFFFFF) * (2 * 3.141593 * 2.0**-32)
    r = math.inf if u1 == 0.0 else math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(y)


RNORM_SPECIAL_DRAWS = [0, 2**64 - 2**10, 2**64 - 2**10 + 1, 2**64 - 2**9, 2**64 - 2, 2**64 - 1]
