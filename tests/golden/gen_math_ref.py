#!/usr/bin/env python3
"""Regenerate tests/golden/math_ref.npz: 256-bit references for the deterministic fp64 primitives
of nlsolver_amd/csrc/nlsg_math.h (and their copies in oracle/oracle_math.c, oracle_lm.c).

For each primitive P the archive holds
  P_x        the arguments: a double's bit pattern, or the 64-bit draw for rnorm / u01 (rnorm_cos
             shares rnorm_x)
  P_hi, P_lo the exact result as a double-double, hi = the correctly rounded double; the error of a
             double d is then (d - hi) - lo to ~106 bits, without mpmath at test time
plus exp_scale (the exact exp(x) is stored times 2^exp_scale, so that results beyond the double
range keep their precision) and rnorm_R (sqrt(-2 ln u1), rounded: the scale of rnorm's bound).

The arguments are drawn from fixed seeds where the primitives go wrong: every binade, both sides of
every argument-reduction rounding point and table edge, the overflow / underflow thresholds, the
zeros of the cosine. Needs mpmath; the tests read only the archive (tests/test_math_accuracy_*.py),
except for a seeded re-computation of a sample when mpmath happens to import.
Runtime: a few seconds. The archive is written byte for byte reproducibly
(uncompressed members, fixed timestamps).
"""
import io
import math
import os
import struct
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "math_ref.npz")
PREC = 256

# the constants of nlsg_math.h that decide where the reductions switch
INVLN2 = 1.44269504088896338700e+00
INVPIO2 = 6.36619772367581382433e-01
TWO_PI = 2 * 3.14159265358979323846          # det_cos_2pi's two_pi
ANGLE = 2 * 3.141593 * 2.0**-32               # det_rnorm's lo_d -> angle factor, 2 pi_ 2^-32
O_THRESHOLD = 7.09782712893383973096e+02
U_THRESHOLD = -7.45133219101941108420e+02


def d2b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def b2d(u):
    return struct.unpack("<d", struct.pack("<Q", int(u)))[0]


def step(x, n):
    """the double n ulps above x (n < 0: below)"""
    for _ in range(abs(n)):
        x = math.nextafter(x, math.inf if n > 0 else -math.inf)
    return x


def around(x, n):
    return [step(x, j) for j in range(-n, n + 1)]


def _mp():
    import mpmath
    mpmath.mp.prec = PREC
    return mpmath


def to_dd(v):
    """(hi, lo): hi = v rounded to the nearest double, lo = v - hi rounded"""
    mp = _mp()
    if v == 0:
        return 0.0, 0.0
    if abs(v) < mp.ldexp(1, -1022):  # subnormal: round on the 2^-1074 grid
        hi = math.ldexp(int(mp.nint(mp.ldexp(v, 1074))), -1074)
    else:
        hi = float(v)
    if math.isinf(hi):
        return hi, 0.0
    return hi, float(v - mp.mpf(hi))


# ---- the exact functions: argument (bit pattern or draw) -> mpf --------------------------------
def u01_of(z):
    return float(int(z)) * 2.0**-64      # (double)z 2^-64: one rounding, as the device converts


def rnorm_angle(z):
    return float(int(z) & 0xFFFFFFFF) * ANGLE  # fl(2 pi_ u2): the one rounding of the angle


def exact(name, u):
    """the exact value of primitive `name` at argument u (mpf), scaled as the archive stores it"""
    mp = _mp()
    if name == "u01":
        return mp.ldexp(mp.mpf(int(u)), -64)
    if name in ("rnorm", "rnorm_cos"):
        c = mp.cos(mp.mpf(rnorm_angle(u)))
        if name == "rnorm_cos":
            return c
        return mp.sqrt(-2 * mp.log(mp.mpf(u01_of(u)))) * c
    x = mp.mpf(b2d(u))
    if name in ("log", "log_unit"):
        return mp.log(x)
    if name == "exp":
        return mp.ldexp(mp.exp(x), exp_scale(b2d(u)))
    if name == "tanh":
        return mp.tanh(x)
    if name == "cos":
        return mp.cos(x)
    if name == "cos_2pi":
        return mp.cos(mp.mpf(TWO_PI * b2d(u)))  # against cos(fl(2 pi x)), the reference's Rastrigin
    raise ValueError(name)


def exp_scale(x):
    return 1000 if x < -700.0 else (-16 if x > 700.0 else 0)


# ---- argument sets --------------------------------------------------------------------------
def args_log(rng):
    xs = []
    for e in range(1, 2047):  # every normal binade, one random mantissa each
        xs.append(b2d((e << 52) | int(rng.integers(0, 2**52))))
    for j in range(52):  # every subnormal binade
        xs.append(b2d((1 << j) | int(rng.integers(0, 2**j)) if j else 1))
    xs += [5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308, 1.0]
    xs += list(1.0 + (2 * rng.random(500) - 1) * 2.0**-10)  # [1 - 2^-10, 1 + 2^-10] densely
    xs += around(1.0, 16)
    for k in range(-4, 5):  # both sides of the sqrt(1/2) split, m = 0x3fe6a09e.... in several binades
        hx = 0x3FE6A09E + (k << 20)
        for lw in (0, 1, 2, 0xFFFFFFFF):
            xs.append(b2d((hx << 32) | lw))
            xs.append(b2d(((hx - 1) << 32) | lw))
    xs.append(math.sqrt(0.5))
    xs += around(math.sqrt(0.5), 3) + around(math.sqrt(2.0), 3)
    return xs


def args_log_unit(rng):
    xs = []
    for e in range(-64, 0):  # [2^-64, 1] by binade
        xs += list(np.ldexp(1.0 + rng.random(6), e))
    xs += [2.0**-64, 1.0, step(1.0, -1), step(1.0, -2), 0.5, step(0.5, 1)]
    for j in range(128):  # every table subinterval: both edges and the centre
        for t20, lw in ((j << 13, 0), ((j << 13) + 4096, 0x12345678), (((j + 1) << 13) - 1, 0xFFFFFFFF)):
            m_ge_1 = t20 + 0x3FE6A09E >= 0x3FF00000
            for k in ((-1, -40) if m_ge_1 else (0, -1, -40)):
                hx = (((k + 0x3FF) << 20) | t20) - 0x3FF00000 + 0x3FE6A09E
                xs.append(b2d((hx << 32) | lw))
    return [x for x in xs if 2.0**-64 <= x <= 1.0]


def args_exp(rng):
    xs = list(4 * rng.random(600) - 2)  # [-2, 2]
    xs += [0.0, -0.0, 1.0, -1.0, 2.0**-30, -(2.0**-30), 2.0**-60]
    mp = _mp()
    for n in range(1, 1025):  # k = trunc(invln2 x + 1/2) steps at x = (n - 1/2) / invln2
        d = float((n - mp.mpf(0.5)) / mp.mpf(INVLN2))
        if d <= O_THRESHOLD:
            xs += [step(d, -1), step(d, 1)]
    for n in range(1, 1076):  # k = trunc(invln2 x - 1/2) steps at x = -(n - 1/2) / invln2
        d = float(-(n - mp.mpf(0.5)) / mp.mpf(INVLN2))
        if d >= U_THRESHOLD:
            xs += [step(d, -1), step(d, 1)]
    xs += list(709.0 + 0.79 * rng.random(200))                 # [709, 709.79]
    xs += list(-708.0 - 37.2 * rng.random(500))                # [-745.2, -708]
    xs += list(-745.2 + 1.2 * rng.random(200))                 # the subnormal-result end, densely
    xs += around(O_THRESHOLD, 3) + around(U_THRESHOLD, 3)
    xs += around(709.0, 2) + around(-708.0, 2) + [709.1, -708.1, 709.7, -745.0, -744.0, -740.0]
    return xs


def args_tanh(rng):
    xs = []
    for e in range(-1074, 0, 6):  # tiny |x| down to subnormal
        x = math.ldexp(1.0 + rng.random(), e) if e > -1022 else math.ldexp(float(rng.integers(1, 2**20)), e)
        xs += [x, -x]
    mp = _mp()
    for n in range(1, 65):  # k = trunc(invln2 2|x| + 1/2) steps at |x| = (n - 1/2) / (2 invln2)
        d = float((n - mp.mpf(0.5)) / (2 * mp.mpf(INVLN2)))
        for x in (step(d, -1), step(d, 1)):
            xs += [x, -x]
    xs += list(0.3 + 0.9 * rng.random(800))    # [0.3, 1.2] densely
    xs += list(22 * rng.random(400)) + list(50 * rng.random(200) - 25)
    xs += around(22.0, 3) + [-x for x in around(22.0, 3)] + [14.93, 3.19, -3.19, 21.9, 30.0]
    return xs


def args_cos(rng):
    xs = list(128 * rng.random(1000) - 64) + list(2 * rng.random(200) - 1)
    xs += [0.0, 1e-300, 2.0**-27, 64.0, -64.0, step(64.0, -1), step(-64.0, 1), -45.553093477052]
    mp = _mp()
    for k in range(-40, 41):  # the nearest doubles to every k pi / 2 in range
        xs += around(float(k * mp.pi / 2), 3)
    for n in range(-40, 42):  # fn = floor(y invpio2 + 1/2) steps at y = (n - 1/2) / invpio2
        xs += around(float((n - mp.mpf(0.5)) / mp.mpf(INVPIO2)), 2)
    return [x for x in xs if -64.0 <= x <= 64.0]


def args_cos_2pi(rng):
    xs = list(10.24 * rng.random(1000) - 5.12)  # Rastrigin's domain
    for j in range(-20, 21):                    # quarter-integers
        xs += around(j / 4, 2)
    edge = 64.0 / TWO_PI                          # the branch at |fl(2 pi x)| = 64
    for x in around(edge, 3):
        xs += [x, -x]
    for e in range(4, 53):                        # large |x| up to 2^52
        for x in np.ldexp(1.0 + rng.random(3), e):
            xs += [float(x), -float(x)]
    xs += [2.0**52, -(2.0**52), 1.4e5, 1e6 + 0.25]
    return xs


def args_draws(rng):
    z = [int(v) for v in rng.integers(0, 2**64, size=800, dtype=np.uint64)]
    z += [int(v) >> int(s) for v, s in zip(rng.integers(0, 2**64, size=400, dtype=np.uint64),
                                          rng.integers(0, 64, size=400))]  # u1 -> 2^-64
    z += [int(v) | ((2**64 - 1) ^ ((2**64 - 1) >> int(s))) for v, s in
          zip(rng.integers(0, 2**64, size=300, dtype=np.uint64), rng.integers(1, 54, size=300))]  # u1 just below 1
    for f in (0.25, 0.5, 0.75):  # low 32 bits where the angle crosses pi/2, pi, 3 pi/2
        lo = int(round(2 * math.pi * f / ANGLE))
        for d in range(-3, 4):
            for hi in (1, 0x7FFFFFFF, int(rng.integers(1, 2**32))):
                z.append((hi << 32) | (lo + d))
    z += [1, 2, 2**32 - 1, 2**32, 2**63, 2**53, 2**53 + 1, 2**64 - 2**11, 2**64 - 2**10 - 1]
    z += [2**k for k in range(64)] + [2**64 - 2**k for k in range(11, 64)]
    return [v for v in z if v != 0 and v < 2**64 - 2**10]  # the special draws: exact checks in the tests


def args_u01():
    return [0, 1, 2, 3, 2**32 - 1, 2**32, 2**32 + 1, 2**63, 2**64 - 1, 2**64 - 2**11, 2**64 - 2**10,
            2**53, 2**53 + 1, 2**64 - 2**10 - 1, 2**64 - 2**10 + 1, 2**54 + 2, 2**54 + 6] + \
           [2**k for k in range(64)] + [2**64 - 2**k for k in range(64)]


SEEDS = {"log": 101, "log_unit": 102, "exp": 103, "tanh": 104, "cos": 105, "cos_2pi": 106, "draws": 107}


def arguments():
    """name -> uint64 array of arguments, deduplicated in first-seen order"""
    sets = {
        "log": [d2b(x) for x in args_log(np.random.default_rng(SEEDS["log"]))],
        "log_unit": [d2b(x) for x in args_log_unit(np.random.default_rng(SEEDS["log_unit"]))],
        "exp": [d2b(x) for x in args_exp(np.random.default_rng(SEEDS["exp"]))],
        "tanh": [d2b(x) for x in args_tanh(np.random.default_rng(SEEDS["tanh"]))],
        "cos": [d2b(x) for x in args_cos(np.random.default_rng(SEEDS["cos"]))],
        "cos_2pi": [d2b(x) for x in args_cos_2pi(np.random.default_rng(SEEDS["cos_2pi"]))],
        "rnorm": args_draws(np.random.default_rng(SEEDS["draws"])),
        "u01": args_u01(),
    }
    sets["rnorm_cos"] = sets["rnorm"]
    return {k: np.array(list(dict.fromkeys(v)), dtype=np.uint64) for k, v in sets.items()}


def build_arrays():
    arrays = {}
    for name, xs in arguments().items():
        hl = [to_dd(exact(name, u)) for u in xs]
        if name != "rnorm_cos":  # the same draws as rnorm
            arrays[name + "_x"] = xs
        arrays[name + "_hi"] = np.array([h for h, _ in hl], dtype=np.float64)
        arrays[name + "_lo"] = np.array([lo for _, lo in hl], dtype=np.float64)
        if name == "exp":
            arrays["exp_scale"] = np.array([exp_scale(b2d(u)) for u in xs], dtype=np.int32)
        if name == "rnorm":
            mp = _mp()
            arrays["rnorm_R"] = np.array([float(mp.sqrt(-2 * mp.log(mp.mpf(u01_of(u))))) for u in xs])
    return arrays


def write_npz(path, arrays):
    """np.savez's layout, with fixed member timestamps and no compression: reproducible bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    arrays = build_arrays()
    write_npz(OUT, arrays)
    n = sum(a.size for k, a in arrays.items() if k.endswith("_hi"))
    print(f"wrote {OUT}: {n} arguments, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
