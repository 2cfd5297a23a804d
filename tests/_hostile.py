"""Hostile objectives for the direct-search solvers, each written twice: as a Python callable (for
tests/_direct_ref.py) and as CustomObjective source text (for the device). TEST INFRASTRUCTURE.

The one rule that makes an exact comparison possible in every summation order and every kernel
layout: a value must not depend on the order of its sum. Every term is an integer of small
magnitude (q is clamped to +-64, so a sum of up to 2^12 terms of q^2 <= 4096 is exact in any
order; the family `huge` scales it by 2^1000, still exact and finite: the longest point used, D = 1026,
gives at most 1026 * 4096 * 2^1000 < 2^1023) or
non-finite (any order gives the same inf or NaN: a sum that holds +inf and -inf is NaN whichever
meets first).

The family is a run-time choice: p(0) = family, p(1), p(2) = thresholds, so one compiled engine
runs all families in one launch with batch row b taking family b (a distinct compiled objective
costs about a second per kernel instantiation). LITERAL is a variant without p(k), for the path
that has no parameter row; VECTOR_SRC is a whole-vector body that returns -0.0 in one region and
+0.0 in another.
"""
import math

import numpy as np

NAN = float("nan")
INF = float("inf")

PLATEAU, ZERO, NAN_BEYOND, ALL_NAN, WALLS, HUGE = 0.0, 1.0, 2.0, 3.0, 4.0, 5.0
FAMILY_NAMES = {PLATEAU: "plateau", ZERO: "zero", NAN_BEYOND: "nan_beyond", ALL_NAN: "all_nan",
                WALLS: "walls", HUGE: "huge"}
N_PARAMS = 3
HUGE_SCALE = 2.0 ** 1000

_Q = "double q = floor(4.0 * xi); q = q < -64.0 ? -64.0 : (q > 64.0 ? 64.0 : q); double pl = q * q;"

# term(xi, xn) of the parametrised family
TERM_SRC = (
    _Q +
    " double fam = p(0), a = p(1), b = p(2);"
    " if (fam == 0.0) return pl;"
    " if (fam == 1.0) return 0.0;"
    " if (fam == 2.0) return xi > a ? __builtin_nan(\"\") : pl;"
    " if (fam == 3.0) return __builtin_nan(\"\");"
    " if (fam == 4.0) return xi < a ? __builtin_inf() : (xi > b ? -__builtin_inf() : pl);"
    " return pl * 0x1p1000;")

# the literal variant: a plateau, NaN beyond 2.25, a +inf wall below -2.5 (no p(k))
LITERAL_SRC = (
    _Q +
    " if (xi > 2.25) return __builtin_nan(\"\");"
    " return xi < -2.5 ? __builtin_inf() : pl;")

# whole-vector body: -0.0 where the clamped floor of 4 x(0) is negative, +0.0 up to p(1), then the
# plateau of the last coordinate
VECTOR_SRC = (
    "double q = floor(4.0 * x(0)); q = q < -64.0 ? -64.0 : (q > 64.0 ? 64.0 : q);"
    " double r = floor(4.0 * x(x.size() - 1)); r = r < -64.0 ? -64.0 : (r > 64.0 ? 64.0 : r);"
    " if (q < 0.0) return -0.0;"
    " if (q < p(1)) return 0.0;"
    " return q + r * r;")


def c_floor(v):
    """floor() of C: NaN, +-inf pass through"""
    if v != v or v in (INF, -INF):
        return v
    return float(math.floor(v))


def _q(xi):
    q = c_floor(4.0 * xi)
    return -64.0 if q < -64.0 else (64.0 if q > 64.0 else q)


def term(xi, row):
    """TERM_SRC, statement by statement"""
    q = _q(xi)
    pl = q * q
    fam, a, b = row[0], row[1], row[2]
    if fam == 0.0:
        return pl
    if fam == 1.0:
        return 0.0
    if fam == 2.0:
        return NAN if xi > a else pl
    if fam == 3.0:
        return NAN
    if fam == 4.0:
        return INF if xi < a else (-INF if xi > b else pl)
    return pl * HUGE_SCALE


def literal_term(xi):
    q = _q(xi)
    pl = q * q
    if xi > 2.25:
        return NAN
    return INF if xi < -2.5 else pl


def family_plain(row):
    """f(x) = sum_i term(x_i) under a parameter row, term by term; the order of the sum is immaterial"""
    row = tuple(float(v) for v in row)

    def f(x):
        acc = 0.0
        for xi in x:
            acc = acc + term(xi, row)
        return acc
    return f


def _terms(x, row):
    """term() over a whole point at once (numpy): the objective is not the subject of these tests
    and a reference run evaluates it 10^5 times; test_direct_rules_cpu holds it to term()"""
    xs = np.asarray(x, dtype=np.float64)
    fam, a, b = row
    with np.errstate(all="ignore"):
        q = np.floor(4.0 * xs)
        q = np.where(q < -64.0, -64.0, np.where(q > 64.0, 64.0, q))
        pl = q * q
        if fam == 0.0:
            return pl
        if fam == 1.0:
            return np.zeros_like(xs)
        if fam == 2.0:
            return np.where(xs > a, NAN, pl)
        if fam == 3.0:
            return np.full_like(xs, NAN)
        if fam == 4.0:
            return np.where(xs < a, INF, np.where(xs > b, -INF, pl))
        return pl * HUGE_SCALE


def family(row):
    """family_plain(row), evaluated with numpy"""
    row = tuple(float(v) for v in row)

    def f(x):
        with np.errstate(all="ignore"):
            return float(np.sum(_terms(x, row)))
    return f


def literal_plain(x):
    acc = 0.0
    for xi in x:
        acc = acc + literal_term(xi)
    return acc


def literal(x):
    xs = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = _terms(xs, (0.0, 0.0, 0.0))
        t = np.where(xs > 2.25, NAN, np.where(xs < -2.5, INF, t))
        return float(np.sum(t))


def vector(row):
    """VECTOR_SRC under a parameter row (only p(1) is read)"""
    b = float(row[1])

    def f(x):
        q, r = _q(x[0]), _q(x[-1])
        if q < 0.0:
            return -0.0
        if q < b:
            return 0.0
        return q + r * r
    return f


# ---- host twins of the source text (tests/test_direct_rules_cpu.py compiles this) ---------------
HOST_TWIN_CPP = r"""
#include <cmath>
#include <cstdint>
static const double *g_row;
static inline double p(uint64_t k) { return g_row[k]; }
static double term_body(double xi, double xn) { (void)xn;
%(term)s
}
static double literal_body(double xi, double xn) { (void)xn;
%(literal)s
}
struct X {
  const double *v; uint64_t n;
  double operator()(uint64_t i) const { return v[i]; }
  uint64_t size() const { return n; }
};
static double vector_body(const X &x, uint64_t D) { (void)D;
%(vector)s
}
extern "C" double twin_term(double xi, const double *row) { g_row = row; return term_body(xi, 0.0); }
extern "C" double twin_literal(double xi) { return literal_body(xi, 0.0); }
extern "C" double twin_vector(const double *x, uint64_t n, const double *row) {
  g_row = row; return vector_body(X{x, n}, n);
}
"""


def host_twin_source():
    return HOST_TWIN_CPP % {"term": TERM_SRC, "literal": LITERAL_SRC, "vector": VECTOR_SRC}
