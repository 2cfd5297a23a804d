"""The systems that take tinyqr off the benign path, and their references — shared by
tests/test_tinyqr_cases_cpu.py, tests/test_tinyqr_hostile_gpu.py and
tests/golden/gen_golden_tinyqr_hostile.py. Nothing here touches the device side.

A system is X of shape (p, n) — the column-major n x p matrix tinyqr takes — with y (n,) and the
`tol` of lm()'s cleanup. Three kinds:

  graded   Vandermonde, Hilbert-like, small integers, columns or rows scaled over hundreds of
           binades: full rank, compared with the EXACT least-squares solution (exact_beta: rational
           arithmetic on the exact values of the float inputs, owing nothing to the oracle or to
           numpy) under the project's bound 8 cond eps max|beta|, cond taken of X with its columns
           scaled to unit length (Givens QR is invariant under power-of-two column scaling; the
           unscaled cond of a column-graded matrix bounds nothing).
  hostile  integer bases (everything not poisoned is exact) with stacked zeros, non-finite entries,
           scalings to the ends of the exponent range, and every kind of `tol`. The reference's
           Givens pair (tinyqr.h:86-97) has no guard for a = b = 0: r = 0 / 0, and NaN runs through
           the rest of the solve. Compared bit for bit only.
  wide     every family again at the column counts of the wavefront kernel's three workgroup
           variants, p in WIDTHS; members of more than 12 columns are compared bit for bit only.

BASE cases (n <= 40, p <= 12) are stored with their inputs and the unmodified reference's outputs in
tests/golden/tinyqr_hostile.json; the wide members are regenerated from here and pinned there by hash.
"""
from fractions import Fraction
from typing import NamedTuple

import numpy as np

EPS = 2.0 ** -52
WIDTHS = (3, 8, 9, 32, 33, 64)  # (128, 8), (256, 32), (512, 64) threads: both sides of each edge
DEFAULT_TOL = 1e-12            # lm()'s third argument (tinyqr.h:464)


class Case(NamedTuple):
    name: str
    X: np.ndarray    # (p, n), C-contiguous
    y: np.ndarray    # (n,)
    tol: float
    kind: str        # "graded" | "hostile"
    bound: str       # graded: "cond" (8 cond eps max|beta|) | "literal" (8 x the literal oracle's error); else ""

    @property
    def n(self):
        return self.X.shape[1]

    @property
    def p(self):
        return self.X.shape[0]


# ---- equality and hashing ----------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal bit for bit, NaN equal to NaN: the sign of zero and of inf counts, a NaN's sign and payload do not"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def fnv(a):
    """FNV-1a over the doubles' bytes, every NaN read as the one quiet NaN (ref_driver tinyqr-hex)"""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1).copy()
    a[np.isnan(a)] = np.float64("nan")
    h = 1469598103934665603
    for b in a.view(np.uint8).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def hexes(a):
    return [float(v).hex() for v in np.ravel(a)]


def unhex(vals):
    return np.array([float.fromhex(v) for v in vals], dtype=np.float64)


# ---- the exact solver --------------------------------------------------------------------------------

def exact_beta(X, y):
    """The least-squares solution of the (p, n) system as Fractions: Gauss-Jordan on the normal
    equations X^T X beta = X^T y, formed from the exact rational values of the float inputs.
    None where X^T X is singular. Inputs must be finite."""
    p, n = X.shape
    cols = [[Fraction(float(v)) for v in X[j]] for j in range(p)]
    yy = [Fraction(float(v)) for v in y]
    A = [[sum(cols[i][k] * cols[j][k] for k in range(n)) for j in range(p)] +
         [sum(cols[i][k] * yy[k] for k in range(n))] for i in range(p)]
    for c in range(p):
        piv = next((r for r in range(c, p) if A[r][c] != 0), None)
        if piv is None:
            return None
        A[c], A[piv] = A[piv], A[c]
        inv = 1 / A[c][c]
        A[c] = [v * inv for v in A[c]]
        for r in range(p):
            if r != c and A[r][c] != 0:
                f = A[r][c]
                A[r] = [a - f * b for a, b in zip(A[r], A[c])]
    return [A[i][p] for i in range(p)]


def max_error(beta, exact):
    """max_i |beta_i - exact_i| as a float, the difference taken exactly; inf if beta is not finite"""
    if not np.all(np.isfinite(beta)):
        return float("inf")
    return float(max(abs(Fraction(float(b)) - e) for b, e in zip(beta, exact)))


def scaled_cond(X):
    """cond_2 of the n x p matrix with its columns scaled to unit 2-norm"""
    A = np.asarray(X, dtype=np.float64).T
    m, e = np.frexp(A)  # norms of columns of 2^-160 .. 2^120 without leaving the range: scale by 2^-max e first
    A = np.ldexp(m, e - e.max(axis=0, keepdims=True))
    return float(np.linalg.cond(A / np.linalg.norm(A, axis=0, keepdims=True)))


def cond_bound(X, exact):
    """the project's bound (tests/test_tinyqr_gpu.py, tests/test_lm_planted_gpu.py): 8 cond eps max|beta|"""
    return 8.0 * scaled_cond(X) * EPS * float(max(abs(e) for e in exact))


# ---- building blocks ---------------------------------------------------------------------------------

def ints(seed, n, p, amp=9):
    """n x p of non-zero integers in [-amp, amp] from a 64-bit LCG: the same on every machine"""
    s = (seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    out = np.empty(n * p)
    for k in range(n * p):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        v = (s >> 33) % (2 * amp)
        out[k] = v - amp if v < amp else v - amp + 1
    return out.reshape(n, p)


def _case(name, A, y, tol=DEFAULT_TOL, kind="hostile", bound=""):
    """A: the n x p matrix as written on paper"""
    return Case(name, np.ascontiguousarray(np.asarray(A, dtype=np.float64).T),
                np.ascontiguousarray(y, dtype=np.float64), float(tol), kind, bound)


# ---- graded families: core(n, p) -> (A, y) -----------------------------------------------------------

def _vandermonde(n, p):
    t = np.arange(1, n + 1) / n
    return np.stack([t ** j for j in range(p)], axis=1), ints(11, n, 1, 5)[:, 0]


def _hilbert(n, p):
    i, j = np.arange(n)[:, None], np.arange(p)[None, :]
    return 1.0 / (i + j + 1), ints(12, n, 1, 5)[:, 0]


def _small_int(n, p):
    return ints(13, n, p), ints(14, n, 1)[:, 0]


def _col_graded(n, p):
    """integer entries times 2^(40 j - 160) per column (j mod 8: the grading repeats in a wider core)"""
    return np.ldexp(ints(15, n, p), (40 * (np.arange(p) % 8) - 160)[None, :]), ints(16, n, 1)[:, 0]


def _row_graded(n, p):
    """rows (of X and y alike) times 2^e, e from -200 to 200 in whole steps: a weighted fit whose weights span
    400 binades"""
    e = np.round(np.linspace(-200, 200, n)).astype(int)
    return np.ldexp(ints(17, n, p), e[:, None]), np.ldexp(ints(18, n, 1)[:, 0], e)


# col_graded runs with tol = 0: the rotations are invariant under a column's power of two, lm()'s cleanup is
# not — at the default tol it reads the whole columns of 2^-160 .. 2^-40 as 0 and the solve divides by them
GRADED = {  # name: (core, n, p, bound, tol)
    "vandermonde_40x6": (_vandermonde, 40, 6, "cond", DEFAULT_TOL),
    "vandermonde_40x9": (_vandermonde, 40, 9, "cond", DEFAULT_TOL),
    "vandermonde_40x12": (_vandermonde, 40, 12, "cond", DEFAULT_TOL),
    "vandermonde_24x12": (_vandermonde, 24, 12, "cond", DEFAULT_TOL),
    "hilbert_12x8": (_hilbert, 12, 8, "cond", DEFAULT_TOL),
    "hilbert_20x10": (_hilbert, 20, 10, "cond", DEFAULT_TOL),
    "small_int_30x8": (_small_int, 30, 8, "cond", DEFAULT_TOL),
    "col_graded_30x8": (_col_graded, 30, 8, "cond", 0.0),
    "row_graded_30x8": (_row_graded, 30, 8, "literal", DEFAULT_TOL),
}


def _graded(name, width=None):
    core, n, p, bound, tol = GRADED[name]
    if width is None:
        A, y = core(n, p)
        return _case(name, A, y, tol, kind="graded", bound=bound)
    # embedded at `width` columns: the family's first min(p, width) columns, then orthogonal-ish integer
    # columns (dense: a zero block under a pivot would meet the reference's 0 / 0), rows as needed
    n = max(n, width + 7)
    pc = min(p, width)
    A, y = core(n, pc)
    A = np.concatenate([A, ints(19 + width, n, width - pc)], axis=1)
    return _case(f"{name}@{width}", A, y, tol, kind="graded", bound=bound)


# ---- hostile families: f(n, p) -> (A, y, tol) --------------------------------------------------------

def _base(n, p, amp=9):
    return ints(21, n, p, amp), ints(22, n, 1, amp)[:, 0]


def _zeros_bottom_col0(n, p):
    A, y = _base(n, p)
    A[n - 2:, 0] = 0.0
    return A, y, DEFAULT_TOL


def _zero_column(n, p):
    A, y = _base(n, p)
    A[:, p // 2] = 0.0
    return A, y, DEFAULT_TOL


def _identity_over_zero_rows(n, p):
    A = np.zeros((n, p))
    A[:p] = np.eye(p)
    return A, _base(n, p)[1], DEFAULT_TOL


def _one_hot(n, p):
    A = np.zeros((n, p))
    A[np.arange(n), np.arange(n) % p] = 1.0
    return A, _base(n, p)[1], DEFAULT_TOL


def _zero_rows_bottom(n, p):
    A, y = _base(n, p)
    A[n - 3:] = 0.0
    return A, y, DEFAULT_TOL


def _zero_rows_top(n, p):
    A, y = _base(n, p)
    A[:3] = 0.0
    return A, y, DEFAULT_TOL


def _last_row_only_column(n, p):
    A, y = _base(n, p)
    A[:n - 1, p // 2] = 0.0
    return A, y, DEFAULT_TOL


def _inf_in_X(n, p):
    """inf in the first column: it climbs to R(0, 0) by rotations of (c, s) = (1, 0) and (0, 1) that leave the
    other columns finite, and beta_0 = finite / inf = 0"""
    A, y = _base(n, p)
    A[n // 2, 0] = np.inf
    return A, y, DEFAULT_TOL


def _inf_in_X_mid(n, p):
    """inf in a later column: the rotations of the columns before it spread it over two rows, whose pair is
    inf / inf"""
    A, y = _base(n, p)
    A[n // 2, p // 2] = np.inf
    return A, y, DEFAULT_TOL


def _nan_in_X(n, p):
    A, y = _base(n, p)
    A[n // 2, p // 2] = np.nan
    return A, y, DEFAULT_TOL


def _nan_in_y(n, p):
    A, y = _base(n, p)
    y[n // 2] = np.nan
    return A, y, DEFAULT_TOL


def _inf_in_y(n, p):
    A, y = _base(n, p)
    y[n // 2] = np.inf
    return A, y, DEFAULT_TOL


def _scaled(k, tol, with_y=False):
    """X 2^k; with_y: y 2^k too, so that beta stays O(1) where X is denormal (y / X would overflow)"""
    def f(n, p):
        A, y = _base(n, p, 3)  # |entries| <= 3: at the base shape a column's norm stays below 8
        return np.ldexp(A, k), np.ldexp(y, k) if with_y else y, tol
    return f


def _tol_dup(tol):
    """a duplicated column: the last pivot is a rounding remnant, which `tol` keeps or reads as 0"""
    def f(n, p):
        A, y = _base(n, p)
        A[:, p - 1] = A[:, p - 2] if p > 1 else A[:, 0]
        return A, y, tol
    return f


def _tol_mix(tol):
    """full rank with one column at 2^-12: entries of R on both sides of 1e-3, all far above 1e-12"""
    def f(n, p):
        A, y = _base(n, p)
        A[:, p // 2] = np.ldexp(A[:, p // 2], -12)
        return A, y, tol
    return f


TOLS = {"0": 0.0, "1e-12": 1e-12, "1e-3": 1e-3, "inf": float("inf"), "nan": float("nan"), "neg": -1.0}

HOSTILE = {  # name: (family, n, p)
    "zeros_bottom_col0": (_zeros_bottom_col0, 12, 5),
    "zero_column": (_zero_column, 12, 5),
    "identity_over_zero_rows": (_identity_over_zero_rows, 12, 5),
    "one_hot_groups": (_one_hot, 12, 4),
    "zero_rows_bottom": (_zero_rows_bottom, 12, 5),
    "zero_rows_top": (_zero_rows_top, 12, 5),
    "last_row_only_column": (_last_row_only_column, 12, 5),
    "inf_in_X": (_inf_in_X, 12, 5),
    "inf_in_X_mid": (_inf_in_X_mid, 12, 5),
    "nan_in_X": (_nan_in_X, 12, 5),
    "nan_in_y": (_nan_in_y, 12, 5),
    "inf_in_y": (_inf_in_y, 12, 5),
    "scale_2^1000": (_scaled(1000, DEFAULT_TOL), 6, 3),
    "scale_2^1021": (_scaled(1021, DEFAULT_TOL), 6, 3),
    "scale_2^-1060": (_scaled(-1060, 0.0, True), 6, 3),
    "scale_2^-1074": (_scaled(-1074, 0.0, True), 6, 3),
}
HOSTILE.update({f"tol_dup_{k}": (_tol_dup(v), 12, 5) for k, v in TOLS.items()})
HOSTILE.update({f"tol_mix_{k}": (_tol_mix(v), 12, 5) for k, v in TOLS.items()})


def _hostile(name, width=None):
    f, n, p = HOSTILE[name]
    if width is not None:
        n, p, name = width + 7, width, f"{name}@{width}"
    A, y, tol = f(n, p)
    return _case(name, A, y, tol)


# what the unmodified reference returns for the base members (measured: tests/golden/tinyqr_hostile.json;
# asserted in tests/test_tinyqr_cases_cpu.py): "nan" = every coefficient NaN, "finite" = all finite
REFERENCE_PATTERN = {
    "zeros_bottom_col0": "nan", "zero_column": "nan", "identity_over_zero_rows": "nan", "one_hot_groups": "nan",
    "zero_rows_bottom": "nan", "zero_rows_top": "finite", "last_row_only_column": "finite",
    "inf_in_X": "finite", "inf_in_X_mid": "nan", "nan_in_X": "nan", "nan_in_y": "nan",
    "scale_2^1000": "finite", "scale_2^1021": "finite", "scale_2^-1060": "finite", "scale_2^-1074": "finite",
}


# ---- the lists ---------------------------------------------------------------------------------------

def base_cases():
    return [_graded(k) for k in GRADED] + [_hostile(k) for k in HOSTILE]


def wide_cases(width):
    return [_graded(k, width) for k in GRADED] + [_hostile(k, width) for k in HOSTILE]


def all_cases():
    out = base_cases()
    for w in WIDTHS:
        out += wide_cases(w)
    return out


def graded_exact_cases():
    """the graded members the exact solver is asked about: p <= 12"""
    return [_graded(k) for k in GRADED] + [_graded(k, w) for w in WIDTHS if w <= 12 for k in GRADED]


_EXACT = {}


def exact_of(case):
    """exact_beta of a graded case, computed once per process"""
    if case.name not in _EXACT:
        _EXACT[case.name] = exact_beta(case.X, case.y)
    return _EXACT[case.name]


# the literal (order 0) oracle's error on row_graded_30x8 against the exact solution, relative to
# max|beta| — measured in tests/test_tinyqr_cases_cpu.py, which asserts it; the device is held to 8 times
# the oracle's own error on each member (a different but equally stable sequence of roundings)
ROW_GRADED_FACTOR = 8.0


# ---- metamorphic relations (bit-exact with tol = 0: every operation of the solve commutes with a power of
# two or a sign, as long as nothing leaves the normal range) ---------------------------------------------------

META_K = (-60, 37)
META_SYSTEMS = ("small_int_30x8", "vandermonde_40x6", "hilbert_12x8")


def meta_relations(X, y):
    """[(label, X', y', expect)] with expect(beta) -> beta' from the untransformed solution"""
    p = X.shape[0]
    out = []
    for k in META_K:
        out.append((f"X*2^{k}", np.ldexp(X, k), y, lambda b, k=k: np.ldexp(b, -k)))
        out.append((f"y*2^{k}", X, np.ldexp(y, k), lambda b, k=k: np.ldexp(b, k)))
        for j in (0, p // 2, p - 1):
            Xs = X.copy()
            Xs[j] = np.ldexp(Xs[j], k)

            def scaled(b, j=j, k=k):
                b = b.copy()
                b[j] = np.ldexp(b[j], -k)
                return b
            out.append((f"col{j}*2^{k}", Xs, y, scaled))
    for j in (0, p // 2, p - 1):
        Xn = X.copy()
        Xn[j] = -Xn[j]

        def negated(b, j=j):
            b = b.copy()
            b[j] = -b[j]
            return b
        out.append((f"-col{j}", Xn, y, negated))
    return out


def in_safe_range(*arrays):
    """every non-zero magnitude within 2^-500 .. 2^500: products of two rounding remnants (2^-106 of an
    entry) and squares of the largest entries stay normal and finite"""
    for a in arrays:
        a = np.abs(np.asarray(a, dtype=np.float64))
        a = a[a != 0]
        if a.size and not (np.all(np.isfinite(a)) and a.min() >= 2.0 ** -500 and a.max() <= 2.0 ** 500):
            return False
    return True


# ---- the reference-order mode's launch arithmetic (nlsg_tinyqr_qr) ------------------------------------------

def qr_chunk(n, p):
    """systems per launch: the workspace of n (n + p) doubles per system is capped at 2 GiB"""
    return max(1, 2 ** 31 // (8 * n * (n + p)))


MAXCH_EDGES = ((120, 8), (121, 8), (500, 12), (501, 12), (1272, 8))  # W = 128, 129, 512, 513, 1280
MULTI = dict(n=1272, p=8, batch=331, launches=(164, 164, 3))


def maxch(n, p):
    W = n + p
    return 2 if W <= 128 else 8 if W <= 512 else 20
