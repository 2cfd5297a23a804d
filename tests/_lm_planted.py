"""Planted Levenberg-Marquardt problems and a reference of the LM step that owes nothing to the oracle.

The reference (plain Python and numpy, never the oracle):

  _update_with_hessian, _gn_all, lm_link_solve   the serial restatement of the reference's loop
                      (nlsolver.h:251-321, :3513-3543): sequential sums, separate multiply and add, libm.
  update_with_hessian_rows   the same solve with each element's sum taken by numpy's cumsum (strictly
                      sequential, so the same roundings in the same order) for widths at which the
                      triple loop takes minutes; tests/test_lm_planted_cpu.py holds it to the serial one
                      bit for bit.
  gn_at_zero          f, g, H at theta = 0 of a tanh or identity model (J = -A, r = y exactly), each sum
                      in row order with the rows' zero entries left out: adding an exact zero changes no
                      sum, so these are _gn_all's bits without its m n^2 work.
  fraction_solve      the exact solution of (H + lambda I) x = g in fractions.Fraction, by the connected
                      components of H's sparsity (a planted matrix has components of one and two
                      coordinates, which keeps n = 1024 cheap); float(Fraction) rounds once.
  first_step          theta after one step from theta0 = 0: the verdict of is_diagonal on the damped
                      matrix, then either one correctly rounded division per coordinate or the Fraction
                      solution rounded once.

The constructions all start at theta0 = 0, where z = 0, tanh(0) = 0 and the slope is 1: J = -A and r = y
without a rounding, and with small-integer (or dyadic) A and y, H = 2 A^T A and g = -2 A^T y are exact in
any summation order, with or without fma. The first step is then a pure test of the step kernel and of
the evaluation's verdict."""
import math
from fractions import Fraction

import numpy as np

THR = 2.220446049250313e-16 * 1e12   # is_diagonal's threshold, DBL_EPSILON * 1e12
UP, DOWN = 4.0, 2.0
EPS = 2.0 ** -52


# ---- the serial restatement, moved here from tests/test_lm_link_cpu.py: unchanged but for lm_link_solve's
# optional update= (the default path is the old one) and the threshold's name --------------------------------
def _update_with_hessian(H, g):
    """math::get_update_with_hessian (oracle_lm.c orc_update_with_hessian_order, order 0): the diagonal
    shortcut, else Cholesky and the two substitutions, every sum taken in index order"""
    n = g.size
    off = H.copy()
    np.fill_diagonal(off, 0.0)
    if not np.any(off > THR):
        return g / np.diag(H)
    L = H.copy()
    for i in range(n):
        for j in range(i):
            s = 0.0
            for k in range(j):
                s += L[i, k] * L[j, k]
            L[i, j] = 1.0 / L[j, j] * (L[i, j] - s)
        s = 0.0
        for k in range(i):
            s += L[i, k] * L[i, k]
        L[i, i] = np.sqrt(L[i, i] - s)
    u = np.zeros(n)
    for i in range(n):
        s = 0.0
        for j in range(i):
            s += L[i, j] * u[j]
        u[i] = (g[i] - s) / L[i, i]
    for i in range(n - 1, -1, -1):
        s = 0.0
        for j in range(i + 1, n):
            s += L[j, i] * u[j]
        u[i] = (u[i] - s) / L[i, i]
    return u


def _gn_all(A, y, x, value, slope):
    """f = sum r^2, g = 2 J^T r, H = 2 J^T J (gn_all, order 0): sums over the rows in row order"""
    m, n = A.shape
    z = np.zeros(m)
    for j in range(n):
        z += A[:, j] * x[j]
    v = value(z)
    r = y - v
    J = -(slope(z, v)[:, None] * A)
    f, g, H = 0.0, np.zeros(n), np.zeros((n, n))
    for i in range(m):
        f += r[i] * r[i]
        g += J[i] * r[i]
        H += np.outer(J[i], J[i])
    return f, 2 * g, 2 * H


def lm_link_solve(A, y, x0, value, slope, *, lam=10.0, up=10.0, down=10.0, max_iter=100, f_delta=1e-12,
                  update=None):
    """orc_lm_solve with solver 0, order 0, on r = y - value(A x); value(z) and slope(z, v) take and
    return numpy vectors. Returns (f, iterations, x, final lambda). update: the solve, by default
    _update_with_hessian."""
    update = update or _update_with_hessian
    x = np.array(x0, dtype=np.float64)
    n = x.size
    cur, g, H = _gn_all(A, y, x, value, slope)
    prev, it = 0.0, 0
    while not (it >= max_iter or abs(prev - cur) < f_delta or np.isnan(prev)):
        H[np.arange(n), np.arange(n)] += lam
        x = x - update(H, g)
        prev = cur
        cur, g, H = _gn_all(A, y, x, value, slope)
        it += 1
        lam = lam / down if cur < prev else lam * up
    return cur, it, x, lam


# ---- links ------------------------------------------------------------------------------------------------
_libm_tanh = np.frompyfunc(math.tanh, 1, 1)


def tanh_link():
    """libm's tanh (math.tanh), the function the reference run calls — numpy's own may differ in the last bit"""
    return (lambda z: _libm_tanh(z).astype(np.float64)), (lambda z, v: 1 - v * v)


def identity_link():
    return (lambda z: z), (lambda z, v: np.ones_like(z))


def run(A, y, *, lam, max_iter, f_delta=0.0, link=None, update=None, x0=None):
    """The restatement from theta0 = 0 with up 4, down 2: (theta, f, iterations, calls, lambda). A sum that
    meets NaN, inf, a zero or a negative pivot goes on as IEEE says, silently."""
    value, slope = link or tanh_link()
    x0 = np.zeros(A.shape[1]) if x0 is None else x0
    with np.errstate(all="ignore"):
        f, it, x, lam = lm_link_solve(A, y, x0, value, slope, lam=lam, up=UP, down=DOWN,
                                      max_iter=max_iter, f_delta=f_delta, update=update)
    return x, float(f), it, it + 1, float(lam)


def update_with_hessian_rows(H, g):
    """_update_with_hessian with the k-sums of a whole column taken at once: cumsum adds strictly left to
    right, starting from the 0.0 put in front, so every element sees the serial loop's roundings"""
    n = g.size
    off = H.copy()
    np.fill_diagonal(off, 0.0)
    if not np.any(off > THR):
        return g / np.diag(H)

    def seq(P):  # row-wise sequential sums of P's columns
        return np.cumsum(np.concatenate([np.zeros((P.shape[0], 1)), P], axis=1), axis=1)[:, -1]

    L = H.copy()
    for j in range(n):   # column j: its diagonal first (row j's last element), then the rows below
        L[j, j] = np.sqrt(L[j, j] - seq(L[j:j + 1, :j] * L[j:j + 1, :j])[0])
        if j + 1 < n:
            L[j + 1:, j] = 1.0 / L[j, j] * (L[j + 1:, j] - seq(L[j + 1:, :j] * L[j, :j]))
    u = np.zeros(n)
    for i in range(n):
        u[i] = (g[i] - seq(L[i:i + 1, :i] * u[None, :i])[0]) / L[i, i]
    for i in range(n - 1, -1, -1):
        u[i] = (u[i] - seq(L[None, i + 1:, i] * u[None, i + 1:])[0]) / L[i, i]
    return u


# ---- exact pieces -------------------------------------------------------------------------------------------
def gn_at_zero(A, y):
    """(f, g, H) at theta = 0 for a link with phi(0) = 0, phi'(0) = 1 and finite A, y: _gn_all's sums, zero
    terms left out"""
    m, n = A.shape
    f, g, H = 0.0, np.zeros(n), np.zeros((n, n))
    for i in range(m):
        f += y[i] * y[i]
        idx = np.flatnonzero(A[i])
        if idx.size:
            Ji = -A[i, idx]
            g[idx] += Ji * y[i]
            H[np.ix_(idx, idx)] += np.outer(Ji, Ji)
    return f, 2 * g, 2 * H


def damped(H, lam):
    Hd = H.copy()
    n = H.shape[0]
    Hd[np.arange(n), np.arange(n)] += lam
    return Hd


def takes_shortcut(Hd):
    off = Hd.copy()
    np.fill_diagonal(off, 0.0)
    return not np.any(off > THR)


def fraction_solve(Hd, g):
    """x with Hd x = g exactly (Hd, g float64, read as the rationals they are), as a list of Fractions;
    Gaussian elimination without pivoting inside each connected component of Hd's sparsity"""
    n = g.size
    comp = list(range(n))

    def find(a):
        while comp[a] != a:
            comp[a] = comp[comp[a]]
            a = comp[a]
        return a

    for i, j in zip(*np.nonzero(Hd)):
        if i != j:
            comp[find(int(i))] = find(int(j))
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    x = [Fraction(0)] * n
    for idx in groups.values():
        k = len(idx)
        M = [[Fraction(float(Hd[a, b])) for b in idx] + [Fraction(float(g[a]))] for a in idx]
        for c in range(k):
            p = next(r for r in range(c, k) if M[r][c] != 0)
            M[c], M[p] = M[p], M[c]
            for r in range(c + 1, k):
                if M[r][c] != 0:
                    w = M[r][c] / M[c][c]
                    M[r] = [a - w * b for a, b in zip(M[r], M[c])]
        for c in range(k - 1, -1, -1):
            s = M[c][k] - sum(M[c][d] * x[idx[d]] for d in range(c + 1, k))
            x[idx[c]] = s / M[c][c]
    return x


def rounded(fr):
    """each Fraction rounded once to float64 (int / int is correctly rounded)"""
    return np.array([v.numerator / v.denominator for v in fr])


def first_step(A, y, lam):
    """theta after one step from 0, and whether the reference takes the shortcut: -(g / diag) by one
    division per coordinate, else minus the Fraction solution rounded once"""
    _, g, H = gn_at_zero(A, y)
    Hd = damped(H, lam)
    if takes_shortcut(Hd):
        with np.errstate(all="ignore"):
            return 0.0 - g / np.diag(Hd), True
    return 0.0 - rounded(fraction_solve(Hd, g)), False


def f_after(A, y, theta, link=None):
    """_gn_all's f at theta (z column by column, r^2 summed in row order)"""
    value, _ = link or tanh_link()
    z = np.zeros(A.shape[0])
    with np.errstate(all="ignore"):
        for j in np.flatnonzero(np.any(A != 0, axis=0) | ~np.isfinite(theta)):
            z += A[:, j] * theta[j]
        r = y - value(z)
        f = 0.0
        for v in r:
            f += v * v
    return float(f)


def f_bound(f, m):
    """How far a correct sum of m squared residuals r = y - tanh(z) may lie from f_after's: two correct
    tanh differ by at most an ulp of a value <= 1 each (2^-52 absolute on r, and |r| >= 0.238 wherever an
    integer y is not 0: 8.4 eps on r^2), and m non-negative terms summed in any order, fused or not, add
    m eps — relative to f, rounded up to (m + 16) eps."""
    return (m + 16) * EPS * f


def pad_rows(A, y, m):
    """zero rows of A with y = 0 up to m rows: they add an exact 0 to every sum"""
    k = m - A.shape[0]
    assert k >= 0
    return np.vstack([A, np.zeros((k, A.shape[1]))]), np.concatenate([y, np.zeros(k)])


# ---- the constructions --------------------------------------------------------------------------------------
def exact_dense(n, rng, band=None):
    """(A (2n, n), y, u): R upper triangular (band: nothing past that many superdiagonals), off-diagonals in
    {-1, 0, 1}, diagonal in {1, 2, 4}, R[0][1] = 1;
    A = [R; R], y = [-R u; -R u] with integer u in [-3, 3]. With lambda0 = 0, H = (2R)^T (2R): the Cholesky
    factor is 2 R^T, the pivots are perfect squares with power-of-two roots, both substitutions stay in
    integers, and theta after one step is -u for every correct implementation."""
    assert n >= 2
    R = np.triu(rng.integers(-1, 2, (n, n)), 1).astype(np.float64)
    if band is not None:
        R = np.tril(R, band)
    R[0, 1] = 1.0
    R[np.arange(n), np.arange(n)] = 2.0 ** rng.integers(0, 3, n)
    u = rng.integers(-3, 4, n).astype(np.float64)
    A = np.vstack([R, R])
    y = np.concatenate([-(R @ u), -(R @ u)])
    Hi = 2 * (A.T @ A)   # small integers: exact in float64 whatever the order of the sums
    assert np.any(Hi[~np.eye(n, dtype=bool)] > 0), "H has a positive off-diagonal"
    assert np.max(np.abs(Hi)) * 3 * n < 2.0 ** 53 and np.array_equal(Hi @ u, -2 * (A.T @ y))   # H u = g
    return A, y, u


def planted(n, i, j, c):
    """(A (n + 1, n), y): A = [I_n; e_i + c e_j], y = 1 .. n + 1. H[i][j] = H[j][i] = 2c exactly and every
    other off-diagonal is 0."""
    assert i != j
    A = np.vstack([np.eye(n), np.zeros((1, n))])
    A[n, i], A[n, j] = 1.0, c
    return A, np.arange(1.0, n + 2)


def planted_values():
    """the four c of a position: at the threshold (shortcut), one ulp above (dense), -1 (shortcut although
    far from diagonal), 1 (plainly dense)"""
    at = THR / 2
    above = float(np.nextafter(at, 1.0))
    assert 2 * at == THR and 2 * above > THR
    return (at, True), (above, False), (-1.0, True), (1.0, False)


def _with_transposes(pos, n):
    pos = sorted(p for p in pos if p[0] != p[1] and 0 <= p[1] < p[0] < n)
    return pos + [(j, i) for i, j in pos]


def planted_positions(n):
    """(i, j) below the diagonal, and their transposes: the corners, both sides of EVERY 16-column edge the
    width has (the 64-column and 128-column edges are among them), and positions in off-diagonal
    super-blocks (or, up to 128 columns, in the last column block's first column)"""
    pos = {(1, 0), (n - 1, 0), (n - 1, n - 2)}
    for e in range(16, n, 16):
        pos.add((e, e - 1))          # the edge between column e - 1 and column e
        if e + 1 < n:
            pos.add((e + 1, e))      # the first pair past it
    if n > 128:
        pos.add((n - 1, 128))
        if n > 256:
            pos.add((n - 44, 5))
    elif n > 16:
        pos.add((n - 1, 16))
    return _with_transposes(pos, n)


def planted_positions_few(n):
    """the part of planted_positions that the CPU file can afford to run the whole restatement and the
    oracle on past 144 columns: corners, the first and the last edge of each kind, the super-block ones"""
    pos = {(1, 0), (n - 1, 0), (n - 1, n - 2)}
    for w in (16, 64, 128, 256, 512):
        for e in {w, (n - 1) // w * w}:
            if w <= e < n:
                pos.add((e, e - 1))
                if e + 1 < n:
                    pos.add((e + 1, e))
    if n > 128:
        pos.add((n - 1, 128))
        if n > 256:
            pos.add((n - 44, 5))
    elif n > 16:
        pos.add((n - 1, 16))
    few = _with_transposes(pos, n)
    assert set(few) <= set(planted_positions(n))
    return few


def planted_step(n, i, j, c, lam):
    """first_step(*planted(n, i, j, c), lam) in O(n), and the shortcut's answer: (theta, shortcut, theta by
    the shortcut). H is diagonal but for H[i][j] = H[j][i] = 2c; its sums have at most two non-zero terms:
    row k's, then the last row's, each product rounded before it is added (gn_at_zero's order)."""
    y = np.arange(1.0, n + 2)
    d = np.full(n, 2.0)
    d[i] = 2 * (1.0 + 1.0)
    d[j] = 2 * (1.0 + c * c)
    g = 2 * (-y[:n])
    g[i] = 2 * (-y[i] + (-1.0) * y[n])
    g[j] = 2 * (-y[j] + (-c) * y[n])
    d = d + lam
    short = 0.0 - g / d
    if not 2 * c > THR:
        return short, True, short
    Hd = np.array([[d[i], 2 * c], [2 * c, d[j]]])
    xi, xj = rounded(fraction_solve(Hd, np.array([g[i], g[j]])))
    theta = short.copy()
    theta[i], theta[j] = 0.0 - xi, 0.0 - xj
    return theta, False, short


def all_negative(n):
    """(A (2n, n), y): R = 2I - superdiagonal, A = [R; R]. H = 4 R^T R has -8 on the first off-diagonals and
    0 elsewhere off the diagonal: dense, yet is_diagonal calls it diagonal and the reference answers g / diag."""
    R = 2.0 * np.eye(n) - np.eye(n, k=1)
    A = np.vstack([R, R])
    y = np.tile(np.arange(1.0, n + 1), 2)
    Hi = 2 * (A.T @ A)
    assert np.all(Hi[~np.eye(n, dtype=bool)] <= 0) and Hi[0, 1] == -8
    return A, y


HOSTILE = ("zero_pivot", "negative_pivot", "zero_column", "nan_y", "inf_y", "orthogonal_y", "f_rises")
_SQ = (2507, 77, 21, 6)   # 2507^2 + 77^2 + 21^2 + 6^2 = 2^22 + 2^21 - 1
assert sum(v * v for v in _SQ) == 2 ** 22 + 2 ** 21 - 1


def hostile(kind, n, last):
    """(A, y, lambda0): a 2 x 2 hostile core in columns (p, q) = (0, 1) or, `last`, (n - 2, n - 1) of an
    otherwise identity A.

      zero_pivot      columns p and q equal, lambda0 = 0: H's core is [[4, 4], [4, 4]], the second pivot 0
      negative_pivot  the same with lambda0 = -8: every pivot is negative
      zero_column     column p zero, lambda0 = 0, H diagonal: the shortcut divides 0 / 0 at p alone
      nan_y, inf_y    row p = e_p + e_q (a dense core), y[p] NaN or +inf, lambda0 = 1
      orthogonal_y    a further row e_p + e_q, y = e_p + e_q - e_last: A^T y = 0, y != 0, lambda0 = 1
      f_rises         lambda0 = 2^-20 - 2 against H = 2 on the plain coordinates: pivots of 2^-20. The core is
                      [[1, 2^-11], [0, 2507 / 2^11]] and three more rows 77, 21, 6 / 2^11 in column q, so
                      that H's core is [[2, 2^-10], [2^-10, 3]] and the damped core [[2^-20, 2^-10],
                      [2^-10, 1 + 2^-20]] = L L^T with L = [[2^-10, 0], [1, 2^-10]]: every number of the
                      solve is dyadic and exact. y = 0.25 e_p sends theta_p to about 2^39 and theta_q to
                      about -2^29, the tanh of six rows saturates, and f goes from 0.0625 to 4.5625."""
    p = n - 2 if last else 0
    q = p + 1
    A, y, lam = np.eye(n), np.arange(1.0, n + 1), 1.0
    if kind in ("zero_pivot", "negative_pivot"):
        A[p, q] = A[q, p] = 1.0
        lam = 0.0 if kind == "zero_pivot" else -8.0
    elif kind == "zero_column":
        A[p, p], lam = 0.0, 0.0
    elif kind in ("nan_y", "inf_y"):
        A[p, q] = 1.0
        y[p] = np.nan if kind == "nan_y" else np.inf
    elif kind == "orthogonal_y":
        A = np.vstack([A, np.zeros((1, n))])
        A[n, p] = A[n, q] = 1.0
        y = np.zeros(n + 1)
        y[p], y[q], y[n] = 1.0, 1.0, -1.0
        assert not np.any(A.T @ y)
    elif kind == "f_rises":
        A = np.vstack([A, np.zeros((3, n))])
        A[p, q] = 2.0 ** -11
        A[q, q] = _SQ[0] / 2.0 ** 11
        for k in range(3):
            A[n + k, q] = _SQ[k + 1] / 2.0 ** 11
        y = np.zeros(n + 3)
        y[p] = 0.25
        lam = 2.0 ** -20 - 2.0
    else:
        raise ValueError(kind)
    return A, y, lam


def banded(n):
    """(A (n, n), y): A = I + superdiagonal, so H = 2 A^T A is tridiagonal with a positive off-diagonal. The
    Givens sweep of tinyqr meets pairs of zeros below the band and divides 0 / 0: the reference returns NaN."""
    return np.eye(n) + np.eye(n, k=1), np.arange(1.0, n + 1)


def dense_qr(n, rng):
    """(A (n + 2, n), y): small integers without a zero, on top of 8 I: every pair a Givens rotation meets in
    H + lambda I is non-zero (cond 2.4 at n = 3 to 2139 at n = 64)"""
    A = rng.integers(1, 4, (n + 2, n)).astype(np.float64) * rng.choice([-1.0, 1.0], (n + 2, n))
    A[:n] += 8.0 * np.eye(n)
    return A, rng.integers(1, 6, n + 2).astype(np.float64)


def stop_rule_cases(f0):
    """(max_iter, f_delta, iterations) of a run whose f0 is finite and whose first step changes f: the test
    is iter >= max_iter || |prev - cur| < f_delta || isnan(prev) with prev = 0 before the first step, so
    f_delta = f0 still runs (strict <), one ulp more does not, inf never runs, NaN never stops"""
    return ((0, 0.0, 0), (1, f0, 1), (1, float(np.nextafter(f0, np.inf)), 0), (1, np.inf, 0), (1, np.nan, 1))


# ---- what both test files use -------------------------------------------------------------------------------
WIDTHS = (2, 3, 16, 17, 63, 64, 65, 80, 127, 128, 129, 144, 255, 256, 257, 300, 513, 1024)
HOSTILE_WIDTHS = (2, 17, 64, 65, 128, 129, 257)
EDGE_WIDTHS = (3, 64, 65, 129, 257)
QR_WIDTHS = (3, 17, 33, 64)
PLANTED_REL_ERR = 4.1e-16   # measured: tests/test_lm_planted_cpu.py test_planted_entry_decides_the_branch

# iteration, calls, lambda after max_iter = 1 and max_iter = 5, from the loop by hand (up 4, down 2):
#   f0 NaN: one step, then isnan(prev) stops.  f0 finite or inf and f NaN from the first step on: the
#   second step is still taken (prev is not NaN, |prev - NaN| < 0 is false), both take `up`.
#   A^T y = 0: cur == prev for ever, `up` every time.  f_rises: `up` once, then cur == prev.
DERIVED = {
    "zero_pivot": ((1, 2, 0.0), (2, 3, 0.0)),
    "negative_pivot": ((1, 2, -32.0), (2, 3, -128.0)),
    "zero_column": ((1, 2, 0.0), (2, 3, 0.0)),
    "nan_y": ((1, 2, 4.0), (1, 2, 4.0)),
    "inf_y": ((1, 2, 4.0), (2, 3, 16.0)),
    "orthogonal_y": ((1, 2, 4.0), (5, 6, 1024.0)),
    "f_rises": ((1, 2, (2.0 ** -20 - 2.0) * 4), (5, 6, (2.0 ** -20 - 2.0) * 1024)),
}


def seeded(n):
    return np.random.default_rng(1000 + n)


def solver_for(n):
    """the triple loop up to 17 columns, its column-at-once twin beyond (proved equal on the CPU)"""
    return None if n <= 17 else update_with_hessian_rows


def qr_reference(A, y, lam):
    """(theta after one exact step, cond of the damped matrix)"""
    _, g, H = gn_at_zero(A, y)
    Hd = damped(H, lam)
    return 0.0 - rounded(fraction_solve(Hd, g)), float(np.linalg.cond(Hd))


def sparse_first_step(A, y, lam, update=update_with_hessian_rows):
    """run(A, y, lam=lam, max_iter=1) for finite data with the evaluations' zero terms left out (gn_at_zero,
    f_after): what the CPU file runs where _gn_all's m n^2 work takes too long"""
    f0, g, H = gn_at_zero(A, y)
    with np.errstate(all="ignore"):
        theta = 0.0 - update(damped(H, lam), g)
    f = f_after(A, y, theta)
    return theta, f, 1, 2, float(lam / DOWN if f < f0 else lam * UP)
