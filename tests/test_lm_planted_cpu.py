"""The references of tests/test_lm_planted_gpu.py, proved without a GPU: for every construction of
tests/_lm_planted.py at the widths the device file uses,

  * the serial restatement gives the Fraction solution rounded once (exact_dense: -u bit for bit);
  * oracle_lm.c in order 0 gives the restatement's theta, f, iteration, function calls and final lambda bit
    for bit (NaN equal to NaN, the signs of inf included); order 1 gives the same but for f after a step on
    tanh data (below);
  * the threshold pair flips is_diagonal at one ulp;
  * the counters the loop must leave on hostile values are the ones derived from nlsolver.h:3513-3543 by
    hand (up 4, down 2), written out as literals in _lm_planted.DERIVED.

Measured here, and held by the tests below so that the figures cannot go stale:

  * f after a step on tanh data: order 1 (the kernels' tanh and summation order) differs from order 0 and the
    restatement by up to 3 ulp (n = 65: 19153.002404100287 against ...305) — theta, the counters and lambda
    are identical. Order 1's f is therefore compared bit for bit only where it is exact (f0, NaN, 0, the
    dyadic cases), and within _lm_planted.f_bound, (m + 16) eps f with m the rows of the case at hand, after
    a step on tanh data; it lies within 0.04 of that bound.
  * dense planted cases, restatement against the Fraction solution, max |x - ref| / max |ref|: 4.06e-16
    (PLANTED_REL_ERR = 4.1e-16) over every position up to 144 columns, the corners, first and last edges of
    each kind and super-block positions up to 513, three positions at 1024. The O(n) Fraction reference
    itself is checked at every position of every width. The device is held to 8 times the figure; the
    smallest gap between the shortcut's answer and the dense one at (i, j), relative to max |ref|, is
    1.2e-7 at n = 300 and 3.5e-8 at n = 1024: the bound is below 1e-7 of it (the condition is 1e-3).
  * QR on dense_qr systems (cond(H + lambda I) = 2.4, 56, 567, 2139 at n = 3, 17, 33, 64) and on the banded
    system at n = 3: both oracle orders lie within 0.05 of the bound 8 cond eps max |ref| that
    tests/test_tinyqr_gpu.py holds tinyqr to."""
import numpy as np
import pytest

from tests import _lm_planted as P
from tests import _oracle as O

from tests._lm_planted import (DERIVED, EDGE_WIDTHS, HOSTILE_WIDTHS, PLANTED_REL_ERR, QR_WIDTHS,  # noqa: E402
                                 WIDTHS, qr_reference, seeded, solver_for)

FULL_MAX = 144   # up to here every planted position goes through the whole restatement and both oracle orders


def orc(lib, A, y, lam, max_iter, order, f_delta=0.0, solver=0):
    st, x, lam_out, _ = O.lm_solve(lib, A, y, np.zeros(A.shape[1]), lam=lam, up=P.UP, down=P.DOWN,
                                   max_iter=max_iter, f_delta=f_delta, order=order, solver=solver)
    return x, st.f_value, st.iteration, st.function_calls_used, lam_out


def same(a, b, m=None):
    """theta, iteration, calls, lambda and f bit for bit (NaN equal to NaN); with m — the order-1 oracle
    after a step on tanh data of m rows — f within f_bound(f, m) instead"""
    ok = np.array_equal(a[0], b[0], equal_nan=True) and a[2:4] == b[2:4]
    ok = ok and np.array_equal(a[4], b[4], equal_nan=True)
    if m is None or (np.isnan(a[1]) and np.isnan(b[1])):
        return ok and np.array_equal(a[1], b[1], equal_nan=True)
    return ok and abs(a[1] - b[1]) <= P.f_bound(a[1], m)


def same_both_orders(oracle, r, A, y, lam, max_iter, tag, f_delta=0.0, stepped=True):
    """order 0 is the restatement bit for bit, f included; order 1 too, but for f after a step on tanh data"""
    m = A.shape[0]
    assert same(r, orc(oracle, A, y, lam, max_iter, 0, f_delta=f_delta)), (tag, 0)
    assert same(r, orc(oracle, A, y, lam, max_iter, 1, f_delta=f_delta), m=m if stepped else None), (tag, 1)


# ---- the reference's own parts ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 16, 17, 33, 65])
def test_the_column_at_once_solve_is_the_serial_one(n):
    cases = [P.exact_dense(n, seeded(n))[:2] + (0.0,), P.planted(n, n - 1, 0, 1.0) + (1.0,),
             P.planted(n, 0, 1, float(np.nextafter(P.THR / 2, 1.0))) + (1.0,), P.all_negative(n) + (0.5,)]
    cases += [P.hostile(kind, n, last) for kind in P.HOSTILE for last in (False, True)]
    rng = seeded(n)
    B = rng.uniform(-1, 1, (n + 3, n))
    cases.append((B, rng.uniform(-1, 1, n + 3), 0.25))
    for A, y, lam in cases:
        with np.errstate(all="ignore"):
            f, g, H = P._gn_all(A, y, np.zeros(n), *P.tanh_link())
        if np.all(np.isfinite(y)):   # (a NaN or inf in y reaches every sum through its zero terms too)
            f2, g2, H2 = P.gn_at_zero(A, y)
            assert f == f2 and np.array_equal(g, g2) and np.array_equal(H, H2)
        Hd = P.damped(H, lam)
        with np.errstate(all="ignore"):
            a, b = P._update_with_hessian(Hd.copy(), g), P.update_with_hessian_rows(Hd.copy(), g)
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("n", [2, 5, 17])
def test_the_verdict_reads_every_row_of_both_triangles(oracle, n):
    """A Gauss-Newton H is symmetric, so a verdict that skipped a row would still meet its entry in the
    mirror column: here one entry stands in one triangle only — in the last row, in the last column, in
    the first column — and the restatement must decide, and solve, as the oracle's literal is_diagonal does"""
    g = np.arange(1.0, n + 1)
    for i, j in ((n - 1, 0), (0, n - 1), (1, 0)):
        for v, dense in ((1.0, True), (float(np.nextafter(P.THR, 1.0)), True), (P.THR, False), (-1.0, False)):
            H = np.diag(np.arange(3.0, n + 3))
            H[i, j] = v
            assert P.takes_shortcut(H) == (not dense)
            want = np.zeros(n)
            Hc = H.copy()
            oracle.orc_update_with_hessian(O._ptr(want), O._ptr(Hc), O._ptr(g), n)
            for solve in (P._update_with_hessian, P.update_with_hessian_rows):
                assert np.array_equal(solve(H.copy(), g), want), (n, i, j, v, solve.__name__)
            if i > j:   # the factorisation reads the lower triangle: there the entry changes the answer
                assert np.array_equal(want, g / np.diag(H)) == (not dense)


def test_fraction_solve_is_exact():
    rng = seeded(7)
    M = rng.integers(-3, 4, (9, 6)).astype(np.float64)
    H = 2 * M.T @ M + np.eye(6)
    x = rng.integers(-5, 6, 6).astype(np.float64)
    assert [int(v) for v in P.fraction_solve(H, H @ x)] == x.tolist()
    H[0, 1:] = H[1:, 0] = 0.0   # two components
    assert np.array_equal(P.rounded(P.fraction_solve(H, H @ x)), x)


# ---- exact_dense ------------------------------------------------------------------------------------------
def restated(n, A, y, lam):
    """the restatement's first step: the whole loop up to 300 columns, its zero-skipping evaluations beyond"""
    if n <= 300:
        return P.run(A, y, lam=lam, max_iter=1, update=solver_for(n))
    return P.sparse_first_step(A, y, lam)


@pytest.mark.parametrize("n", WIDTHS)
def test_exact_dense_first_step_is_minus_u(oracle, n):
    A, y, u = P.exact_dense(n, seeded(n))   # (asserts H u = g in integers)
    R2 = 2 * A[:n]
    assert np.array_equal(R2.T @ R2, 2 * (A.T @ A))   # H = (2R)^T (2R), in integers
    assert np.all(np.isin(np.diag(R2), (2, 4, 8))) and not np.any(np.tril(R2, -1))
    if n <= 300:
        f0, g, H = P.gn_at_zero(A, y)
        assert f0 == float(np.sum(y.astype(np.int64) ** 2)) and not P.takes_shortcut(H)
        assert np.array_equal(H, 2.0 * (A.T @ A)) and np.array_equal(g, -2.0 * (A.T @ y))   # integers: any order
        if n <= 33:
            assert np.array_equal(P.rounded(P.fraction_solve(H, g)), u)
            assert np.array_equal(P.first_step(A, y, 0.0)[0], -u)
    r = restated(n, A, y, 0.0)
    assert np.array_equal(r[0], -u) and r[2:] == (1, 2, 0.0) and r[1] == P.f_after(A, y, -u)
    same_both_orders(oracle, r, A, y, 0.0, 1, n)
    o = orc(oracle, A, y, 0.0, 1, 1)
    print(f"n {n} order 1: f {o[1]!r} restatement {r[1]!r}, "
          f"{abs(o[1] - r[1]) / P.f_bound(r[1], 2 * n):.3f} of the bound")


# ---- planted ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", WIDTHS)
def test_planted_entry_decides_the_branch(oracle, n):
    """Every position: the threshold pair flips, the O(n) reference is the generic one, the bound sits below
    1e-3 of the gap. The whole restatement and both oracle orders: every position up to 144 columns, the
    corners, first and last edges and super-block positions up to 513, three positions at 1024."""
    positions = P.planted_positions(n)
    assert len(set(positions)) == len(positions) and all(0 <= i < n and 0 <= j < n and i != j for i, j in positions)
    assert all(p in positions for e in range(16, n, 16) for p in ((e, e - 1), (e - 1, e)))
    heavy = positions if n <= FULL_MAX else P.planted_positions_few(n) if n <= 513 \
        else [(1, 0), (n - 1, n - 2), (n - 1, 128)]
    worst, gap = 0.0, np.inf
    for i, j in positions:
        for c, shortcut in P.planted_values():
            ref, sc, short = P.planted_step(n, i, j, c, 1.0)
            assert sc == shortcut and (2 * c == P.THR, 2 * c > P.THR) == ((c == P.THR / 2), not shortcut)
            if shortcut:
                assert np.array_equal(ref, short)
            else:
                scale = np.max(np.abs(ref))
                others = np.ones(n, dtype=bool)
                others[[i, j]] = False
                assert np.array_equal(ref[others], short[others])   # one division each, either way
                gap = min(gap, min(abs(short[i] - ref[i]), abs(short[j] - ref[j])) / scale)
            if (i, j) not in heavy:
                continue
            A, y = P.planted(n, i, j, c)
            _, g, H = P.gn_at_zero(A, y)
            assert H[i, j] == H[j, i] == 2 * c and np.count_nonzero(H - np.diag(np.diag(H))) == 2
            generic, sc = P.first_step(A, y, 1.0)
            assert sc == shortcut and np.array_equal(generic, ref)
            r = restated(n, A, y, 1.0)
            assert r[2:4] == (1, 2) and r[4] in (0.5, 4.0)
            if shortcut:
                assert np.array_equal(r[0], ref)
            else:
                worst = max(worst, np.max(np.abs(r[0] - ref)) / scale)
            same_both_orders(oracle, r, A, y, 1.0, 1, (n, i, j, c))
    print(f"n {n}: {len(positions)} positions ({len(heavy)} through restatement and oracle), restatement within "
          f"{worst:.3e} of the Fraction solution, smallest gap between the branches {gap:.3e} "
          f"(both relative to max |theta|)")
    assert worst <= PLANTED_REL_ERR
    assert 8 * PLANTED_REL_ERR < 1e-3 * gap


# ---- all negative -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", WIDTHS)
def test_all_negative_off_diagonals_take_the_shortcut(oracle, n):
    A, y = P.all_negative(n)
    _, g, H = P.gn_at_zero(A, y)
    assert np.array_equal(H, 2.0 * (A.T @ A)) and H[1, 0] == -8 and P.takes_shortcut(P.damped(H, 1.0))
    ref, sc = P.first_step(A, y, 1.0)
    assert sc and np.array_equal(ref, 0.0 - g / (np.diag(H) + 1.0))
    true = 0.0 - np.linalg.solve(P.damped(H, 1.0), g)
    assert np.max(np.abs(true - ref)) > 0.1   # the shortcut's answer is not the solve's
    r = restated(n, A, y, 1.0)
    assert np.array_equal(r[0], ref)
    same_both_orders(oracle, r, A, y, 1.0, 1, n)


# ---- hostile ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", HOSTILE_WIDTHS)
@pytest.mark.parametrize("kind", P.HOSTILE)
def test_hostile_values_follow_the_loop(oracle, n, kind):
    for last in (False, True):
        A, y, lam = P.hostile(kind, n, last)
        p = n - 2 if last else 0
        for k, want in zip((1, 5), DERIVED[kind]):
            r = P.run(A, y, lam=lam, max_iter=k, update=solver_for(n))
            assert r[2:] == want, (kind, n, last, k, r[2:])
            for order in (0, 1):
                assert same(r, orc(oracle, A, y, lam, k, order)), (kind, n, last, k, order)
            theta, f = r[0], r[1]
            if kind == "zero_column" and k == 1:
                assert np.flatnonzero(np.isnan(theta)).tolist() == [p]
            elif kind == "orthogonal_y":
                assert not np.any(theta) and f == 3.0
            elif kind == "f_rises":
                assert f == 4.5625 and P.gn_at_zero(A, y)[0] == 0.0625   # the rise is gross
                assert theta[p] > 2.0 ** 39 and theta[p + 1] < -2.0 ** 28
                assert not np.any(np.delete(theta, [p, p + 1]))
            else:
                assert np.isnan(f)
            if kind in ("zero_pivot", "negative_pivot", "nan_y", "inf_y"):
                assert not np.any(np.isfinite(theta[[p, p + 1]]))


# ---- the stop rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_WIDTHS)
def test_stop_rule_edges(oracle, n):
    A, y, u = P.exact_dense(n, seeded(n))
    f0 = P.gn_at_zero(A, y)[0]
    assert f0 == float(int(f0)) and f0 > 0
    for max_iter, f_delta, iters in P.stop_rule_cases(f0) + ((3, np.nan, 3),):
        r = P.run(A, y, lam=0.0, max_iter=max_iter, f_delta=f_delta, update=solver_for(n))
        assert r[2:4] == (iters, iters + 1) and r[4] == 0.0, (n, max_iter, f_delta)
        if iters == 0:
            assert not np.any(r[0]) and r[1] == f0
        elif iters == 1:
            assert np.array_equal(r[0], -u)
        if iters <= 1:
            same_both_orders(oracle, r, A, y, 0.0, max_iter, (n, max_iter, f_delta), f_delta=f_delta,
                             stepped=iters == 1)
        else:   # (past the first step H is singular where tanh saturates: only the counters are defined)
            for order in (0, 1):
                assert orc(oracle, A, y, 0.0, max_iter, order, f_delta=f_delta)[2:4] == r[2:4], (n, order)


# ---- the identity link ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_WIDTHS)
def test_identity_link_whole_run(n):
    A, y, u = P.exact_dense(n, seeded(n))
    theta, f, it, calls, lam = P.run(A, y, lam=0.0, max_iter=6, link=P.identity_link(), update=solver_for(n))
    assert np.array_equal(theta, -u) and f == 0.0 and (it, calls, lam) == (6, 7, 0.0)


# ---- QR -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", QR_WIDTHS)
def test_qr_step_references(oracle, n):
    A, y = P.banded(n)
    for order in (0, 1):
        theta, f, it, calls, lam = orc(oracle, A, y, 1.0, 1, order, solver=1)
        if n >= 17:
            assert np.all(np.isnan(theta)) and np.isnan(f) and (it, calls, lam) == (1, 2, 4.0), (n, order)
        else:   # no rotation of the sweep meets a pair of zeros: the bound of the dense systems holds
            ref, cond = qr_reference(A, y, 1.0)
            bound = 8 * cond * P.EPS * np.max(np.abs(ref))
            err = np.max(np.abs(theta - ref))
            print(f"n {n} banded, order {order}: cond {cond:.2f}, {err / bound:.3f} of the bound")
            assert err <= bound and (it, calls) == (1, 2), (n, order, err, bound)
    A, y = P.dense_qr(n, seeded(n))
    ref, cond = qr_reference(A, y, 1.0)
    bound = 8 * cond * P.EPS * np.max(np.abs(ref))
    for order in (0, 1):
        theta, f, it, calls, lam = orc(oracle, A, y, 1.0, 1, order, solver=1)
        err = np.max(np.abs(theta - ref))
        print(f"n {n} order {order}: cond {cond:.2f}, |theta - ref| {err:.3e}, {err / bound:.3f} of the bound")
        assert err <= bound and (it, calls) == (1, 2)
