"""The LM step kernels and the evaluations' is_diagonal verdict against references that owe nothing to
oracle_lm.c's order 1: the constructions of tests/_lm_planted.py (proved on the CPU, against both oracle
orders and fractions.Fraction, by tests/test_lm_planted_cpu.py), each one LMEngine call on a small batch,
up 4, down 2, from theta0 = 0.

Widths and routes (the environment is read when the engine is made):
  2, 3, 16, 17, 63, 64     lm_iter_kernel
  65, 80, 127, 128         default, NLSG_LM_WIDE_CHOL=0, NLSG_LM_WIDE_MFMA=0
  129, 144, 255, 256       the same three and NLSG_LM_WIDE256=0
  257, 300, 513, 1024      default, NLSG_LM_WIDE_CHOL=0, NLSG_LM_WIDE_MFMA=0

Exact cases assert bit equality: theta, iteration, function calls, done, lambda everywhere, and f wherever
it is exact by construction (integers, dyadic numbers, NaN, 0). After a step on tanh data f is a sum of
inexact squares: the oracle's order 1 (the kernels' tanh and summation order) differs there from order 0
and the restatement by up to 3 ulp, so the device's f is held to _lm_planted.f_bound, (m + 16) eps f, a bound
from the formats (measured: order 1 lies within 0.04 of it, the device within 0.08).

Tolerances measured on the CPU (tests/test_lm_planted_cpu.py asserts them):
  dense planted cases   the serial restatement lies within 4.06e-16 max |theta| of the Fraction solution over
                        the positions the CPU file runs it on (all up to 144 columns); the device is held
                        to 8 x 4.1e-16 max |theta| (measured: 0.13 of that). The smallest
                        gap between the shortcut's answer and the dense one at (i, j) is 3.5e-8 max |theta|
                        (n = 1024): the bound is 1e-7 of it, and the test asserts it below 1e-3 of the gap of
                        the case at hand.
  QR                    8 cond eps max |ref| as in tests/test_tinyqr_gpu.py, cond of H + lambda I at hand
                        (2.4, 56, 567, 2139 at n = 3, 17, 33, 64); oracle and device lie within 0.05 of it."""
import numpy as np
import pytest

from tests import _lm_planted as P
from tests._lm_planted import (DERIVED, EDGE_WIDTHS, HOSTILE_WIDTHS, PLANTED_REL_ERR, QR_WIDTHS, WIDTHS,
                               qr_reference, seeded, solver_for)

pytestmark = pytest.mark.gpu

ENV = ("NLSG_LM_WIDE_CHOL", "NLSG_LM_WIDE_MFMA", "NLSG_LM_WIDE256")
KW = dict(up=P.UP, down=P.DOWN)


def routes(n):
    if n <= 64:
        return ("default",)
    if 128 < n <= 256:
        return ("default",) + ENV
    return ("default",) + ENV[:2]


def width_routes(widths):
    return [pytest.param(n, r, id=f"{n}-{r}") for n in widths for r in routes(n)]


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available()
    import nlsolver_amd
    return nlsolver_amd


def solve(mod, monkeypatch, route, A, y, *, lam, max_iter, f_delta=0.0, model=None, solver=None):
    """one engine on the batch (A, y) under `route`, from theta0 = 0: (theta, status list, lambda)"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if route != "default":
        monkeypatch.setenv(route, "0")
    model = model or mod.TanhRegression(A, y)
    kw = dict(KW, lam=lam, max_iter=max_iter, f_delta=f_delta)
    if solver is not None:
        kw["solver"] = solver
    with mod.LMEngine(model, **kw) as eng:
        B, n = eng.cfg.batch, eng.cfg.n
        return eng.minimize(np.zeros((B, n)))


def counters(st):
    return st.iteration, st.function_calls_used, st.done


_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def stack(problems):
    """problems (A, y) of one width padded with zero rows to the tallest: (A [B, m, n], y [B, m])"""
    m = max(A.shape[0] for A, _ in problems)
    padded = [P.pad_rows(A, y, m) for A, y in problems]
    return np.stack([a for a, _ in padded]), np.stack([b for _, b in padded])


def ordinary(n):
    """two exact_dense problems of width n: (A, y, u) each"""
    return cached(("dense", n), lambda: [P.exact_dense(n, seeded(n + 5000 * k)) for k in (0, 1)])


# ---- exact_dense ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,route", width_routes(WIDTHS))
def test_exact_dense_first_step(mod, monkeypatch, n, route):
    """H = (2R)^T (2R), g = H u in integers: the factor is 2 R^T, every pivot a perfect square, both
    substitutions stay in integers, theta = -u whatever the order of the sums"""
    probs = ordinary(n)
    A, y = stack([(a, b) for a, b, _ in probs])
    want_f = cached(("dense_f", n), lambda: [P.f_after(a, b, -u) for a, b, u in probs])
    theta, st, lam = solve(mod, monkeypatch, route, A, y, lam=0.0, max_iter=1)
    for b, (_, yb, u) in enumerate(probs):
        assert np.array_equal(theta[b], -u), (n, route, b, np.flatnonzero(theta[b] != -u)[:8])
        assert counters(st[b]) == (1, 2, 1) and lam[b] == 0.0
        f0 = float(np.sum(yb * yb))
        print(f"n {n} {route} problem {b}: f {st[b].f_value!r}, restatement {want_f[b]!r}, "
              f"{abs(st[b].f_value - want_f[b]) / P.f_bound(want_f[b], yb.size):.3f} of the bound")
        assert want_f[b] < f0 and abs(st[b].f_value - want_f[b]) <= P.f_bound(want_f[b], yb.size)


# ---- one entry decides is_diagonal ------------------------------------------------------------------------
def planted_reference(n):
    """[(i, j, c, shortcut, theta, theta by the shortcut)] over every position and the four values"""
    out = []
    for i, j in P.planted_positions(n):
        for c, shortcut in P.planted_values():
            ref, sc, short = P.planted_step(n, i, j, c, 1.0)   # (held to first_step on the CPU)
            assert sc == shortcut
            out.append((i, j, c, shortcut, ref, short))
    return out


PLANTED_BATCH = 128   # problems per engine: at n = 1024 a gigabyte of design matrices


@pytest.mark.parametrize("n,route", width_routes(WIDTHS))
def test_single_entry_decides_is_diagonal(mod, monkeypatch, n, route):
    """A = [I; e_i + c e_j]: H[i][j] = H[j][i] = 2c is the only off-diagonal. c = thr / 2 and c = -1 take the
    shortcut (one correctly rounded division per coordinate: bit equality), c one ulp above thr / 2 and
    c = 1 the dense solve (the Fraction solution within 8 x 4.1e-16 max |theta|, a bound below 1e-3 of the
    distance to the shortcut's answer at i and j). Every position and value of the width, in batches of at
    most 128 problems."""
    ref = cached(("planted", n), lambda: planted_reference(n))
    theta, st, lam = [], [], []
    for b0 in range(0, len(ref), PLANTED_BATCH):
        part = ref[b0:b0 + PLANTED_BATCH]
        A = np.zeros((len(part), n + 1, n))
        A[:, np.arange(n), np.arange(n)] = 1.0
        for b, (i, j, c, *_) in enumerate(part):
            A[b, n, i], A[b, n, j] = 1.0, c
        y = np.tile(np.arange(1.0, n + 2), (len(part), 1))
        out = solve(mod, monkeypatch, route, A, y, lam=1.0, max_iter=1)
        theta.extend(out[0]), st.extend(out[1]), lam.extend(out[2])
    worst = 0.0
    for b, (i, j, c, shortcut, want, short) in enumerate(ref):
        tag = (n, route, i, j, c)
        assert counters(st[b]) == (1, 2, 1) and lam[b] in (0.5, 4.0), tag
        if shortcut:
            assert np.array_equal(theta[b], want), (tag, np.flatnonzero(theta[b] != want)[:8])
            continue
        scale = np.max(np.abs(want))
        bound = 8 * PLANTED_REL_ERR * scale
        gap = min(abs(short[i] - want[i]), abs(short[j] - want[j]))
        assert bound < 1e-3 * gap, tag
        err = np.max(np.abs(theta[b] - want))
        worst = max(worst, err / bound)
        assert err <= bound, (tag, err, bound)
        assert abs(theta[b][i] - short[i]) > 0.5 * gap and abs(theta[b][j] - short[j]) > 0.5 * gap, tag
    print(f"n {n} {route}: {len(ref)} problems, dense cases within {worst:.3f} of the bound")


@pytest.mark.parametrize("n,route", width_routes(WIDTHS))
def test_all_negative_off_diagonals_take_the_shortcut(mod, monkeypatch, n, route):
    """H = 4 R^T R with R = 2I - superdiagonal: -8 beside the diagonal, and the reference answers g / diag"""
    A, y = P.all_negative(n)
    want, sc = cached(("negative", n), lambda: P.first_step(A, y, 1.0))
    assert sc
    probs = ordinary(n)
    Ab, yb = stack([(A, y), (probs[0][0], probs[0][1])])   # a dense neighbour
    theta, st, lam = solve(mod, monkeypatch, route, Ab, yb, lam=1.0, max_iter=1)
    assert np.array_equal(theta[0], want), (n, route, np.flatnonzero(theta[0] != want)[:8])
    assert counters(st[0]) == (1, 2, 1) and lam[0] in (0.5, 4.0)


# ---- hostile values -----------------------------------------------------------------------------------------
def hostile_groups(n):
    """{lambda0: [(kind, last, A, y)]}: lambda0 belongs to the engine, so a batch holds the kinds that share it"""
    groups = {}
    for kind in P.HOSTILE:
        for last in (False, True):
            A, y, lam = P.hostile(kind, n, last)
            groups.setdefault(lam, []).append((kind, last, A, y))
    return groups


@pytest.mark.parametrize("max_iter", [1, 5])
@pytest.mark.parametrize("n,route", width_routes(HOSTILE_WIDTHS))
def test_hostile_first_step_and_run(mod, monkeypatch, n, route, max_iter):
    """Zero and negative pivots, 0 / 0 in one coordinate of the shortcut, NaN and inf in y, a zero gradient
    with f != 0, a step that makes f rise: theta (NaN equal to NaN, inf by sign), f, iteration, calls, done
    and lambda equal the restatement's, and the two ordinary problems of the batch have the bits they have
    in a batch of their own."""
    groups = cached(("hostile", n), lambda: hostile_groups(n))
    probs = ordinary(n)
    for lam0, members in groups.items():
        Ab, yb = stack([(A, y) for _, _, A, y in members] + [(a, b) for a, b, _ in probs])
        m = Ab.shape[1]
        theta, st, lam = solve(mod, monkeypatch, route, Ab, yb, lam=lam0, max_iter=max_iter)
        alone = solve(mod, monkeypatch, route, *stack([P.pad_rows(a, b, m) for a, b, _ in probs]), lam=lam0,
                      max_iter=max_iter)
        for b, (kind, last, A, y) in enumerate(members):
            tag = (kind, n, route, last, max_iter)
            want = cached(("hostile_run",) + tag[:2] + tag[3:],
                          lambda: P.run(A, y, lam=lam0, max_iter=max_iter, update=solver_for(n)))
            assert want[2:] == DERIVED[kind][max_iter == 5], tag
            assert np.array_equal(theta[b], want[0], equal_nan=True), (tag, theta[b][:4], want[0][:4])
            assert np.array_equal(st[b].f_value, want[1], equal_nan=True), (tag, st[b].f_value, want[1])
            assert counters(st[b]) == want[2:4] + (1,), (tag, counters(st[b]))
            assert np.array_equal(lam[b], want[4], equal_nan=True), (tag, lam[b], want[4])
        k = len(members)
        assert np.array_equal(theta[k:], alone[0], equal_nan=True) and np.array_equal(lam[k:], alone[2], equal_nan=True)
        for s, t in zip(st[k:], alone[1]):
            assert counters(s) == counters(t) and np.array_equal(s.f_value, t.f_value, equal_nan=True)


# ---- the stop rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,route", width_routes(EDGE_WIDTHS))
def test_stop_rule_edges(mod, monkeypatch, n, route):
    """f0 = sum y^2 is an exact integer: max_iter = 0 and f_delta one ulp above f0 or inf leave theta0
    untouched after one call; f_delta = f0 (strict <) and NaN run their iteration"""
    probs = ordinary(n)
    A, y = stack([(a, b) for a, b, _ in probs])
    f0 = [float(np.sum(b * b)) for _, b, _ in probs]
    want_f = cached(("dense_f", n), lambda: [P.f_after(a, b, -u) for a, b, u in probs])
    for max_iter, f_delta, iters in P.stop_rule_cases(f0[0]):   # the edge is problem 0's
        theta, st, lam = solve(mod, monkeypatch, route, A, y, lam=0.0, max_iter=max_iter, f_delta=f_delta)
        tag = (n, route, max_iter, f_delta)
        assert counters(st[0]) == (iters, iters + 1, 1) and lam[0] == 0.0, tag
        if iters == 0:
            assert not np.any(theta[0]) and not np.any(np.signbit(theta[0])) and st[0].f_value == f0[0], tag
        else:
            assert np.array_equal(theta[0], -probs[0][2]), tag
            assert abs(st[0].f_value - want_f[0]) <= P.f_bound(want_f[0], y.shape[1]), tag
        # the neighbour has another f0: it runs unless max_iter or an infinite f_delta forbids it
        runs = max_iter > 0 and not (abs(0.0 - f0[1]) < f_delta)
        assert counters(st[1]) == (int(runs), int(runs) + 1, 1), tag
        assert np.array_equal(theta[1], -probs[1][2] if runs else np.zeros(n)), tag


# ---- a link that is exact: the generic Link instantiations over a whole run ---------------------------------
CURVE_BIDIAGONAL = ("const int k = (int)t(0);\n"
                    "r = y - (t(1) * th(k) + (k + 1 < n ? t(2) * th(k + 1) : 0.0));\n"
                    "J(k) = -t(1);  J(k + 1) = -t(2);")


@pytest.mark.parametrize("n,route", width_routes(EDGE_WIDTHS))
def test_identity_link_whole_run(mod, monkeypatch, n, route):
    """exact_dense through LinkRegression with value `return z;` and slope `return 1.0;`: J = -A at every
    theta, so after the exact first step r = 0, f = 0 and g = 0 exactly, and with f_delta = 0 the run goes to
    max_iter with theta = -u, f = 0.0 and lambda = 0"""
    probs = ordinary(n)
    A, y = stack([(a, b) for a, b, _ in probs])
    model = mod.LinkRegression(A, y, "return z;", "return 1.0;")
    theta, st, lam = solve(mod, monkeypatch, route, A, y, lam=0.0, max_iter=6, model=model)
    for b, (_, _, u) in enumerate(probs):
        assert np.array_equal(theta[b], -u), (n, route, b)
        assert st[b].f_value == 0.0 and counters(st[b]) == (6, 7, 1) and lam[b] == 0.0, (n, route, b)


@pytest.mark.parametrize("n", [3, 64])
def test_curve_model_linear_first_step(mod, monkeypatch, n):
    """lm_curve_iter_kernel shares lm_step_wave: exact_dense with a bidiagonal R as a curve model, row k of
    A given by its data (k, R[k][k], R[k][k + 1]). The residual is linear, so f after the step is 0.0."""
    probs = [P.exact_dense(n, seeded(n + 7000 * k), band=1) for k in (0, 1)]
    t = np.zeros((2, 2 * n, 3))
    for b, (A, _, _) in enumerate(probs):
        R = A[:n]
        rows = np.stack([np.arange(n, dtype=np.float64), np.diag(R), np.append(np.diag(R, 1), 0.0)], axis=1)
        t[b] = np.vstack([rows, rows])
    y = np.stack([b for _, b, _ in probs])
    model = mod.CurveModel(t, y, CURVE_BIDIAGONAL, n)
    theta, st, lam = solve(mod, monkeypatch, "default", None, None, lam=0.0, max_iter=1, model=model)
    for b, (_, _, u) in enumerate(probs):
        assert np.array_equal(theta[b], -u), (n, b)
        assert st[b].f_value == 0.0 and counters(st[b]) == (1, 2, 1) and lam[b] == 0.0, (n, b)


# ---- the QR step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", QR_WIDTHS)
def test_qr_step_on_structural_zeros_and_exact_systems(mod, monkeypatch, n):
    """tinyqr's givens_rotation divides 0 / 0 on a pair of zeros: a banded H makes the reference return NaN
    from 17 columns on (both oracle orders, tests/test_lm_planted_cpu.py), and so must the device; below,
    and on a dense integer system, the step is within 8 cond eps max |ref| of the Fraction solution."""
    from nlsolver_amd._capi import LM_QR
    banded, dense = P.banded(n), P.dense_qr(n, seeded(n))
    A, y = stack([banded, dense])
    theta, st, lam = solve(mod, monkeypatch, "default", A, y, lam=1.0, max_iter=1, solver=LM_QR)
    for b, (Ab, yb) in enumerate((banded, dense)):
        ref, cond = cached(("qr", n, b), lambda: qr_reference(Ab, yb, 1.0))
        assert counters(st[b]) == (1, 2, 1)
        if b == 0 and n >= 17:
            assert np.all(np.isnan(theta[b])) and np.isnan(st[b].f_value) and lam[b] == 4.0, (n, theta[b][:4])
            continue
        bound = 8 * cond * P.EPS * np.max(np.abs(ref))
        err = np.max(np.abs(theta[b] - ref))
        print(f"n {n} problem {b}: cond {cond:.2f}, |theta - ref| {err:.3e}, {err / bound:.3f} of the bound")
        assert err <= bound and lam[b] in (0.5, 4.0), (n, b, err, bound)
