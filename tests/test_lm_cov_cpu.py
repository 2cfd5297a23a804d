"""Parameter covariance of a Levenberg-Marquardt fit (nlsg_lm_covariance, LMEngine.covariance / stderr), as
far as the host decides it before any device is touched — the entry point and its argtypes, the scale
argument, the null-engine refusal, the header against a library without the symbol — and the yardsticks
of tests/test_lm_cov_gpu.py:

  lm_covariance_ref   cov = c (J^T J)^-1 as a plain Cholesky inverse in float64: G = J^T J by sums in row
                      order, G = L L^T, X = L^-1, cov = c X^T X; ok = every pivot > 0 (and f finite in
                      residual mode), else all NaN.
  exact_problem       problems whose G^-1 is exact in float64 whatever the order of operations: G = L L^T
                      with L = L0 diag(d), L0 unit lower triangular with entries in {-1, 0, 1} (+-1 on the
                      whole subdiagonal, +-1 below it with probability 0.5 at n <= 5, 0.15 at n <= 33, 0.05
                      beyond), d_j in {1, 2, 4, 8}. The design matrix is A = L^T followed by four zero rows,
                      y is 0 on the first n rows and 2 on the last four: at theta = 0, f = 16 and
                      s2 = 16 / 4 = 4. The Cholesky pivots are the d_j^2, so roots, reciprocals and
                      divisions are exact, G^-1 has integer numerators over powers of two.
  rational_inverse    the inverse of a symmetric positive definite matrix in fractions.Fraction.
  enclosed_inverse    the exact inverse of the exact Gram matrix of a float64 J, rounded once — without the
                      minutes rational elimination takes at n = 64: an approximate inverse X is refined by
                      Newton's iteration in integer arithmetic until the exactly computed residual
                      R = I - G X is below 2^-300; then G^-1 = X (I - R)^-1, so every entry of G^-1 lies
                      within delta = |X|_inf |R|_inf / (1 - |R|_inf) of X's, and where both ends of that
                      interval round to the same double (asserted for every entry) that double IS the exact
                      inverse rounded once.

The property the exact GPU cases rest on is proved here for the very seeds they use: run in Fractions,
lm_covariance_ref's every partial sum is a dyadic number of at most 40 significant bits, and its float64
run returns the rational result bit for bit."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import nlsolver_amd
from nlsolver_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_N = (1, 2, 5, 33, 64)
B = 3


# ---- the yardstick --------------------------------------------------------------------------------------
def _cholesky_inverse(G, n, zero, one, root, note=lambda v: v):
    """(X^T X lower triangle as a full symmetric list of lists, pivots) with G = L L^T, X = L^-1; every
    partial sum passes through note(). Scalars are floats or Fractions."""
    L = [[zero] * n for _ in range(n)]
    piv = []
    for j in range(n):
        s = zero
        for k in range(j):
            s = note(s + note(L[j][k] * L[j][k]))
        d = note(G[j][j] - s)
        piv.append(d)
        if not d > 0:
            return None, piv
        L[j][j] = root(d)
        for i in range(j + 1, n):
            s = zero
            for k in range(j):
                s = note(s + note(L[i][k] * L[j][k]))
            L[i][j] = note(note(G[i][j] - s) / L[j][j])
    X = [[zero] * n for _ in range(n)]
    for i in range(n):
        for c in range(i + 1):
            s = zero
            for k in range(c, i):
                s = note(s + note(L[i][k] * X[k][c]))
            X[i][c] = note(note((one if i == c else zero) - s) / L[i][i])
    inv = [[zero] * n for _ in range(n)]
    for i in range(n):
        for c in range(i + 1):
            s = zero
            for k in range(i, n):
                s = note(s + note(X[k][i] * X[k][c]))
            inv[i][c] = inv[c][i] = s
    return inv, piv


def _gram(J):
    m, n = J.shape
    G = np.zeros((n, n))
    for r in range(m):  # sums in row order
        G += np.outer(J[r], J[r])
    return G


def lm_covariance_ref(J, f, m, scale):
    """J (m', n) float64 (m' may leave out all-zero rows; m is the model's count), f = sum r^2,
    scale "residual" / "absolute" -> (cov (n, n), s2, ok)"""
    J = np.asarray(J, dtype=np.float64)
    n = J.shape[1]
    s2 = f / (m - n) if m > n else np.nan
    with np.errstate(all="ignore"):
        G = _gram(J)
        inv, _ = _cholesky_inverse(G.tolist(), n, 0.0, 1.0, lambda d: float(np.sqrt(d)))
    ok = inv is not None and (scale == "absolute" or bool(np.isfinite(f)))
    if not ok:
        return np.full((n, n), np.nan), s2, False
    return (s2 if scale == "residual" else 1.0) * np.array(inv), s2, True


# ---- exact problems -------------------------------------------------------------------------------------
def exact_factor(n, seed):
    """L = L0 diag(d) as integers"""
    rng = np.random.default_rng(seed)
    p = 0.5 if n <= 5 else 0.15 if n <= 33 else 0.05
    L0 = np.eye(n, dtype=np.int64)
    for i in range(1, n):
        for j in range(i):
            sign = int(rng.choice([-1, 1]))
            if j == i - 1 or rng.random() < p:
                L0[i, j] = sign
    d = 2 ** rng.integers(0, 4, n)
    return L0 * d[None, :]


@functools.lru_cache(maxsize=None)
def exact_problem(n, b, pad=4):
    """problem b of the exact batch at n: A (n + pad, n), y (n + pad,), and G^-1 as float64, exact"""
    L = exact_factor(n, 1000 * n + b)
    A = np.concatenate([L.T.astype(np.float64), np.zeros((pad, n))])
    y = np.concatenate([np.zeros(n), np.full(pad, 2.0)])
    inv = rational_inverse((L @ L.T).tolist())
    ginv = np.array([[float(v) for v in row] for row in inv])
    assert all(Fraction(float(v)) == v for row in inv for v in row), "G^-1 is not representable"
    for a in (A, y, ginv):
        a.setflags(write=False)
    return A, y, ginv


def exact_batch(n, pad=4):
    """A (B, m, n), y (B, m), G^-1 (B, n, n)"""
    return tuple(np.stack(x) for x in zip(*(exact_problem(n, b, pad) for b in range(B))))


def rational_inverse(G):
    """the inverse of a symmetric positive definite matrix (lists of ints or Fractions), in Fractions:
    G = L D L^T, G^-1 = L^-T D^-1 L^-1"""
    n = len(G)
    G = [[Fraction(v) for v in row] for row in G]
    L = [[Fraction(0)] * n for _ in range(n)]
    D = [Fraction(0)] * n
    for j in range(n):
        D[j] = G[j][j] - sum(L[j][k] * L[j][k] * D[k] for k in range(j))
        assert D[j] > 0
        for i in range(j + 1, n):
            L[i][j] = (G[i][j] - sum(L[i][k] * L[j][k] * D[k] for k in range(j))) / D[j]
    X = [[Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for i in range(n):
        for c in range(i):
            X[i][c] = -sum(L[i][k] * X[k][c] for k in range(c, i))
    inv = [[None] * n for _ in range(n)]
    for i in range(n):
        for c in range(i + 1):
            inv[i][c] = inv[c][i] = sum(X[k][i] * X[k][c] / D[k] for k in range(i, n))
    return inv


def _dyadic_ints(a):
    """a float64 array as (object array of Python ints, s) with a = ints / 2^s exactly"""
    ratios = [float(v).as_integer_ratio() for v in np.asarray(a, dtype=np.float64).ravel()]
    s = max(q.bit_length() - 1 for _, q in ratios)
    ints = np.array([p << (s - (q.bit_length() - 1)) for p, q in ratios], dtype=object).reshape(np.shape(a))
    return ints, s


def enclosed_inverse(J):
    """float64 (n, n): the inverse of the exact J^T J of the float64 matrix J, rounded once"""
    J = np.asarray(J, dtype=np.float64)
    n = J.shape[1]
    Ji, a = _dyadic_ints(J)
    Gi = Ji.T.dot(Ji)  # exact, scale 2^-2a
    X0 = np.linalg.inv(J.T @ J)
    Xi, s = _dyadic_ints(0.5 * (X0 + X0.T))
    keep = 640  # fraction bits X is cut back to between the steps (an approximation may be cut anywhere)
    if s < keep:
        Xi, s = Xi * (1 << (keep - s)), keep
    eye = np.array([[int(i == j) for j in range(n)] for i in range(n)], dtype=object)
    for _ in range(12):
        Ri = eye * (1 << (2 * a + s)) - Gi.dot(Xi)  # R = I - G X, exact, scale 2^-(2a + s)
        rnorm = Fraction(max(sum(abs(v) for v in row) for row in Ri.tolist()), 1 << (2 * a + s))
        if rnorm < Fraction(1, 1 << 300):
            break
        Xi = (Xi * (1 << (2 * a + s)) + Xi.dot(Ri)) // (1 << (2 * a + s + s - keep))  # X + X R, cut to `keep`
        s = keep
    else:
        raise AssertionError(f"Newton's iteration did not reach 2^-300: |R| = {float(rnorm):.3e}")
    xnorm = max(sum(abs(v) for v in row) for row in Xi.tolist())
    delta = int(xnorm * rnorm / (1 - rnorm)) + 1  # in units of 2^-s
    out = np.empty((n, n))
    for i in range(n):
        for j in range(n):
            lo, hi = (Xi[i, j] - delta) / (1 << s), (Xi[i, j] + delta) / (1 << s)  # int / int: rounded once
            assert lo == hi, f"entry ({i}, {j}): the enclosure straddles a rounding boundary"
            out[i, j] = lo
    return out


def bits_needed(v):
    """significant bits of a dyadic rational"""
    v = Fraction(v)
    assert v.denominator & (v.denominator - 1) == 0, f"{v} is not dyadic"
    p = abs(v.numerator)
    return (p // (p & -p)).bit_length() if p else 0


# ---- the yardsticks' own tests --------------------------------------------------------------------------
@pytest.mark.parametrize("n", EXACT_N)
def test_the_exact_cases_are_exact_in_float64(n):
    """the seeds of tests/test_lm_cov_gpu.py: no partial sum of the Cholesky inverse needs more than 40
    bits, its float64 run is the rational run, and both are the rational inverse"""
    for b in range(B):
        A, y, ginv = exact_problem(n, b)
        J = -A
        G = _gram(J)
        assert np.array_equal(G, G.T) and np.array_equal(G, np.rint(G))
        widest = [0]

        def note(v):
            widest[0] = max(widest[0], bits_needed(v))
            return v

        def root(d):
            r = Fraction(int(np.sqrt(float(d))))
            assert r * r == d, f"pivot {d} is not a square"
            return r

        Gq = [[Fraction(int(v)) for v in row] for row in G]
        inv_q, piv = _cholesky_inverse(Gq, n, Fraction(0), Fraction(1), root, note)
        print(f"n {n} problem {b}: widest partial sum {widest[0]} bits, pivots in {sorted(set(map(int, piv)))}")
        assert widest[0] <= 40
        assert set(map(int, piv)) <= {1, 4, 16, 64}
        assert inv_q == rational_inverse(Gq)
        r = y - A @ np.zeros(n)
        f = float(r @ r)
        assert f == 16.0
        for scale, c in (("absolute", 1.0), ("residual", 4.0)):
            cov, s2, ok = lm_covariance_ref(J, f, n + 4, scale)
            assert ok and s2 == 4.0
            assert np.array_equal(cov, c * ginv)
            assert np.array_equal(cov, np.array([[float(c * v) for v in row] for row in inv_q]))
        assert np.array_equal(np.linalg.inv(G), ginv)  # (numpy's LU gets it too)


def test_the_batch_holds_three_different_problems():
    for n in EXACT_N[1:]:
        A = exact_batch(n)[0]
        assert not np.array_equal(A[0], A[1]) and not np.array_equal(A[1], A[2]), n


def test_the_reference_fails_where_the_contract_says():
    A, y, _ = exact_problem(5, 1)
    J = -np.array(A)
    J[:, 3] = J[:, 1]  # two identical columns: the pivot is exactly 0
    cov, s2, ok = lm_covariance_ref(J, 16.0, 9, "absolute")
    assert not ok and np.all(np.isnan(cov)) and cov.shape == (5, 5)
    J = -np.array(A)
    J[:, 2] = 0.0
    assert not lm_covariance_ref(J, 16.0, 9, "residual")[2]
    J = -np.array(A)
    assert not lm_covariance_ref(J, np.nan, 9, "residual")[2]
    assert lm_covariance_ref(J, np.nan, 9, "absolute")[2]  # (f does not enter)
    assert np.isnan(lm_covariance_ref(J[:5], 0.0, 5, "absolute")[1])  # m = n: no residual variance


def test_the_enclosed_inverse_is_the_rational_one():
    rng = np.random.default_rng(7)
    J = rng.uniform(-1.0, 1.0, (30, 12))
    Jq = [[Fraction(float(v)) for v in row] for row in J]
    G = [[sum(Jq[r][i] * Jq[r][j] for r in range(30)) for j in range(12)] for i in range(12)]
    want = np.array([[float(v) for v in row] for row in rational_inverse(G)])  # (Fraction -> float: rounded once)
    got = enclosed_inverse(J)
    assert np.array_equal(got, want)
    # and what the issue measured of float inverses on such inputs: a fraction of kappa eps
    kappa = np.linalg.cond(J.T @ J)
    for name, inv in (("numpy.linalg.inv", np.linalg.inv(J.T @ J)),
                      ("Cholesky inverse", lm_covariance_ref(J, 1.0, 31, "absolute")[0])):
        ratio = np.max(np.abs(inv - want)) / (kappa * 2.0 ** -52 * np.max(np.abs(want)))
        print(f"{name}: err / (kappa eps) = {ratio:.3f}")
        assert ratio <= 4.0


# ---- the boundary ---------------------------------------------------------------------------------------
def test_the_symbol_and_its_argtypes_load():
    lib = _capi.lib()
    assert "nlsg_lm_covariance" in _capi.OPTIONAL_SYMBOLS
    fn = _capi.require("nlsg_lm_covariance")
    assert fn is lib.nlsg_lm_covariance
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, _capi.pd, C.c_int32, _capi.pd, _capi.pd, C.POINTER(C.c_int32)]
    assert (_capi.LM_COV_RESIDUAL, _capi.LM_COV_ABSOLUTE) == (0, 1)
    assert lib.nlsg_abi_version() == 1


def test_a_null_engine_is_an_invalid_argument():
    lib = _capi.lib()
    theta, cov = np.zeros(4), np.zeros(16)
    rc = lib.nlsg_lm_covariance(None, theta.ctypes.data_as(_capi.pd), 0, cov.ctypes.data_as(_capi.pd), None, None)
    assert rc == _capi.NLSG_ERR_INVALID_ARG and b"null" in lib.nlsg_last_error()


class _NoLibrary:
    """an engine whose every touch of the library is an error"""
    cfg = type("cfg", (), dict(batch=3, n=2))()
    covariance = nlsolver_amd.LMEngine.covariance

    @property
    def _h(self):
        raise AssertionError("the library was touched")


@pytest.mark.parametrize("scale", ["Residual", "sigma", 2, -1, None, True, 0.0])
def test_a_bad_scale_is_a_value_error_before_the_library(scale):
    for method in (nlsolver_amd.LMEngine.covariance, nlsolver_amd.LMEngine.stderr):
        with pytest.raises(ValueError, match="scale"):
            method(_NoLibrary(), np.zeros((3, 2)), scale)
    lm = nlsolver_amd.LevenbergMarquardt(nlsolver_amd.TanhRegression(np.zeros((3, 4, 2)), np.zeros((3, 4))))
    for method in (lm.covariance, lm.stderr):
        with pytest.raises(ValueError, match="scale"):
            method(np.zeros((3, 2)), scale)  # (raised before an engine is made: no device here)


def test_the_scale_names_and_constants():
    from nlsolver_amd.lm import _cov_scale
    assert _cov_scale("residual") == _cov_scale(_capi.LM_COV_RESIDUAL) == 0
    assert _cov_scale("absolute") == _cov_scale(np.int32(_capi.LM_COV_ABSOLUTE)) == 1


# ---- the header against a library without the symbol ----------------------------------------------------
def test_the_header_names_the_missing_symbol_and_leaves_no_engine(tmp_path):
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe, stub, log = str(tmp_path / "header_lm_cov_missing"), str(tmp_path / "libnlsg_stub.so"), str(tmp_path / "log")
    flags = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(flags + ["-fPIC", "-shared", os.path.join(cpp, "stub_nlsg.cpp"), "-o", stub])
    subprocess.check_call(flags + [os.path.join(cpp, "header_lm_cov_missing.cpp"), "-o", exe, "-ldl"])
    env = dict(os.environ, NLSG_LIBRARY=stub, NLSG_STUB_LOG=log)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout.splitlines()[0] == "minimized"
    assert "device_error: the loaded library has no nlsg_lm_covariance" in r.stdout
    calls = open(log).read().splitlines()
    assert [c.split()[0] for c in calls].count("nlsg_lm_create") == 1  # minimize's engine; covariance made none
    assert calls[-1] == "live_engines 0"
