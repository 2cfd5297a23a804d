"""Parity tests: batched HIP BFGS (through the C-ABI) vs oracle_bfgs.c with the kernel's
summation tree (tree=1): bit-exact iterates, objective values, counters, inverse Hessians.
Against the reference arithmetic (tree=0, pinned by goldens): objective within 1e-12."""
import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available()
    import nlsolver_amd
    return nlsolver_amd


def starts(batch, n, seed=0):
    rng = np.random.default_rng(seed)
    x = 1.0 + 0.5 * (rng.random((batch, n)) - 0.5)
    x[0] = 1.0  # the golden start
    return x


@pytest.mark.parametrize("n,batch", [(8, 5), (64, 9), (100, 4), (130, 6), (257, 3), (1024, 4)])
@pytest.mark.parametrize("kw", [dict(max_iter=100, grad_eps=1e-10, alpha=1.0),
                                dict(max_iter=100, grad_eps=5e-3, alpha=1.0),
                                dict(max_iter=7, grad_eps=0.0, alpha=0.5)])
def test_bfgs_batch_bit_exact_vs_tree_oracle(mod, oracle, n, batch, kw):
    d, b, c = O.quad_problem(n)
    x0 = starts(batch, n, seed=n)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    for p in range(batch):
        ref, xr, _ = O.bfgs_quad(oracle, x0[p], tree=1, **kw)
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used), f"problem {p}"
        assert st[p].f_value == ref.f_value, f"problem {p}"
        assert np.array_equal(x[p], xr), f"problem {p}"
        assert st[p].done == 1


def assert_gradient_within_rounding(g, x, d, b, c):
    """The downloaded gradient of the G6 quadratic against the exact one at the device's own iterate:
    g*_i = d_i x_i + c sum(x) - b_i in rationals. Whatever the order of the n - 1 additions of sum(x),
    the product with c, the product d_i x_i and the two additions that join them, the computed value
    is within gamma_{n+2} (|d_i x_i| + |c| sum|x_j| + |b_i|) of it, gamma_k = k u / (1 - k u),
    u = 2^-53 (the standard bound of a sum of k + 1 terms in any order, each term carrying at most
    one more rounding): derived, nothing measured."""
    from fractions import Fraction as Fr
    n = len(x)
    k, u = n + 2, Fr(1, 2**53)
    gamma = k * u / (1 - k * u)
    xs = [Fr(float(v)) for v in x]
    sx, sabs = sum(xs), sum(abs(v) for v in xs)
    cf = Fr(float(c))
    for i in range(n):
        di, bi = Fr(float(d[i])), Fr(float(b[i]))
        exact = di * xs[i] + cf * sx - bi
        bound = gamma * (abs(di * xs[i]) + abs(cf) * sabs + abs(bi))
        assert abs(Fr(float(g[i])) - exact) <= bound, (i, float(g[i]), float(exact), float(bound))


def test_bfgs_inverse_hessian_and_gradient_after_k_iterations(mod, oracle):
    """State after exactly k turns (max_iter = k): gradient and H^-1 bit-exact."""
    n, batch, k = 96, 3, 4
    d, b, c = O.quad_problem(n)
    x0 = starts(batch, n, seed=7)
    kw = dict(max_iter=k, grad_eps=0.0, alpha=1.0)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, **kw) as eng:
        eng.init(x0)
        eng.step(k)
        g, H = eng.download_state()
        x, _ = eng.download()
    import ctypes as C
    for p in range(batch):
        # replay the oracle by hand for k iterations to obtain H: run k and k-1 ... simpler:
        # the quadratic's gradient at the device iterate must equal the device gradient, and
        # the device iterate must equal the oracle's iterate after k iterations
        Href = np.zeros((n, n))
        ref, xr, _ = O.bfgs_quad(oracle, x0[p], tree=1, hessian=Href, **kw)
        assert np.array_equal(x[p], xr)
        sx = x[p].sum()
        assert np.allclose(g[p], d * x[p] + c * sx - b, rtol=1e-13, atol=1e-13)
        assert_gradient_within_rounding(g[p], x[p], d, b, c)
        # H stays symmetric up to the rounding of the (denom*s_i)*s_j term and maps y to ~s
        assert np.allclose(H[p], H[p].T, rtol=0, atol=1e-9)
        assert np.array_equal(H[p], Href), (p, np.argwhere(H[p] != Href)[:4])


def test_bfgs_matches_reference_arithmetic_within_1e12(mod, oracle, golden):
    """Device result vs the reference itself (golden, sequential sums) on the G6 starts."""
    g = golden("bfgs.json")
    for name in ("n8", "n64", "n1024", "n64_default_stop"):
        c = g[name]
        n = c["n"]
        d, b, cc = O.quad_problem(n)
        x0 = np.full((1, n), float.fromhex(c["x0"]))
        kw = dict(max_iter=c["max_iter"], grad_eps=float.fromhex(c["grad_eps"]),
                  alpha=float.fromhex(c["alpha"]))
        st = mod.BFGS(mod.QuadDiagRank1(d, b, cc), None, kw["max_iter"], kw["grad_eps"],
                      kw["alpha"], reference_order=False).minimize(x0[0])  # (the tree-order kernels)
        fref = float.fromhex(c["f"])
        assert abs(st.f_value - fref) <= 1e-12 * abs(fref), name
        if kw["grad_eps"] >= 1e-6:
            assert (st.iteration, st.function_calls_used, st.gradient_evals_used) == \
                (c["iters"], c["fcalls"], c["gcalls"])


def test_bfgs_config3_shape_sample(mod, oracle):
    """BASELINE config 3's shape (n = 1024) with a reduced batch: every problem bit-exact,
    problems finish at different iterations (done-mask)."""
    n, batch = 1024, 24
    d, b, c = O.quad_problem(n)
    x0 = starts(batch, n, seed=3)
    x0[5] *= 3.0
    kw = dict(max_iter=50, grad_eps=1e-6, alpha=1.0)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    iters = set()
    for p in range(batch):
        ref, xr, _ = O.bfgs_quad(oracle, x0[p], tree=1, **kw)
        assert st[p].iteration == ref.iteration and st[p].f_value == ref.f_value
        assert np.array_equal(x[p], xr)
        iters.add(st[p].iteration)
    assert len(iters) > 1


def test_bfgs_config3_full_batch(mod, oracle):
    """BASELINE configs[2] at its full size — n = 1024, batch = 4096 independent starts (32 GiB of
    inverse Hessians: 64-bit offsets, every block of the H passes in use): 18 sampled problems
    including the first and the LAST index bit for bit against the tree oracle; every problem
    finished, inside max_iter, no higher than it started (More-Thuente's sufficient decrease),
    and problems stop at different iterations (done mask)."""
    n, batch = 1024, 4096
    d, b, c = O.quad_problem(n)
    rng = np.random.default_rng(33)
    x0 = 1.0 + 0.5 * (rng.random((batch, n)) - 0.5)
    x0[::7] *= 1.0 + rng.random((len(x0[::7]), 1))  # spread the iteration counts
    kw = dict(max_iter=50, grad_eps=1e-6, alpha=1.0)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    sample = sorted({0, 1, 7, 255, 256, 2047, 2048, 4094, 4095, *rng.integers(0, batch, 9).tolist()})
    assert len(sample) >= 16
    for p in sample:
        ref, xr, _ = O.bfgs_quad(oracle, x0[p], tree=1, **kw)
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used), p
        assert st[p].f_value == ref.f_value and np.array_equal(x[p], xr), p

    def quad(v):
        sv = v.sum(axis=1)
        return 0.5 * (v * v * d).sum(axis=1) + 0.5 * c * sv * sv - (v * b).sum(axis=1)

    f_start, f_end = quad(x0), np.array([s.f_value for s in st])
    assert all(s.done == 1 and 1 <= s.iteration <= 50 for s in st)
    assert np.all(f_end <= f_start) and np.allclose(f_end, quad(x), rtol=1e-12, atol=1e-12)
    assert len({s.iteration for s in st}) > 1
    # all of them are near the one minimiser of the convex quadratic. How near is the reference's
    # own behaviour, not a device tolerance: its stop test (nlsolver.h:3239-3241) fires
    # when ||g|| < grad_eps OR when the DIFFERENCE of two successive gradient norms does,
    # | ||g_k|| - ||g_{k-1}|| | < grad_eps — so a start whose norm stalls between two iterations
    # stops with ||g|| ~ 1e-3 still on the table (measured spread of the end points: 1.1e-3 with these 4096
    # starts; the sampled problems above are bit-equal to the oracle's runs, which is the parity)
    assert np.max(np.abs(x - x[0])) < 1e-2


@pytest.mark.parametrize("obj,n,batch", [("rosenbrock", 2, 6), ("rosenbrock", 5, 4),
                                         ("rosenbrock", 16, 5), ("rosenbrock", 128, 4),
                                         ("rosenbrock", 130, 3), ("rosenbrock", 256, 2),
                                         ("sphere", 7, 4), ("styblinski_tang", 64, 4),
                                         ("rastrigin", 2, 4), ("rastrigin", 48, 3)])
@pytest.mark.parametrize("kw", [dict(max_iter=6, grad_eps=0.0, alpha=1.0),
                                dict(max_iter=40, grad_eps=5e-3, alpha=0.5)])
def test_bfgs_default_finite_difference_gradient_bit_exact(mod, oracle, obj, n, batch, kw):
    """The reference's default-gradient path (fin_diff, nlsolver.h:1385-1413) on built-in
    objectives: every probe is a full evaluation in the lane-tree order, so iterates, objective
    value and the counters (4 n function calls per gradient) equal the tree oracle bit for bit."""
    rng = np.random.default_rng(1000 + n)
    x0 = 0.8 + 0.4 * (rng.random((batch, n)) - 0.5)
    with mod.BFGSEngine(obj, batch, dim=n, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    for p in range(batch):
        ref, xr, _, _ = O.bfgs_fd(oracle, obj, x0[p], tree=1, **kw)
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used), f"problem {p}"
        assert st[p].f_value == ref.f_value, f"problem {p}"
        assert np.array_equal(x[p], xr), f"problem {p}"
        assert st[p].done == 1


def test_bfgs_finite_difference_close_to_reference(mod, oracle, golden):
    """Device (lane tree) vs the reference itself (golden, sequential sums), short horizon."""
    from tests.test_oracle_golden import hx
    g = golden("bfgs_fd.json")["rosenbrock_n128_20iters"]
    x0 = (hx(g["x0"]) + hx(g["x0_step"]) * np.arange(g["n"], dtype=np.float64)).reshape(1, -1)
    with mod.BFGSEngine("rosenbrock", 1, dim=g["n"], max_iter=3, grad_eps=0.0, alpha=1.0) as eng:
        x, st = eng.minimize(x0.copy())
    ref, xr, _, _ = O.bfgs_fd(oracle, "rosenbrock", x0[0], max_iter=3, grad_eps=0.0, alpha=1.0,
                              tree=0)
    assert (st[0].iteration, st[0].gradient_evals_used) == (ref.iteration, ref.gradient_evals_used)
    assert abs(st[0].f_value - ref.f_value) <= 1e-6 * abs(ref.f_value)
    assert np.max(np.abs(x[0] - xr)) <= 1e-5


@pytest.mark.parametrize("obj,n,batch", [("rosenbrock", 257, 2), ("rosenbrock", 300, 2),
                                         ("sphere", 600, 2), ("rosenbrock", 1024, 2)])
def test_bfgs_finite_difference_gradient_past_256_dimensions(mod, oracle, obj, n, batch):
    """The default-gradient model past the old 256-dimension limit (the reference has none,
    nlsolver.h:1385-1413): first size past it, ragged chunk counts, the largest vector the
    wave holds. 4 n probes per gradient, each a full evaluation; bit-exact vs the tree oracle."""
    kw = dict(max_iter=3, grad_eps=0.0, alpha=1.0)
    rng = np.random.default_rng(2000 + n)
    x0 = 0.8 + 0.4 * (rng.random((batch, n)) - 0.5)
    with mod.BFGSEngine(obj, batch, dim=n, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    for p in range(batch):
        ref, xr, _, _ = O.bfgs_fd(oracle, obj, x0[p], tree=1, **kw)
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used), f"problem {p}"
        assert st[p].f_value == ref.f_value and np.array_equal(x[p], xr), f"problem {p}"


def test_bfgs_rejects_more_than_1024_dimensions(mod):
    with pytest.raises(RuntimeError, match="1024"):
        mod.BFGSEngine("rosenbrock", 2, dim=1100)


# ---- NLSG_BFGS_SYMMETRIC: the rank-2 update restated so that H stays bitwise symmetric, upper
# ---- 128 x 128 blocks only (include/nlsg_c_api.h; oracle tree = 2)
@pytest.mark.parametrize("n,batch", [(8, 5), (64, 6), (100, 4), (128, 3), (130, 5), (257, 3), (1024, 3)])
@pytest.mark.parametrize("kw", [dict(max_iter=100, grad_eps=1e-8, alpha=1.0),
                                dict(max_iter=100, grad_eps=5e-3, alpha=1.0),
                                dict(max_iter=7, grad_eps=0.0, alpha=0.5)])
def test_bfgs_symmetric_bit_exact_vs_oracle(mod, oracle, n, batch, kw):
    d, b, c = O.quad_problem(n)
    x0 = starts(batch, n, seed=n)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, symmetric=True, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    for p in range(batch):
        ref, xr, _ = O.bfgs_quad(oracle, x0[p], tree=2, **kw)
        assert (st[p].iteration, st[p].function_calls_used, st[p].gradient_evals_used) == \
            (ref.iteration, ref.function_calls_used, ref.gradient_evals_used), f"problem {p}"
        assert st[p].f_value == ref.f_value, f"problem {p}"
        assert np.array_equal(x[p], xr), f"problem {p}"
        assert st[p].done == 1


@pytest.mark.parametrize("n", [96, 130, 300])
def test_bfgs_symmetric_inverse_hessian_bit_exact_and_symmetric(mod, oracle, n):
    """The stored upper blocks after k updates, expanded: equal to the oracle's H bit for bit, and
    the oracle's H (computed on the whole matrix with the restated formula) is bitwise symmetric —
    which is what makes keeping half of it legitimate."""
    batch, k = 3, 5
    d, b, c = O.quad_problem(n)
    x0 = starts(batch, n, seed=70 + n)
    kw = dict(max_iter=k, grad_eps=0.0, alpha=1.0)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, symmetric=True, **kw) as eng:
        eng.init(x0)
        eng.step(k)
        g, H = eng.download_state()
    for p in range(batch):
        Href = np.zeros((n, n))
        O.bfgs_quad(oracle, x0[p], tree=2, hessian=Href, **kw)
        assert np.array_equal(Href, Href.T)
        assert np.array_equal(H[p], Href), p


def test_bfgs_symmetric_matches_reference_within_1e12(mod, golden):
    """Symmetric restatement vs the reference itself (golden, literal update, sequential sums) on
    the G6 runs: f within 1e-12 relative, and where the stop test is not at the rounding floor
    (grad_eps = 5e-3) the same iteration / call counts."""
    g = golden("bfgs.json")
    for name in ("n8", "n64", "n1024", "n64_default_stop"):
        c = g[name]
        n = c["n"]
        d, b, cc = O.quad_problem(n)
        x0 = np.full((1, n), float.fromhex(c["x0"]))
        kw = dict(max_iter=c["max_iter"], grad_eps=float.fromhex(c["grad_eps"]),
                  alpha=float.fromhex(c["alpha"]))
        st = mod.BFGS(mod.QuadDiagRank1(d, b, cc), None, kw["max_iter"], kw["grad_eps"],
                      kw["alpha"], symmetric=True).minimize(x0[0])
        fref = float.fromhex(c["f"])
        assert abs(st.f_value - fref) <= 1e-12 * abs(fref), name
        if kw["grad_eps"] >= 1e-6:
            assert (st.iteration, st.function_calls_used, st.gradient_evals_used) == \
                (c["iters"], c["fcalls"], c["gcalls"])


def test_bfgs_symmetric_config3_full_batch(mod, oracle):
    """BASELINE configs[2] at full size with the symmetric restatement (18 GiB of upper blocks
    instead of 32 GiB): sampled problems incl. the first and the last bit for bit vs oracle tree 2,
    and every problem within 1e-10 of what the literal engine reaches."""
    n, batch = 1024, 4096
    d, b, c = O.quad_problem(n)
    rng = np.random.default_rng(34)
    x0 = 1.0 + 0.5 * (rng.random((batch, n)) - 0.5)
    x0[::7] *= 1.0 + rng.random((len(x0[::7]), 1))
    kw = dict(max_iter=50, grad_eps=1e-6, alpha=1.0)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), batch, symmetric=True, **kw) as eng:
        x, st = eng.minimize(x0.copy())
    sample = sorted({0, 1, 255, 2048, 4094, 4095, *rng.integers(0, batch, 6).tolist()})
    for p in sample:
        ref, xr, _ = O.bfgs_quad(oracle, x0[p], tree=2, **kw)
        assert (st[p].iteration, st[p].function_calls_used) == (ref.iteration, ref.function_calls_used), p
        assert st[p].f_value == ref.f_value and np.array_equal(x[p], xr), p
    assert all(s.done == 1 and 1 <= s.iteration <= 50 for s in st)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), 64, **kw) as eng:
        x_lit, st_lit = eng.minimize(x0[:64].copy())
    f_sym = np.array([s.f_value for s in st[:64]])
    f_lit = np.array([s.f_value for s in st_lit])
    assert np.allclose(f_sym, f_lit, rtol=1e-10, atol=0)
