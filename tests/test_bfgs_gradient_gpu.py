"""BFGS with the analytic gradient of a compiled objective (CustomObjective grad_body=,
nlsg_bfgs_create_gradient): the model kBfgsCustomGrad of nlsg_bfgs_kernels.h on the device.

What is compared with what, always bit for bit:
  * the gradient at the start with the body's expression evaluated in Python floats (no contraction on
    either side), at the sizes where the lane layout changes: one coordinate, odd sizes (the scalar load
    path), the lane and chunk boundaries of CHUNKS 1, 2, 4 and 8, a partial last workgroup (batch 5);
  * `s`, the sum of terms handed to the body, with the engine's own f(x0) — and in reference order with
    an index-order Python loop —, also under a non-linear finish;
  * whole solves with the engine that is pinned to the reference: a whole-vector objective with D
    parameters that restates the G6 quadratic against QuadDiagRank1 (x, status, g, H; the problems stop at
    different iterations, so waves leave the lock-step driver one by one), literal and symmetric update;
  * the per-lane (terms) form with its whole-vector twin over multi-iteration runs, and a coefficient
    given as p(0) with the literal one; new rows take effect without a rebuild;
  * the terms form in reference order with QuadDiagRank1 in reference order;
  * the reference's counts with a Grad functor (function_calls_used == gradient_evals_used) and f_value
    at the returned x on the Rosenbrock chain, both summation orders;
  * the drop-in header's BFGS<Custom, double, device::analytic_grad> with the Python drop-in."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROSEN_TERM = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;"
ROSEN_GRAD = ("double g = 0.0; if (i + 1 < D) g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi); "
              "if (i > 0) g = g + 200.0 * (xi - xm * xm); return g;")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rosen_grad_py(x):
    """ROSEN_GRAD in Python floats, operation by operation"""
    D = len(x)
    out = []
    for i in range(D):
        xi = float(x[i])
        g = 0.0
        if i + 1 < D:
            xn = float(x[i + 1])
            g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi)
        if i > 0:
            xm = float(x[i - 1])
            g = g + 200.0 * (xi - xm * xm)
        out.append(g)
    return out


def rosen_terms_py(x):
    out = []
    for i in range(len(x) - 1):
        xi, xn = float(x[i]), float(x[i + 1])
        t1 = 1 - xi
        t2 = xn - xi * xi
        out.append(t1 * t1 + 100 * t2 * t2)
    return out


def index_order_sum(terms):
    acc = 0.0
    for t in terms:
        acc = acc + t
    return acc


def rosen_starts(D, B):
    """every problem another start, no two neighbours alike"""
    return np.array([[-1.2 + 0.1 * b + 0.125 * ((5 * i + 3 * b) % 17) for i in range(D)] for b in range(B)])


def quad_starts(D, B=6):
    return np.array([[(1 + 0.25 * b + 0.01 * ((7 * i + 3 * b) % 11)) * (-1.0 if i % 3 == 0 else 1.0)
                      for i in range(D)] for b in range(B)])


def rosenbrock(grad=True):
    import nlsolver_amd
    return nlsolver_amd.CustomObjective(ROSEN_TERM, chain=True, grad_body=ROSEN_GRAD if grad else None)


def status_tuple(st):
    return [(int(bits(s.f_value)[0]), s.iteration, s.function_calls_used, s.gradient_evals_used) for s in st]


# ---- 1: the gradient at the start ---------------------------------------------------------------
GRAD_SIZES = [(D, False) for D in (1, 2, 3, 64, 65, 128, 129, 130, 257, 513, 1024)] + \
             [(D, True) for D in (3, 129, 1024)]


@pytest.mark.parametrize("D,ref", GRAD_SIZES)
def test_gradient_at_the_start_is_the_bodys_expression(D, ref):
    import nlsolver_amd
    B = 5
    x0 = rosen_starts(D, B)
    with nlsolver_amd.BFGSEngine(rosenbrock(), B, dim=D, reference_order=ref) as eng:
        assert eng.gradient_used == "analytic"
        eng.init(x0)
        g, _ = eng.download_state(hessian=False)
    want = np.array([rosen_grad_py(x0[b]) for b in range(B)])
    assert g.shape == (B, D)
    assert same(g, want), (D, ref, np.argwhere(bits(g) != bits(want))[:4])


def test_a_compiler_error_names_the_gradient_bodys_line():
    import nlsolver_amd
    obj = nlsolver_amd.CustomObjective("return xi * xi;", grad_body="double g = 2.0 * xi;\nreturn g +;")
    with pytest.raises(nlsolver_amd.NlsgError) as ei:
        nlsolver_amd.BFGSEngine(obj, 2, dim=3)
    assert ei.value.code == 1 and "grad_body:2" in str(ei.value)


# ---- 2: `s` ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [False, True])
def test_s_is_the_sum_that_finish_receives(ref):
    import nlsolver_amd
    D, B = 130, 5
    obj = nlsolver_amd.CustomObjective(ROSEN_TERM, chain=True, grad_body="return s + xi;")
    x0 = rosen_starts(D, B)
    with nlsolver_amd.BFGSEngine(obj, B, dim=D, max_iter=0, reference_order=ref) as eng:
        x, st = eng.minimize(x0.copy())
        g, _ = eng.download_state(hessian=False)
    assert same(x, x0)
    for b in range(B):
        assert st[b].iteration == 0 and st[b].function_calls_used == 1 and st[b].gradient_evals_used == 1
        f0 = st[b].f_value                     # identity finish: f(x0) IS s
        if ref:
            assert bits(f0) == bits(index_order_sum(rosen_terms_py(x0[b]))), b
        assert same(g[b], [f0 + float(v) for v in x0[b]]), b


def test_s_under_a_non_linear_finish_in_reference_order():
    import nlsolver_amd
    D, B = 130, 5
    body = ROSEN_GRAD.replace("return g;", "return g / (2.0 * sqrt(s));")
    obj = nlsolver_amd.CustomObjective(ROSEN_TERM, chain=True, finish_body="return sqrt(s);", grad_body=body)
    x0 = rosen_starts(D, B)
    with nlsolver_amd.BFGSEngine(obj, B, dim=D, max_iter=0, reference_order=True) as eng:
        _, st = eng.minimize(x0.copy())
        g, _ = eng.download_state(hessian=False)
    for b in range(B):
        s = index_order_sum(rosen_terms_py(x0[b]))
        assert bits(st[b].f_value) == bits(math.sqrt(s)), b
        assert same(g[b], [v / (2.0 * math.sqrt(s)) for v in rosen_grad_py(x0[b])]), b


# ---- 3: whole solves against the engine pinned to the reference ---------------------------------------
QUAD_ITERATIONS = {129: [20, 20, 27, 27, 18, 27], 130: [18, 27, 28, 18, 27, 26]}  # the CPU oracle, tree order


def quad_weights(D):
    return np.array([10.0 ** (1.5 * i / (D - 1)) for i in range(D)])


def solve_quadratic_both_ways(D, symmetric):
    import nlsolver_amd
    B = 6
    d = quad_weights(D)
    obj = nlsolver_amd.CustomObjective("return 0.5 * x.sum([](double v, uint64_t i) { return p(i) * v * v; });",
                                       vector=True, n_params=D, grad_body="return p(i) * x(i);")
    x0 = quad_starts(D, B)
    kw = dict(max_iter=100, grad_eps=5e-3, alpha=1.0, symmetric=symmetric)
    with nlsolver_amd.BFGSEngine(obj, B, dim=D, **kw) as eng:
        assert eng.gradient_used == "analytic"
        x, st = eng.minimize(x0.copy(), params=np.tile(d, (B, 1)))
        g, H = eng.download_state()
    with nlsolver_amd.BFGSEngine(nlsolver_amd.QuadDiagRank1(d, np.zeros(D), 0.0), B, **kw) as eng:
        xq, stq = eng.minimize(x0.copy())
        gq, Hq = eng.download_state()
    return (x, st, g, H), (xq, stq, gq, Hq)


@pytest.mark.parametrize("D", [129, 130])
def test_vector_form_with_parameters_equals_the_quadratic_engine(D):
    (x, st, g, H), (xq, stq, gq, Hq) = solve_quadratic_both_ways(D, False)
    assert [s.iteration for s in stq] == QUAD_ITERATIONS[D]
    assert min(s.iteration for s in st) >= 10          # whole runs, not a trivial agreement
    for s in st:
        assert s.function_calls_used == s.gradient_evals_used == 3 * s.iteration + 1
    assert status_tuple(st) == status_tuple(stq)
    assert same(x, xq)
    assert same(g, gq)
    assert same(H, Hq)


def test_vector_form_equals_the_quadratic_engine_with_the_symmetric_update():
    (x, st, g, H), (xq, stq, gq, Hq) = solve_quadratic_both_ways(130, True)
    assert min(s.iteration for s in st) >= 10
    assert status_tuple(st) == status_tuple(stq)
    assert same(x, xq) and same(g, gq) and same(H, Hq)


# ---- 4: the terms form against its whole-vector twin ---------------------------------------------------
def quartic(form, c="16.0", c2="32.0", n_params=0):
    """0.5 sum (x^4 - c x^2 + 5 x) and its derivative 0.5 (4 x^3 - c2 x + 5), c2 = 2 c, by terms or whole-vector"""
    import nlsolver_amd
    term = f"double q = xi * xi; return 0.5 * (q * q - {c} * q + 5.0 * xi);"
    grad = f"return 0.5 * (4.0 * xi * xi * xi - {c2} * xi + 5.0);"
    if form == "terms":
        return nlsolver_amd.CustomObjective(term, n_params=n_params, grad_body=grad)
    return nlsolver_amd.CustomObjective("return x.sum([](double xi, uint64_t) { " + term + " });", vector=True,
                                        n_params=n_params, grad_body="double xi = x(i); " + grad)


def run_tree(obj, D, rows=None, B=6):
    import nlsolver_amd
    with nlsolver_amd.BFGSEngine(obj, B, dim=D) as eng:
        out = []
        for r in ([None] if rows is None else rows):
            x, st = eng.minimize(quad_starts(D, B), params=None if r is None else np.full((B, 1), r))
            g, _ = eng.download_state(hessian=False)
            out.append((x, status_tuple(st), g))
    return out if rows is not None else out[0]


@pytest.mark.parametrize("D", [5, 130])
def test_terms_form_equals_its_vector_twin(D):
    x, st, g = run_tree(quartic("terms"), D)
    xv, stv, gv = run_tree(quartic("vector"), D)
    assert max(s[1] for s in st) >= 3                  # several iterations
    assert st == stv
    assert same(x, xv) and same(g, gv)


def test_a_coefficient_as_a_parameter_equals_the_literal_and_rows_are_replaced():
    D = 130
    literal16 = run_tree(quartic("terms"), D)
    literal12 = run_tree(quartic("terms", "12.0", "24.0"), D)
    # (2.0 * p(0) is exact: 32.0 and 24.0, the literals' own constants)
    by16, by12, again16 = run_tree(quartic("terms", "p(0)", "2.0 * p(0)", 1), D, rows=[16.0, 12.0, 16.0])
    for got, want in ((by16, literal16), (by12, literal12), (again16, literal16)):
        assert got[1] == want[1]
        assert same(got[0], want[0]) and same(got[2], want[2])
    assert not same(by16[0], by12[0])                  # the rows did change the problem


# ---- 5: reference order, terms form ----------------------------------------------------------------------
def test_terms_form_in_reference_order_equals_the_quadratic_engine():
    import nlsolver_amd
    D, B = 129, 6
    obj = nlsolver_amd.CustomObjective("return 3.0 * xi * xi;", finish_body="return 0.5 * s;",
                                       grad_body="return 3.0 * xi;")
    x0 = quad_starts(D, B)
    with nlsolver_amd.BFGSEngine(obj, B, dim=D, reference_order=True) as eng:
        x, st = eng.minimize(x0.copy())
        g, H = eng.download_state()
    quad = nlsolver_amd.QuadDiagRank1(np.full(D, 3.0), np.zeros(D), 0.0)
    with nlsolver_amd.BFGSEngine(quad, B, reference_order=True) as eng:
        xq, stq = eng.minimize(x0.copy())
        gq, Hq = eng.download_state()
    assert min(s.iteration for s in st) >= 1
    assert status_tuple(st) == status_tuple(stq)
    assert same(x, xq) and same(g, gq) and same(H, Hq)


# ---- 6: invariants on the Rosenbrock chain -----------------------------------------------------------------
@pytest.mark.parametrize("D,ref", [(16, False), (16, True), (130, False), (130, True)])
def test_counts_and_values_on_the_rosenbrock_chain(D, ref):
    import nlsolver_amd
    B = 6
    x0 = rosen_starts(D, B)
    with nlsolver_amd.BFGSEngine(rosenbrock(), B, dim=D, reference_order=ref) as eng:
        x, st = eng.minimize(x0.copy())
    for b in range(B):
        assert st[b].iteration >= 1
        assert st[b].function_calls_used == st[b].gradient_evals_used, b      # a Grad functor's counts
        assert st[b].f_value < index_order_sum(rosen_terms_py(x0[b])), b
    if ref:
        for b in range(B):
            assert bits(st[b].f_value) == bits(index_order_sum(rosen_terms_py(x[b]))), b
    else:
        with nlsolver_amd.BFGSEngine(rosenbrock(), B, dim=D, max_iter=0) as eng:
            _, st0 = eng.minimize(x.copy())
        assert [bits(s.f_value) for s in st0] == [bits(s.f_value) for s in st]
    # the default gradient on the same objective pays 4 D objective evaluations per gradient
    with nlsolver_amd.BFGSEngine(rosenbrock(), B, dim=D, max_iter=3, reference_order=ref,
                                 gradient="finite_difference") as eng:
        assert eng.gradient_used == "finite_difference"
        _, stf = eng.minimize(x0.copy())
    for b in range(B):
        assert stf[b].function_calls_used > 4 * D * stf[b].gradient_evals_used, b


# ---- 7: the drop-in header -----------------------------------------------------------------------------------
def test_header_analytic_grad_equals_the_python_drop_in(tmp_path):
    import nlsolver_amd
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_bfgs_gradient")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_bfgs_gradient.cpp"), "-o", exe, "-ldl"])
    D = 16
    x0 = rosen_starts(D, 1)[0]
    argv = [float(v).hex() for v in x0]
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    env.pop("NLSG_SUMMATION", None)   # (the header's default order is the drop-in's: reference)
    for mode, obj, used in (("analytic", rosenbrock(), "analytic"),
                            ("default", rosenbrock(grad=False), "finite_difference")):
        solver = nlsolver_amd.BFGS(obj)
        x = x0.copy()
        st = solver.minimize(x)
        assert solver.gradient_used == used
        got = json.loads(subprocess.check_output([exe, mode] + argv, env=env, text=True, timeout=300))
        assert same([float.fromhex(v) for v in got["x"]], x), mode
        assert bits(float.fromhex(got["f"])) == bits(st.f_value), mode
        assert (got["iters"], got["fcalls"], got["gcalls"]) == \
            (st.iteration, st.function_calls_used, st.gradient_evals_used), mode
        if mode == "analytic":
            assert st.iteration >= 1 and st.function_calls_used == st.gradient_evals_used
    # minimize_batch and Custom::params under analytic_grad: two starts, one row shown to both
    xb = quad_starts(5, 2)
    solver = nlsolver_amd.BFGS(quartic("terms", "p(0)", "2.0 * p(0)", 1), params=[16.0])
    want = xb.copy()
    stb = solver.minimize(want)
    assert solver.gradient_used == "analytic"
    got = json.loads(subprocess.check_output([exe, "batch", float(16.0).hex()] + [float(v).hex() for v in xb.ravel()],
                                             env=env, text=True, timeout=300))
    assert len(got) == 2
    for b in range(2):
        assert same([float.fromhex(v) for v in got[b]["x"]], want[b]), b
        assert bits(float.fromhex(got[b]["f"])) == bits(stb[b].f_value), b
        assert (got[b]["iters"], got[b]["fcalls"], got[b]["gcalls"]) == \
            (stb[b].iteration, stb[b].function_calls_used, stb[b].gradient_evals_used), b
        assert stb[b].iteration >= 1
    r = subprocess.run([exe, "empty"] + argv, env=env, text=True, capture_output=True, timeout=300)
    assert r.returncode == 3 and "grad_body" in r.stderr
