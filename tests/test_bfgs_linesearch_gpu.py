"""The More-Thuente search of the BFGS device engines (mt_cstep in nlsg_bfgs_kernels.h, cvsrch in
nlsg_bfgs_turn.h — a restructured text, not a transcription) against the reference's own runs, branch by branch.

tests/golden/bfgs_mt.json holds the reference's BFGS on members of a line-search family (see
tests/test_oracle_bfgs_mt_golden.py, which shows that the fixture takes every branch of cstep / cvsrch). Here
the family is a CustomObjective with its gradient body and the member's numbers as run-time parameters p(k):
a batch is a batch of independent line searches. The bodies restate the expression tree of the reference
driver's functors operation for operation, and the objective is a sum of ONE term, so tree order and reference
order have the same bits and all four engines — lock step and resident, either order — must return the
fixture's x, f, iteration and call counts bit for bit (NaN equal to NaN), and leave the oracle's gradient and
inverse Hessian in download_state(). Nothing here has a tolerance.

dim 1: term(xi) = family(xi; p(0..4)). dim 2: the chain form, whose single term is
family(x_0; p(0..4)) + family(x_1; p(5..9)); the gradient body picks its five parameters by i.
One engine per step length alpha and max_iter (1: the search alone; 6: what the solver does after a search
that failed); the engines of a source share one compilation."""
import numpy as np
import pytest

from tests import _oracle as O
from tests.test_oracle_golden import hx

pytestmark = pytest.mark.gpu


def family(x, P):
    """the family's value at `x` (an expression) under the five parameter expressions P, as oracle_bfgs.c fam_f"""
    return (f"(({P[0]} * ({x} * {x}) + {P[1]} * {x} + {P[2]}) * {x} + {P[3]}) * {x}"
            f" + {P[4]} * (({x} * {x}) / (1 + {x} * {x}))")


def slope(x, P):
    """its derivative, as oracle_bfgs.c fam_g"""
    return (f"((4 * {P[0]} * {x} + 3 * {P[1]}) * {x} + 2 * {P[2]}) * {x} + {P[3]}"
            f" + {P[4]} * ((2 * {x}) / ((1 + {x} * {x}) * (1 + {x} * {x})))")


def objective(mod, dim, literal=None):
    """literal: the five numbers of a dim-1 member written into the bodies instead of p(k)"""
    if literal is not None:
        assert dim == 1
        P = ["(" + float(v).hex() + ")" for v in literal]
        return mod.CustomObjective("return " + family("xi", P) + ";", grad_body="return " + slope("xi", P) + ";")
    P0 = [f"p({k})" for k in range(5)]
    Pi = [f"p(5 * i + {k})" for k in range(5)]
    grad = "return " + slope("xi", Pi) + ";"
    if dim == 1:
        return mod.CustomObjective("return " + family("xi", P0) + ";", n_params=5, grad_body=grad)
    P1 = [f"p({k})" for k in range(5, 10)]
    term = f"const double f0 = {family('xi', P0)}; const double f1 = {family('xn', P1)}; return f0 + f1;"
    return mod.CustomObjective(term, chain=True, n_params=10, grad_body=grad)


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    return nlsolver_amd


@pytest.fixture(scope="module")
def records(golden, oracle):
    """{name: record + the oracle's gradient and inverse Hessian after the solve}, computed once"""
    out = {}
    for name, r in golden("bfgs_mt.json").items():
        rec = dict(name=name, n=r["n"], max_iter=r["max_iter"], alpha=hx(r["alpha"]),
                   params=[hx(v) for v in r["params"]], x0=[hx(v) for v in r["x0"]],
                   x=[hx(v) for v in r["x"]], f=hx(r["f"]), iters=r["iters"], fcalls=r["fcalls"],
                   gcalls=r["gcalls"])
        assert hx(r["grad_eps"]) == 0.0 and rec["iters"] >= 1
        st, x, _, _, g, H = O.bfgs_mt(oracle, rec["params"], rec["x0"], max_iter=rec["max_iter"],
                                      alpha=rec["alpha"], tree=0)
        assert same(x, rec["x"]) and same([st.f_value], [rec["f"]])  # (the CPU test's subject, restated)
        rec["g"], rec["H"] = g, H
        out[name] = rec
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def batches(records, dim):
    """[(alpha, max_iter, [records])]: the members of one step length and max_iter are one batch"""
    groups = {}
    for rec in records.values():
        if rec["n"] == dim:
            groups.setdefault((rec["alpha"], rec["max_iter"]), []).append(rec)
    return [(a, m, recs) for (a, m), recs in sorted(groups.items())]


def check_problem(rec, x, st, g, H, tag):
    what = f"{tag} {rec['name']} params {rec['params']} x0 {rec['x0']} alpha {rec['alpha']}"
    assert same(x, rec["x"]), (what, "x", x.tolist(), rec["x"])
    assert same([st.f_value], [rec["f"]]), (what, "f", st.f_value, rec["f"])
    assert (st.iteration, st.function_calls_used, st.gradient_evals_used) == \
        (rec["iters"], rec["fcalls"], rec["gcalls"]), (what, "iteration, function calls, gradient calls")
    if g is not None:
        assert same(g, rec["g"]), (what, "gradient", g.tolist(), rec["g"].tolist())
        assert same(H, rec["H"]), (what, "H", H.tolist(), rec["H"].tolist())


@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("ref", [False, True], ids=["tree", "reference_order"])
@pytest.mark.parametrize("resident", [False, True], ids=["lock_step", "resident"])
def test_every_record_on_the_device(mod, records, dim, ref, resident):
    obj = objective(mod, dim)
    groups = batches(records, dim)
    if dim == 1:
        assert len({a for a, _, _ in groups}) == 9 and {m for _, m, _ in groups} == {1, 6}
    seen = 0
    for alpha, max_iter, recs in groups:
        B = len(recs)
        assert B <= 100
        x0 = np.array([r["x0"] for r in recs])
        rows = np.array([r["params"] for r in recs])
        with mod.BFGSEngine(obj, B, dim=dim, max_iter=max_iter, grad_eps=0.0, alpha=alpha,
                            reference_order=ref, resident=resident) as eng:
            assert eng.gradient_used == "analytic" and eng.resident == resident
            x, st = eng.minimize(x0.copy(), params=rows)
            g, H = eng.download_state()
        tag = f"dim {dim} {'resident' if resident else 'lock step'} {'reference' if ref else 'tree'} order:"
        for b, rec in enumerate(recs):
            check_problem(rec, x[b], st[b], g[b], H[b], tag)
            assert st[b].done == 1
        seen += B
    assert seen == sum(r["n"] == dim for r in records.values())


_W1 = "case1_open_and_bracketed_case3_case4_bisection_exit1"


@pytest.mark.parametrize("max_iter", [1, 6])
def test_literals_in_the_body_give_the_same_bits(mod, records, max_iter):
    """the member's five numbers as literals instead of p(k): the parameter staging is not what decides"""
    rec = records[f"{_W1}/m{max_iter}"]
    with mod.BFGSEngine(objective(mod, 1, literal=rec["params"]), 1, dim=1, max_iter=max_iter, grad_eps=0.0,
                        alpha=rec["alpha"]) as eng:
        x, st = eng.minimize(np.array([rec["x0"]]))
        g, H = eng.download_state()
    check_problem(rec, x[0], st[0], g[0], H[0], "literals:")


@pytest.mark.parametrize("driver", ["turns", "resident"])
@pytest.mark.parametrize("name", [_W1, "cstep_reject_overflowing_quartic"])
def test_drop_in(mod, records, driver, name):
    """BFGS(f, None, 1, 0.0, alpha, driver=...) as the reference's class is called: one search"""
    rec = records[f"{name}/m1"]
    solver = mod.BFGS(objective(mod, 1), None, 1, 0.0, rec["alpha"], driver=driver, params=rec["params"])
    x = np.array(rec["x0"])
    st = solver.minimize(x)
    assert solver.driver_used == driver and solver.gradient_used == "analytic"
    check_problem(rec, x, st, None, None, f"drop-in, driver {driver}:")
