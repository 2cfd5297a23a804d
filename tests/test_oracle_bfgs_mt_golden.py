"""Pins oracle_bfgs.c's More-Thuente search (cstep, cvsrch) branch by branch to the reference's own runs.

tests/golden/bfgs_mt.json holds the reference's BFGS (nlsolver.h:3169-3286) on members of a line-search
family without transcendental functions (oracle/ref_driver_more.inc MtFamily; per coordinate
f = ((a q + b x + c) x + d) x + e (q / w), q = x x, w = 1 + q, analytic gradient functor), each at max_iter 1
and 6 with grad_eps 0. At n = 1 the first turn (H = I, d = -g) is exactly one search on
phi(t) = f(x0 - t g(x0)) from stp = alpha, so a member of the family is one line search; max_iter 6 adds
what the solver does after a search that failed (rho infinite or NaN, the reset guard). Several members
run through inf and NaN on purpose. The two-coordinate pairs make H and dir = -H g take part.

1. The oracle equals the reference's x, f, counts and every logged objective value bit for bit (NaN equal
   to NaN), under tree = 0 and tree = 1: a sum of one or two terms has one order.
2. The oracle's branch masks (oracle.h ORC_MT_*, set where the branch is taken) cover EVERY branch of the
   search over the fixture, and each branch has a named record that must take it (WITNESS). The three
   branches a search of the family's value lists did not reach in a first turn turned out reachable by
   directed constructions, so the list of exceptions is empty:
     cstep rejecting its input (infoc = 0)   a quartic 1e200 x^4: the first trial overflows, f = g = inf; case 4
                                             not bracketed sends stp to stmax = 5 stp, whose f - f is NaN and
                                             whose next step is NaN; the trial after it has dx (stp - stx) >= 0
     case 4 not bracketed, stp <= stx        the same quartic from alpha = 1e15: a NaN step compares false with
                                             stx, so stpmin is taken
     exit 2 (xtol)                           b x^3 - 1e100 x^2 from x0 = 0.7: the bracket collapses below
                                             xtol stmax within 7 evaluations; also reached in a later turn of
                                             a plain member (0, 1, -1, 0, -1) from x0 = 1.2, alpha = 0.1

Coverage (records of the fixture whose solve takes the branch, of 166; measured by
test_every_branch_is_covered, which prints the table):
  c1_open 116        c1_bracketed 99    c1_left 30         c1_cubic 66        c1_average 104
  c2_open 26         c2_bracketed 78    c2_left 46         c2_cubic 66        c2_secant 60
  c3_open 39         c3_bracketed 65    c3_left 15         c3_r_negative 86   c3_stpmax 52
  c3_stpmin 9        c3_root_clamped 31 c3_b_cubic 60      c3_b_secant 34     c3_o_cubic 28
  c3_o_secant 29     c4_bracketed 45    c4_right 13        c4_open_stpmax 30  c4_open_stpmin 2
  safeguard_up 19    safeguard_down 8   cstep_reject 2     not_descent 10     fallback_stx 68
  stage_2 94         modified 2         bisection 38       exit_1 121         exit_2 3
  exit_3 54          exit_4 4           exit_5 3           exit_6 15

Taking a branch is not yet depending on it, so the fixture was also tried against deliberately altered copies
of the oracle (one edit each; comparisons that stop matching the reference, of 332 = 166 records under both
orders): fp >= fx for fp > fx 58; the not-bracketed pick of case 3 flipped 56; the safeguard's direction 232;
case 4's gamma
sign 78; case 1's 230; case 3's stpmin replaced by stpmax 12; the swap sty = stx dropped 156; dgxm = dgx +
dgtest in the modified function 4; infoc == 0 dropped from the fallback 4; exit 5 dropped 6; exit 6 dropped
30; dginit > 0 for >= 0 20; 0.7 for 0.66 in the forced bisection 4 and dg > dgtest in exit 4 4 (both zero
before the two members named for them were added). Edits that no record notices, and why: max(0, .) removed
from case 3's root (a NaN gamma fails r < 0 just as gamma == 0 fails gamma != 0: the same substitute step);
exit 2 dropped (its condition also makes stp = stx and with it exit 6: the same return); max for min(ftol,
gtol) in the stage test (between the two thresholds exit 1 fires first); stpmax for stpmin in case 4 not
bracketed (only a NaN step gets there, and every later value is NaN either way); fym = fy - stx dgtest in the
modified function (fy is read by bracketed case 4 alone; 400 000 members of the value lists show no
difference); <= for < in case 3's bracketed pick (a tie of two distances).
"""
import math

import pytest

from tests import _oracle as O
from tests.test_oracle_golden import hx

# Branches that may be missing from the fixture, each with the reason it cannot arise from BFGS::solve's
# fixed stpmin, stpmax, xtol. A cap, not a convenience: all three candidates (cstep_reject, c4_open_stpmin,
# exit_2) have witnesses, so nothing may be missing.
EXCEPTIONS = {}

# branch -> the record that must take it (the members the fixture was built around)
_W1 = "case1_open_and_bracketed_case3_case4_bisection_exit1/m1"
_W4 = "case2_open_secant_case3_open_cubic_case4_right/m1"
WITNESS = {
    "c1_open": _W1, "c1_bracketed": _W1, "c1_average": _W1, "c3_bracketed": _W1, "c3_b_cubic": _W1,
    "c3_b_secant": _W1, "c3_r_negative": _W1, "c3_stpmax": _W1, "c4_bracketed": _W1, "bisection": _W1,
    "exit_1": _W1,
    "c1_cubic": "case1_cubic_pick_and_left/m1", "c1_left": "case1_cubic_pick_and_left/m1",
    "c2_bracketed": "case2_bracketed_cubic_stage2/m1", "c2_cubic": "case2_bracketed_cubic_stage2/m1",
    "stage_2": "case2_bracketed_cubic_stage2/m1",
    "c2_open": _W4, "c2_secant": _W4, "c3_open": _W4, "c3_o_cubic": _W4, "c4_right": _W4,
    "c2_left": "case2_left/m1", "c3_left": "case3_left/m1", "c3_stpmin": "case3_stpmin/m1",
    "c3_o_secant": "case3_open_secant/m1", "c3_root_clamped": "case3_root_clamped/m1",
    "c4_open_stpmax": "case4_open_stpmax_fallback_exit3/m1",
    "fallback_stx": "case4_open_stpmax_fallback_exit3/m1", "exit_3": "case4_open_stpmax_fallback_exit3/m1",
    "exit_4": "exit4/m1", "exit_5": "exit5_one_evaluation/m1", "exit_6": "exit6/m1",
    "modified": "modified_function/m1", "safeguard_down": "safeguard_down/m1",
    "safeguard_up": "safeguard_up/m1", "not_descent": "not_descent/m1",
    "cstep_reject": "cstep_reject_overflowing_quartic/m1",
    "c4_open_stpmin": "case4_open_stpmin_overflowing_quartic/m1",
    "exit_2": "exit2_first_turn/m1",
}


def same_bits(a, b):
    """equal bit for bit, NaN equal to NaN"""
    a, b = list(a), list(b)
    return len(a) == len(b) and all(
        (math.isnan(u) and math.isnan(v)) or (u == v and math.copysign(1.0, u) == math.copysign(1.0, v))
        for u, v in zip(a, b))


def run_record(oracle, r, tree):
    return O.bfgs_mt(oracle, [hx(v) for v in r["params"]], [hx(v) for v in r["x0"]], max_iter=r["max_iter"],
                     grad_eps=hx(r["grad_eps"]), alpha=hx(r["alpha"]), tree=tree)


@pytest.fixture(scope="module")
def runs(oracle, golden):
    """{record name: (record, {tree: oracle run})}, computed once"""
    return {name: (r, {tree: run_record(oracle, r, tree) for tree in (0, 1)})
            for name, r in golden("bfgs_mt.json").items()}


def test_fixture_shape(runs):
    """every member at max_iter 1 and 6, grad_eps 0; witnesses, 40 members, 20 pairs; nine step lengths"""
    names = {n.split("/")[0] for n in runs}
    assert {n for n in runs} == {f"{m}/m{k}" for m in names for k in (1, 6)}
    assert sum(n.startswith("member_") for n in names) == 40 and sum(n.startswith("pair_") for n in names) == 20
    assert all(r["n"] == (2 if n.startswith("pair_") else 1) for n, (r, _) in runs.items())
    assert all(hx(r["grad_eps"]) == 0.0 and r["max_iter"] == int(n[-1]) for n, (r, _) in runs.items())
    assert len({r["alpha"] for r, _ in runs.values()}) == 9
    # the reference ran: the functor's own gradient count is the status's, the log holds every call
    assert all(r["gcalls"] == r["g_calls_seen"] and r["fcalls"] == len(r["f_vals"]) for r, _ in runs.values())


@pytest.mark.parametrize("tree", [0, 1])
def test_oracle_matches_reference_on_every_record(runs, tree):
    wrong = []
    for name, (r, by_tree) in runs.items():
        st, x, flog, _, _, _ = by_tree[tree]
        if not same_bits(x, [hx(v) for v in r["x"]]):
            wrong.append((name, "x", x.tolist(), r["x"]))
        if not same_bits([st.f_value], [hx(r["f"])]):
            wrong.append((name, "f", st.f_value, r["f"]))
        if (st.iteration, st.function_calls_used, st.gradient_evals_used) != (r["iters"], r["fcalls"], r["gcalls"]):
            wrong.append((name, "counts", (st.iteration, st.function_calls_used, st.gradient_evals_used),
                          (r["iters"], r["fcalls"], r["gcalls"])))
        if not same_bits(flog, [hx(v) for v in r["f_vals"]]):
            wrong.append((name, "f_vals"))
    assert not wrong, wrong[:8]


def test_masks_do_not_depend_on_the_order(runs):
    assert all(by_tree[0][3] == by_tree[1][3] for _, by_tree in runs.values())


def test_every_branch_is_covered(runs):
    """the union of the masks is every branch (at most EXCEPTIONS missing, and none is), and every branch's
    named record takes it"""
    assert set(EXCEPTIONS) <= {"cstep_reject", "c4_open_stpmin", "exit_2"}
    assert set(WITNESS) | set(EXCEPTIONS) == set(O.MT_BRANCHES) and not set(WITNESS) & set(EXCEPTIONS)
    hits = {b: [name for name, (_, by_tree) in runs.items() if b in by_tree[0][3]] for b in O.MT_BRANCHES}
    print("\nbranch, records taking it (of %d)" % len(runs))
    for b in O.MT_BRANCHES:
        print(f"  {b:18s} {len(hits[b]):4d}")
    print("exceptions remaining:", EXCEPTIONS or "none")
    missed = {b: rec for b, rec in WITNESS.items() if rec not in hits[b]}
    assert not missed, f"branch -> the record that should take it and does not: {missed}"
    uncovered = [b for b in O.MT_BRANCHES if not hits[b] and b not in EXCEPTIONS]
    assert not uncovered, uncovered


def test_device_bodies_restate_the_family(oracle, runs):
    """the source text tests/test_bfgs_linesearch_gpu.py hands to the device, read as Python (the same
    operators, the same grouping, IEEE doubles without contraction), equals the oracle's fam_f / fam_g at every
    record's start, bit for bit: max_iter 0 makes the oracle return f(x0) and the gradient at x0"""
    from tests.test_bfgs_linesearch_gpu import family, slope
    for name, (r, _) in runs.items():
        params = [hx(v) for v in r["params"]]
        env = dict(p=lambda k: params[k], __builtins__={})
        for pt in ([hx(v) for v in r["x0"]], [hx(v) for v in r["x"]]):  # (the end points: inf and NaN too)
            st, _, _, _, g, _ = O.bfgs_mt(oracle, params, pt, max_iter=0, alpha=1.0)
            f = [eval(family("x", [f"p({5 * i + k})" for k in range(5)]), dict(env, x=pt[i]))
                 for i in range(r["n"])]
            want = 0.0 + f[0] if r["n"] == 1 else 0.0 + (f[0] + f[1])
            assert same_bits([want], [st.f_value]), name
            got = [eval(slope("x", [f"p(5 * i + {k})" for k in range(5)]), dict(env, x=pt[i], i=i))
                   for i in range(r["n"])]
            assert same_bits(got, g), name


def test_a_search_is_one_first_turn(runs):
    """max_iter 1 at n = 1: one search, at most 20 evaluations after f(x0), each with its gradient, then the
    gradient at the new point and the closing value: fcalls = 2 + nfev, gcalls = 2 + nfev, nfev <= 20"""
    for name, (r, _) in runs.items():
        if r["max_iter"] == 1:
            assert r["iters"] == 1 and r["fcalls"] == r["gcalls"] and 2 <= r["fcalls"] <= 22, name
    assert runs["exit5_one_evaluation/m1"][0]["fcalls"] == 3
    assert runs["not_descent/m1"][0]["fcalls"] == 2  # no search at all
    assert runs["case4_open_stpmax_fallback_exit3/m1"][0]["fcalls"] == 22
