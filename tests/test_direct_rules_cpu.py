"""The independent references of tests/_direct_ref.py (Nelder-Mead, the NM / PSO hybrid, SANN)
anchored from three sides, and the coverage conditions of the case list that
tests/test_direct_rules_gpu.py runs on the device (tests/_direct_cases.py):

  * on the oracle's built-in objectives, where scores are finite and tie-free and all the rules
    coincide, each reference equals the C restatement bit for bit: the keying and the arithmetic;
  * RefNelderMead equals the committed runs of the reference itself (tests/golden/nm.json, up to
    16-D) and the unmodified reference's runs on the hostile families (tests/golden/nm_hostile.json,
    even n: an odd n is the reference's out-of-bounds write);
  * the hostile objectives' source text, compiled for the host, agrees with its Python twin on a
    grid of edges;
  * over the GPU module's exact case list the references' own counters show every action, every
    scan category (the frozen scan and the B3 quirk included), every SANN outcome and the hybrid's
    tied and NaN sort keys at least three times per kernel class.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import _direct_cases as Cs
from tests import _direct_ref as R
from tests import _hostile as H
from tests import _oracle as O

BUILTIN = ("rosenbrock", "sphere", "styblinski_tang")
ANCHOR_SIZES = (2, 7, 33, 130)


def tree_objective(lib, name):
    def f(x):
        a = np.array(x, dtype=np.float64)
        return float(lib.orc_objective_tree(O.OBJ[name], O._ptr(a), a.size))
    return f


def same_run(st, x, res):
    return (np.array_equal(x, np.array(res.x)) and R.same_bits(st.f_value, res.f_value) and
            st.iteration == res.iteration and st.function_calls_used == res.function_calls_used)


# ---- anchors on the oracle's objectives -------------------------------------------------------------
@pytest.mark.parametrize("n", ANCHOR_SIZES)
def test_ref_nelder_mead_equals_the_oracle_on_builtin_objectives(oracle, n):
    iters = 60 if n < 100 else 12
    for obj in BUILTIN:
        x0 = 0.5 + 0.01 * np.arange(n)
        for kw in (dict(), dict(minimize=False, upper=2.0, lower=-2.0), dict(restarts=1, step=0.75)):
            st, x, eps, _ = O.nm_run(oracle, x0, obj=obj, eps=0.0, max_iter=iters, no_change=1000, order=1, **kw)
            rkw = dict(kw)
            if "upper" in rkw:
                rkw["upper"], rkw["lower"] = [rkw["upper"]] * n, [rkw["lower"]] * n
            res = R.RefNelderMead(tree_objective(oracle, obj), eps=0.0, max_iter=iters, no_change=1000,
                                  tree=True, **rkw).run(x0)
            assert same_run(st, x, res), (obj, kw)
            assert R.same_bits(eps, res.eps)


@pytest.mark.parametrize("n", ANCHOR_SIZES)
def test_ref_hybrid_equals_the_oracle_on_builtin_objectives(oracle, n):
    iters = 30 if n < 30 else (6 if n < 100 else 2)
    P = R.Prims(oracle)
    for obj in BUILTIN:
        x0 = 0.5 + 0.01 * np.arange(n)
        for kw in (dict(), dict(minimize=False, upper=2.0, lower=-2.0)):
            st, x, _ = O.nmpso_sync(oracle, obj, x0, 77, 3, eps=0.0, max_iter=iters, no_change=1000, **kw)
            rkw = dict(kw)
            if "upper" in rkw:
                rkw["upper"], rkw["lower"] = [rkw["upper"]] * n, [rkw["lower"]] * n
            res = R.RefHybrid(tree_objective(oracle, obj), P, seed=77, instance=3, eps=0.0, max_iter=iters,
                              no_change=1000, **rkw).run(x0)
            assert same_run(st, x, res), (obj, kw)


@pytest.mark.parametrize("n", ANCHOR_SIZES)
def test_ref_sann_equals_the_oracle_on_builtin_objectives(oracle, n):
    iters = 20 if n < 100 else 6
    P = R.Prims(oracle)
    for obj in BUILTIN:
        x0 = 0.5 + 0.01 * np.arange(n)
        for minimize in (True, False):
            st, x, _ = O.sann_sync(oracle, obj, x0, 77, 5, minimize=minimize, max_iter=iters, temp_iter=5,
                                   temp_max=10.0)
            res = R.RefSANN(tree_objective(oracle, obj), P, seed=77, chain=5, minimize=minimize,
                            max_iter=iters, temp_iter=5, temp_max=10.0).run(x0)
            assert same_run(st, x, res), (obj, minimize)


def test_draw_rows_are_the_scalar_primitives(oracle):
    P = R.Prims(oracle)
    k = P.key(12345, 678)
    assert P.u01_row(k, 3, 2, 9) == [P.u01(P.key(k, 3 + 2 * i)) for i in range(9)]
    assert P.rnorm_row(k, 0, 2, 9) == [P.rnorm(P.key(k, 2 * i)) for i in range(9)]


# ---- anchors on the reference's own runs --------------------------------------------------------------
def rosenbrock_serial(x):
    acc = 0.0
    for i in range(len(x) - 1):
        t1 = 1 - x[i]
        t2 = x[i + 1] - x[i] * x[i]
        acc = acc + (t1 * t1 + 100 * t2 * t2)
    return acc


def test_ref_nelder_mead_reproduces_the_reference_runs(golden):
    g = golden("nm.json")
    ran = 0
    for name, run in g.items():
        if "D" not in run or run["D"] > 16:
            continue
        n = run["D"]
        fh = float.fromhex
        x0 = [fh(run["x0"]) + fh(run["x0_step"]) * float(i) for i in range(n)]
        bounded = bool(run["bounded"])
        res = R.RefNelderMead(rosenbrock_serial, minimize=bool(run["minimize"]),
                              upper=[fh(run["upper"])] * n if bounded else None,
                              lower=[fh(run["lower"])] * n if bounded else None, step=fh(run["step"]),
                              eps=fh(run["eps"]), max_iter=run["max_iter"], no_change=run["no_change"],
                              restarts=run["restarts"], tree=False, stop_margin=False).run(x0)
        assert (res.function_calls_used, res.iteration) == (run["fcalls"], run["iters"]), name
        assert R.same_bits(res.f_value, fh(run["f"])), name
        assert all(R.same_bits(a, fh(b)) for a, b in zip(res.x, run["x"])), name
        ran += 1
    assert ran >= 6


def test_ref_nelder_mead_reproduces_the_reference_on_hostile_objectives(golden):
    runs = golden("nm_hostile.json")["runs"]
    assert sorted(runs) == sorted(f"{name}/{r}" for name, r in Cs.golden_runs())
    assert len(runs) >= 30
    sizes, kinds = set(), set()
    for key, run in runs.items():
        name, r = key.split("/")
        batch = Cs.batch_by_name(name)
        assert batch.n % 2 == 0
        res, _ = Cs.nm_reference(batch, False)[int(r)]
        assert (res.function_calls_used, res.iteration) == (run["fcalls"], run["iters"]), key
        assert R.same_value(res.f_value, float.fromhex(run["f"])), key
        assert all(R.same_bits(a, float.fromhex(b)) for a, b in zip(res.x, run["x"])), key
        sizes.add(batch.n)
        kinds.add((batch.minimize, batch.bounded, batch.restarts > 0))
    assert sizes == {2, 4, 8, 16, 64}
    assert {k[0] for k in kinds} == {True, False} and {k[1] for k in kinds} == {True, False}
    assert {k[2] for k in kinds} == {True, False}


# ---- the source text and its Python twin --------------------------------------------------------------
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostile_twin")
    src, lib = os.path.join(d, "twin.cpp"), os.path.join(d, "libtwin.so")
    with open(src, "w") as fh:
        fh.write(H.host_twin_source())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib])
    t = C.CDLL(lib)
    pd = C.POINTER(C.c_double)
    t.twin_term.restype, t.twin_term.argtypes = C.c_double, [C.c_double, pd]
    t.twin_literal.restype, t.twin_literal.argtypes = C.c_double, [C.c_double]
    t.twin_vector.restype, t.twin_vector.argtypes = C.c_double, [pd, C.c_uint64, pd]
    return t


def edge_grid(thresholds):
    pts = [0.0, -0.0, H.NAN, H.INF, -H.INF, 1e300, -1e300, 16.0, -16.25, 17.5, -17.5]
    for t in thresholds:
        pts += [t, math.nextafter(t, H.INF), math.nextafter(t, -H.INF)]
    pts += [k / 4.0 for k in range(-70, 71)]  # every step of the plateau, the clamp included
    pts += [math.nextafter(k / 4.0, -H.INF) for k in range(-8, 9)]
    return pts


def test_source_text_agrees_with_its_python_twin(twin):
    rows = sorted({(r.family, r.a, r.b) for r in Cs.NM_ROWS + list(Cs.SANN_ROWS) + list(Cs.HYB_ROWS)
                   + list(Cs.SANN_STREAMED)})
    assert {r[0] for r in rows} == set(H.FAMILY_NAMES)
    for row in rows:
        arr = (C.c_double * 3)(*row)
        grid = edge_grid([row[1], row[2]])
        for xi in grid:
            assert R.same_bits(twin.twin_term(xi, arr), H.term(xi, row)), (row, xi)
        # the numpy form that the reference runs call, against the plain one
        assert all(R.same_bits(a, H.term(xi, row)) for a, xi in zip(H._terms(grid, row), grid)), row
        for lo in range(0, len(grid) - 7, 5):
            pt = grid[lo:lo + 7]
            assert R.same_value(H.family(row)(pt), H.family_plain(row)(pt)), (row, pt)
    grid = edge_grid([2.25, -2.5])
    for xi in grid:
        assert R.same_bits(twin.twin_literal(xi), H.literal_term(xi)), xi
    for lo in range(0, len(grid) - 7, 5):
        assert R.same_value(H.literal(grid[lo:lo + 7]), H.literal_plain(grid[lo:lo + 7]))
    for b in (0.0, 1.0, 2.0, 3.0, 8.0, 64.0):
        arr = (C.c_double * 3)(0.0, b, 0.0)
        for x0 in edge_grid([b / 4.0]):
            for last in (0.3, -0.0, H.NAN, -17.0, 1.0):
                pt = np.array([x0, 0.5, last])
                got = twin.twin_vector(O._ptr(pt), 3, arr)
                assert R.same_bits(got, H.vector((0.0, b, 0.0))(list(pt))), (b, x0, last)
    # the signed zeros really are there
    assert math.copysign(1.0, H.vector((0.0, 2.0, 0.0))([-0.2, 0.0])) == -1.0
    assert math.copysign(1.0, H.vector((0.0, 2.0, 0.0))([0.1, 0.0])) == 1.0


def test_values_do_not_depend_on_the_order_of_the_sum():
    rng = np.random.default_rng(11)
    for row in sorted({(r.family, r.a, r.b) for r in Cs.NM_ROWS}):
        for _ in range(20):
            x = rng.uniform(-20, 20, size=257)
            terms = H._terms(x, row)
            want = H.family(row)(x)
            for _ in range(3):
                acc = 0.0
                for t in rng.permutation(terms):
                    acc = acc + float(t)
                assert R.same_value(acc, want)
            assert R.same_value(R._tree_sum([float(t) for t in terms]), want)


# ---- coverage of the GPU module's case list ------------------------------------------------------------
NM_MUST = ("act:accept", "act:expand", "act:contract_outside", "act:contract_inside", "act:shrink",
           "scan:tied_min", "scan:tied_max", "scan:nan_among_scores", "scan:frozen", "scan:b3_quirk",
           "stop:max_iter", "stop:std_err")


@pytest.mark.parametrize("cls", sorted(Cs.NM_CLASSES))
def test_nelder_mead_cases_reach_every_rule(cls):
    for tree in (True, False):  # the tree order and reference_order=True
        counts = Cs.Counter()
        for b in Cs.nm_batches():
            if b.n in Cs.NM_CLASSES[cls] and b.source == "family":
                counts.update(Cs.total_counts(Cs.nm_reference(b, tree)))
        short = {k: counts[k] for k in NM_MUST if counts[k] < 3}
        assert not short, (cls, tree, short)
    assert any(b.restarts for b in Cs.nm_batches()) and any(not b.minimize for b in Cs.nm_batches())


def test_nelder_mead_stop_verdicts_are_decisive():
    """RefNelderMead asserts a factor of 2 between std_err and eps wherever both are finite and
    positive; here: the runs really do meet an eps that is 0, NaN, negative, inf and positive."""
    seen = set()
    for b in Cs.nm_batches():
        for res, _ in Cs.nm_reference(b, True):
            e = res.eps
            seen.add("nan" if e != e else "inf" if e == H.INF else "zero" if e == 0.0 else
                     "negative" if e < 0.0 else "positive")
    assert seen == {"nan", "inf", "zero", "negative", "positive"}


SANN_MUST = ("accepted_better", "accepted_equal", "accepted_worse", "rejected", "best_taken_equal", "best_kept",
             "diff:nan", "diff:beyond_710t")


@pytest.mark.parametrize("cls", sorted(Cs.SANN_CLASSES))
def test_sann_cases_reach_every_outcome(cls):
    counts = Cs.Counter()
    for b in Cs.sann_batches():
        if b.D in Cs.SANN_CLASSES[cls] and b.source == "family":
            counts.update(Cs.total_counts(Cs.sann_reference(b)))
    short = {k: counts[k] for k in SANN_MUST if counts[k] < 3}
    assert not short, (cls, short)
    if cls != "streamed":
        assert counts["diff:+inf"] + counts["diff:-inf"] >= 3


def test_sann_required_starts():
    b = next(b for b in Cs.sann_batches() if b.name == "D2_min")
    ref = Cs.sann_reference(b)
    for c, row in enumerate(b.rows):
        res, counts = ref[c]
        x0 = Cs.start(row, b.D)
        if row.family == H.ALL_NAN or (row.family == H.NAN_BEYOND and row.x0 > row.a):
            # a NaN start: nothing is ever accepted and x comes back untouched
            assert res.x == x0 and res.f_value != res.f_value
            assert counts["rejected"] == b.max_iter * (b.temp_iter - 1)
        if row.family == H.WALLS and row.x0 < row.a:  # a +inf start
            assert counts["diff:-inf"] >= 1 and counts["diff:nan"] >= 1 and res.f_value < H.INF
        if row.family == H.WALLS and row.a < -1e8:  # reaches -inf; an equal -inf is inf - inf: not taken
            assert res.f_value == -H.INF and counts["diff:nan"] >= 3 and counts["best_taken_equal"] == 0
    for name in ("D2_zero_t", "D130_zero_t", "D1026_zero_t"):
        # t = 0: an equal trial is accepted by `difference <= 0.0` alone, and the NaN point is taken
        b = next(b for b in Cs.sann_batches() if b.name == name)
        ref = Cs.sann_reference(b)
        assert Cs.total_counts(ref)["accepted_equal"] >= 3 * b.max_iter * (b.temp_iter - 1)
        assert all(v != v for v in ref[0][0].x) and ref[0][0].f_value == 0.0
    neg = next(b for b in Cs.sann_batches() if b.name == "D2_negative_t")
    assert Cs.total_counts(Cs.sann_reference(neg))["accepted_worse"] >= 30


HYB_MUST = ("sort:tied_in_simplex", "sort:nan_key", "h2:same", "h2:differs", "act:accept", "act:expand",
            "act:contract_outside", "act:contract_inside", "act:shrink", "stop:max_iter", "stop:std_err")


@pytest.mark.parametrize("cls", sorted(Cs.HYB_CLASSES))
def test_hybrid_cases_reach_every_rule(cls):
    counts = Cs.Counter()
    first_nan = 0
    for b in Cs.hyb_batches():
        if b.n in Cs.HYB_CLASSES[cls] and b.source == "family":
            ref = Cs.hyb_reference(b)
            counts.update(Cs.total_counts(ref))
            # the first particle's initial value is NaN: the H2 counter can never count
            nan_first = [(res, c) for res, c in ref if res.first_value != res.first_value]
            assert all(c["h2:same"] == 0 for _, c in nan_first)
            first_nan += sum(1 for res, _ in nan_first if res.iteration > 0)
    short = {k: counts[k] for k in HYB_MUST if counts[k] < 3}
    assert not short, (cls, short)
    assert first_nan >= 2


def test_hybrid_sees_minus_zero_against_plus_zero():
    """The first particle's value is a zero of one sign and later particles hold zeros of the other:
    the sort must take them for one key and keep the first particle first (a sort by bits would put a
    -0.0 of a later particle ahead of it and return that particle's x), and H2's == counts."""
    counts = Cs.Counter()
    for b in Cs.hyb_batches():
        if b.source == "vector":
            counts.update(Cs.total_counts(Cs.hyb_reference(b)))
    assert counts["sort:plus_zero_before_minus_zero"] >= 3 and counts["h2:same_at_zero"] >= 3
