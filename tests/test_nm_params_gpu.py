"""Run-time objective parameters of Nelder-Mead and the NM/PSO hybrid (CustomObjective(n_params=...),
NMEngine / NMPSOEngine.set_params): start or instance b of a parametrised batch must equal, bit for
bit, a batch-1 engine of the SAME body with row b's numbers baked into its source as literals -- the
path that existed before these engines took parameters. The literals are float.hex() in parentheses
and the bodies let a parameter enter through + - * / only, so the compiler has nothing to fold
differently. For the hybrid the literal engine takes inst_lo = b and the same seed.

Every engine here costs one run-time compilation, which dominates the time: the engines are made
once per module and shared (ENGINES); the second set of rows of the replacement test is a rotation
of the first, so the literal engines serve both.

Shapes, Nelder-Mead: n 2 (one wave), 9 (odd n, three waves, scalar shrink), 16 (128-bit shrink),
128 (the full-row shrink, LDS nearly full), 130 (two chunks per lane, simplex in global memory).
Hybrid: n 2, 9, 33 (packed kernel), 130 (wide kernel)."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3
SEED = 12374563468
STATUS_FIELDS = ("f_value", "iteration", "function_calls_used", "gradient_evals_used", "hessian_evals_used",
                 "best_index", "val_no_change", "std_err", "done", "reserved")


@pytest.fixture(scope="module")
def m():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def status_tuple(st, b=0):
    """every Status field, the two doubles as their bit patterns. best_index is the start's index
    in its own batch: b in the parametrised batch, 0 in the literal batch of one, so it is taken
    relative to the start."""
    out = []
    for f in STATUS_FIELDS:
        v = getattr(st, f)
        if f in ("f_value", "std_err"):
            out.append(int(np.float64(v).view(np.uint64)))
        elif f == "best_index":
            out.append(int(v) - b)
        else:
            out.append(int(v))
    return tuple(out)


def lit(v):
    return "(" + float(v).hex() + ")"


# ---- the objectives: p(k) and their twins with literals ---------------------------------------------
def n_params_of(form, D):
    if form.startswith("ends"):
        return int(form[4:])
    if form.startswith("cends"):
        return int(form[5:])
    return {"terms": 3, "chain": 2, "vector": 2 * D, "one": 1, "chain1": 1, "chain3": 3}[form]


def body(form, D, row=None):
    """row None: the parametrised body; else the same body with row's values as literals"""
    P = (lambda k: f"p({k})") if row is None else (lambda k: lit(row[k]))
    if form == "terms":
        return f"double r = xi - {P(0)}; return {P(1)} * r * r + r / {P(2)};"
    if form == "chain":
        return f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; return t1 * t1 + {P(1)} * t2 * t2;"
    if form == "chain1":
        return f"double t1 = 1 - xi, t2 = xn - xi * xi; return t1 * t1 + {P(0)} * t2 * t2;"
    if form == "chain3":
        return (f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; "
                f"return t1 * t1 + {P(1)} * t2 * t2 + t1 / {P(2)};")
    if form == "one":
        return f"double r = xi - {P(0)}; return r * r;"
    if form.startswith("ends"):
        return f"double r = xi - {P(0)}; return {P(n_params_of(form, D) - 1)} * r * r;"
    if form.startswith("cends"):  # the chain form with its two parameters at the ends of a long row
        return (f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; "
                f"return t1 * t1 + {P(n_params_of(form, D) - 1)} * t2 * t2;")
    assert form == "vector"
    if row is None:
        return "return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return p(D + i) * r * r; });"
    table = ", ".join(lit(v) for v in row)
    return (f"const double q[{2 * D}] = {{{table}}}; "
            "return x.sum([&](double xi, uint64_t i) { double r = xi - q[i]; return q[D + i] * r * r; });")


def objective(m, form, D, row=None):
    return m.CustomObjective(body(form, D, row), chain=form.startswith(("chain", "cends")), vector=form == "vector",
                             n_params=n_params_of(form, D) if row is None else 0)


def rows_for(form, D, salt=0):
    """[B, n_params]: distinct rows, weights positive, divisors away from zero"""
    rng = np.random.default_rng(2000 + 17 * D + salt)
    n = n_params_of(form, D)
    if form == "vector":
        return np.concatenate([rng.uniform(-1.0, 1.0, (B, D)), rng.uniform(0.5, 2.0, (B, D))], axis=1)
    if form.startswith("ends"):
        return np.concatenate([rng.uniform(-1.0, 1.0, (B, n - 1)), rng.uniform(0.5, 2.0, (B, 1))], axis=1)
    if form.startswith("cends"):
        return np.concatenate([rng.uniform(0.5, 1.5, (B, 1)), rng.uniform(-1.0, 1.0, (B, n - 2)),
                               rng.uniform(50.0, 150.0, (B, 1))], axis=1)
    if form == "chain":
        return np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(50.0, 150.0, B)], axis=1)
    if form == "chain1":
        return rng.uniform(50.0, 150.0, (B, 1))
    if form == "chain3":
        return np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(50.0, 150.0, B), rng.uniform(2.0, 4.0, B)], axis=1)
    return rng.uniform(0.5, 3.0, (B, n))


def x0_for(D):
    return np.stack([(0.6 + 0.5 * b) * (1.0 + 0.001 * np.arange(D)) for b in range(B)])


def bounds_for(D):
    """(upper, lower) [D], shared by the batch as the engines take them; they cut into the path"""
    hi = 1.9 * (1.0 + 0.01 * np.arange(D))
    return hi, -0.25 * hi


# ---- engines, made once ------------------------------------------------------------------------------
@contextlib.contextmanager
def engines(m):
    """(kind, form, D, extra, row or None[, b]) -> engine; closed when the module is done"""
    made = {}

    def get(kind, form, D, extra=(), row=None, b=0):
        key = (kind, form, D, tuple(extra), None if row is None else tuple(float(v) for v in row),
               b if kind == "hyb" else 0)
        if key not in made:
            obj = objective(m, form, D, row)
            batch = B if row is None else 1
            if kind == "nm":
                made[key] = m.NMEngine(obj, batch, D, **dict(extra))
            else:
                made[key] = m.NMPSOEngine(obj, batch, D, seed=SEED, inst_lo=0 if row is None else b,
                                          **dict(extra))
        return made[key]

    try:
        yield get
    finally:
        for eng in made.values():
            eng.close()


@pytest.fixture(scope="module")
def ENGINES(m):
    """engines(m), made once for the module"""
    with engines(m) as get:
        yield get


def solve(eng, kind, D, x0, bounded, params=None):
    """(x, [status tuples relative to the start]) of one solve"""
    hi, lo = bounds_for(D) if bounded else (None, None)
    if kind == "nm":
        x, sts, _ = eng.minimize(x0.copy(), hi, lo, params=params)
    else:
        x, sts = eng.minimize(x0.copy(), lo, hi, params=params)
    return x, sts


def assert_matches_baked(ENGINES, kind, form, D, extra, rows, x0=None, get=None):
    """the parametrised engine under `rows` against the literal engines of each row"""
    get = get or ENGINES
    bounded = dict(extra).get("bounded", False)
    x0 = x0_for(D) if x0 is None else x0
    par = get(kind, form, D, extra)
    x, sts = solve(par, kind, D, x0, bounded, rows)
    got = [status_tuple(s, b) for b, s in enumerate(sts)]
    for b in range(B):
        baked = get(kind, form, D, extra, rows[b], b)
        xb, sb = solve(baked, kind, D, x0[b:b + 1], bounded)
        tag = f"{kind} {form} n {D} {dict(extra)}, start {b}"
        assert same(x[b], xb[0]), tag
        assert got[b] == status_tuple(sb[0]), tag
    return x, got


# ---- 1. start b is the literal engine of row b -------------------------------------------------------
REF, TREE = (("reference_order", True),), ()


def nm_extra(order, max_iter, **kw):
    return tuple(sorted(dict(dict(order), max_iter=max_iter, **kw).items()))


# n = 128 replaces every vertex once before its first shrink (about 126 iterations from these starts, by
# the CPU oracle's count of evaluations): the cases that must shrink run that long and do not stop on an
# unchanged best. An iteration there is microseconds; the time is the four compilations, as everywhere.
LONG = dict(no_change_best_tol=1000)
NM_CASES = [
    ("terms", 2, nm_extra(TREE, 40)), ("chain", 2, nm_extra(REF, 40)),
    ("terms", 9, nm_extra(REF, 40, bounded=True)), ("chain", 9, nm_extra(TREE, 40)),
    ("chain", 9, nm_extra(REF, 40)), ("vector", 9, nm_extra(TREE, 30, minimize=False)),
    ("chain", 16, nm_extra(TREE, 30)),
    ("chain", 16, nm_extra(REF, 30, restarts=1)),
    ("chain", 128, nm_extra(TREE, 160, **LONG)), ("chain", 128, nm_extra(REF, 160, **LONG)),
    ("vector", 128, nm_extra(TREE, 8)),
    ("terms", 130, nm_extra(TREE, 8)), ("chain", 130, nm_extra(REF, 8)),
]
# the cases whose shrink (and the rescoring of every row behind it) the third test pins
SHRINK_CASES = [c for c in NM_CASES if c[0] == "chain" and c[1] in (9, 16, 128) and not dict(c[2]).get("restarts")]


def case_id(c):
    return f"{c[0]}-n{c[1]}" + "".join(f"-{k}{int(v)}" for k, v in c[2])


@pytest.mark.parametrize("form,D,extra", NM_CASES, ids=[case_id(c) for c in NM_CASES])
def test_nm_starts_equal_the_literal_engines(ENGINES, form, D, extra):
    x, sts = assert_matches_baked(ENGINES, "nm", form, D, extra, rows_for(form, D))
    assert len(set(sts)) == B  # the rows and starts do tell the solves apart
    if not dict(extra).get("restarts"):
        assert all(0 < s[1] <= dict(extra)["max_iter"] for s in sts)


# ---- 2. the phase-per-barrier kernel -----------------------------------------------------------------
def test_nm_without_the_driver_wave(m, monkeypatch):
    """NLSG_NM_DRIVER=0 is read when an engine is made: nm_solve_kernel<., 1> at n <= 128"""
    monkeypatch.setenv("NLSG_NM_DRIVER", "0")
    made = {}

    def get(kind, form, D, extra=(), row=None, b=0):
        key = None if row is None else tuple(row)
        if key not in made:
            made[key] = m.NMEngine(objective(m, form, D, row), B if row is None else 1, D, **dict(extra))
        return made[key]

    try:
        for order in (TREE, REF):
            made.clear()
            x, sts = assert_matches_baked(None, "nm", "chain", 9, nm_extra(order, 30), rows_for("chain", 9), get=get)
            assert len(set(sts)) == B
            for eng in made.values():
                eng.close()
    finally:
        for eng in made.values():
            eng.close()


# ---- 3. the shrink path is on the road ---------------------------------------------------------------
@pytest.mark.parametrize("form,D,extra", SHRINK_CASES, ids=[case_id(c) for c in SHRINK_CASES])
def test_the_cases_shrink(ENGINES, form, D, extra):
    """a case that never shrinks does not test the rescoring (nm_shrink_rows*, nm_rescore_lanes):
    the literal engines' own phase counters say that these do"""
    rows, x0 = rows_for(form, D), x0_for(D)
    shrinks = [int(ENGINES("nm", form, D, extra, rows[b]).phase_cycles(x0[b:b + 1])[0, 7]) for b in range(B)]
    assert max(shrinks) > 0, shrinks
    par = ENGINES("nm", form, D, extra)
    par.set_params(rows)
    assert [int(v) for v in par.phase_cycles(x0)[:, 7]] == shrinks


# ---- 4. alignment ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["chain1", "chain3"])
def test_an_odd_row_keeps_the_simplex_rows_aligned(ENGINES, form):
    """n_params 1 and 3 in front of the n = 16 simplex, whose shrink moves a lane's pair with one
    128-bit LDS access: the row is padded to 16 bytes"""
    extra = nm_extra(TREE, 30)
    rows = rows_for(form, 16)
    assert_matches_baked(ENGINES, "nm", form, 16, extra, rows)
    x0 = x0_for(16)
    assert max(int(ENGINES("nm", form, 16, extra, rows[b]).phase_cycles(x0[b:b + 1])[0, 7]) for b in range(B)) > 0


# ---- 5. the budget's edge ----------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["1", "0"], ids=["driver-wave", "phase-kernel"])
def test_fewer_term_buffers_than_waves(m, monkeypatch, driver):
    """n = 128 in reference order with 2048 parameters, read at both ends: 16 KiB of the 22 KiB behind
    the image, so 6 of the 16 waves have a term buffer. In the phase-per-barrier kernel (NLSG_NM_DRIVER=0)
    those waves alone rescore a shrink, a row at a time; each row's sum is a serial chain, so the bits
    do not change -- and the cases do shrink."""
    monkeypatch.setenv("NLSG_NM_DRIVER", driver)
    assert m.NMEngine.fits(128, True, 2048)
    form, D, extra = "cends2048", 128, nm_extra(REF, 160, **LONG)
    rows, x0 = rows_for(form, D), x0_for(D)
    made = {}

    def get(kind, form, D, extra=(), row=None, b=0):
        key = None if row is None else tuple(row)
        if key not in made:
            made[key] = m.NMEngine(objective(m, form, D, row), B if row is None else 1, D, **dict(extra))
        return made[key]

    try:
        x, sts = assert_matches_baked(None, "nm", form, D, extra, rows, get=get)
        assert len(set(sts)) == B
        assert max(int(get("nm", form, D, extra, rows[b]).phase_cycles(x0[b:b + 1])[0, 7]) for b in range(B)) > 0
    finally:
        for eng in made.values():
            eng.close()


@pytest.mark.parametrize("ref", [False, True], ids=["tree", "reference"])
def test_the_largest_row_that_fits(m, ENGINES, ref):
    NM = m.NMEngine
    most = max(k for k in range(1, 4097) if NM.fits(128, ref, k))
    form, extra = f"ends{most}", nm_extra(REF if ref else TREE, 6)
    rows, x0 = rows_for(form, 128), x0_for(128)
    x, sts, _ = ENGINES("nm", form, 128, extra).minimize(x0.copy(), params=rows)
    assert all(np.isfinite(s.f_value) and s.iteration > 0 for s in sts)
    xb, sb, _ = ENGINES("nm", form, 128, extra, rows[1]).minimize(x0[1:2].copy())
    assert same(x[1], xb[0]) and status_tuple(sts[1], 1) == status_tuple(sb[0])
    with pytest.raises(m.NlsgError) as ei:
        NM(objective(m, f"ends{most + 2}", 128), B, 128, **dict(extra))
    assert ei.value.code == 2 and "163840" in str(ei.value)


# ---- 6. the hybrid -----------------------------------------------------------------------------------
def hyb_extra(max_iter, **kw):
    return tuple(sorted(dict(max_iter=max_iter, **kw).items()))


HYB_CASES = [("terms", 2, hyb_extra(30)), ("chain", 9, hyb_extra(30, bounded=True)),
             ("vector", 33, hyb_extra(20)), ("chain", 33, hyb_extra(20, minimize=False)),
             ("terms", 130, hyb_extra(5)), ("ends4096", 2, hyb_extra(30))]


@pytest.mark.parametrize("form,D,extra", HYB_CASES, ids=[case_id(c) for c in HYB_CASES])
def test_hybrid_instances_equal_the_literal_engines(ENGINES, form, D, extra):
    x, sts = assert_matches_baked(ENGINES, "hyb", form, D, extra, rows_for(form, D))
    assert len(set(sts)) == B
    assert all(s[1] > 0 for s in sts)


# ---- 6b. the widest shapes with the largest row ------------------------------------------------------
@pytest.mark.parametrize("kind", ["nm", "hyb"])
def test_the_widest_shape_with_the_largest_row(m, ENGINES, kind):
    """n = 1024 (eight chunks per lane) with 4096 parameters: the largest static row in front of the
    largest dynamic block of either engine (the hybrid's view is 123 008 bytes there); start 1 against
    its literal twin"""
    D, form = 1024, "ends4096"
    extra = nm_extra(REF, 3) if kind == "nm" else hyb_extra(2)
    assert (m.NMEngine.fits(D, True, 4096) if kind == "nm" else m.NMPSOEngine.fits(D, 4096))
    rows, x0 = rows_for(form, D), x0_for(D)
    x, sts = solve(ENGINES(kind, form, D, extra), kind, D, x0, False, rows)
    xb, sb = solve(ENGINES(kind, form, D, extra, rows[1], 1), kind, D, x0[1:2], False)
    assert same(x[1], xb[0]) and status_tuple(sts[1], 1) == status_tuple(sb[0])
    assert sts[1].iteration > 0


# ---- 7. replacement without a rebuild ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nm", "hyb"])
def test_rows_are_replaced_without_a_rebuild(ENGINES, kind):
    """one engine: rows A, A rotated, A again; the rotation's literal engines are A's"""
    form, D, extra = ("terms", 9, nm_extra(REF, 40, bounded=True)) if kind == "nm" else ("terms", 2, hyb_extra(30))
    A = rows_for(form, D)
    first = assert_matches_baked(ENGINES, kind, form, D, extra, A)
    if kind == "nm":
        second = assert_matches_baked(ENGINES, kind, form, D, extra, np.roll(A, 1, axis=0))
    else:  # (a literal hybrid engine is tied to its instance index: the rotated rows have no twins)
        second = solve(ENGINES(kind, form, D, extra), kind, D, x0_for(D), False, np.roll(A, 1, axis=0))
    assert not same(first[0], second[0])
    again = assert_matches_baked(ENGINES, kind, form, D, extra, A)
    assert same(first[0], again[0]) and first[1] == again[1]


# ---- 8. independence ---------------------------------------------------------------------------------
def test_permuting_starts_and_rows_permutes_the_results(ENGINES):
    """(Nelder-Mead only: a hybrid instance's draws are keyed by its index in the batch)"""
    form, D, extra = "chain", 9, nm_extra(TREE, 40)
    eng, rows, x0 = ENGINES("nm", form, D, extra), rows_for(form, D), x0_for(D)
    perm = [2, 0, 1]
    x, sts = solve(eng, "nm", D, x0, False, rows)
    xp, stsp = solve(eng, "nm", D, x0[perm], False, rows[perm])
    assert same(xp, x[perm])
    got = [status_tuple(s, b) for b, s in enumerate(sts)]
    assert [status_tuple(s, b) for b, s in enumerate(stsp)] == [got[i] for i in perm]
    assert len(set(got)) == B


# ---- 10. meaning -------------------------------------------------------------------------------------
def test_the_value_is_the_rows_function_of_the_returned_point(ENGINES):
    """reference order, terms at n = 9: f is the terms of the returned point added in index order"""
    form, D, extra = "terms", 9, nm_extra(REF, 40, bounded=True)
    rows, x0 = rows_for(form, D), x0_for(D)
    hi, lo = bounds_for(D)

    def value(x, row):
        p0, p1, p2 = (float(v) for v in row)
        acc = 0.0
        for xi in (float(v) for v in x):
            r = xi - p0
            acc = acc + (p1 * r * r + r / p2)
        return acc

    for b in range(B):  # the literal engines first: the rule itself, on the path that predates parameters
        xb, sb, _ = ENGINES("nm", form, D, extra, rows[b]).minimize(x0[b:b + 1].copy(), hi, lo)
        assert sb[0].f_value == value(xb[0], rows[b]), f"literal engine, start {b}"
    x, sts, _ = ENGINES("nm", form, D, extra).minimize(x0.copy(), hi, lo, params=rows)
    for b in range(B):
        assert sts[b].f_value == value(x[b], rows[b]), f"start {b}"


# ---- 11. one line fit per series ---------------------------------------------------------------------
def test_a_line_fit_per_series(m):
    K = 24
    obj = m.CustomObjective(f"double s = 0.0; for (int k = 0; k < {K}; k++) {{ double r = p(k) - (x(0) + x(1) * k); "
                            "s = s + r * r; } return s;", vector=True, n_params=K)
    rng = np.random.default_rng(7)
    truth = np.array([[1.0, 0.5], [-2.0, 0.25], [0.5, -0.75]])
    rows = truth[:, :1] + truth[:, 1:] * np.arange(K) + rng.normal(0.0, 0.05, (B, K))

    def value(x, row):
        s = 0.0
        for k in range(K):
            r = float(row[k]) - (float(x[0]) + float(x[1]) * k)
            s = s + r * r
        return s

    x = np.zeros((B, 2)) + [[0.1, 0.1], [0.2, -0.1], [-0.1, 0.2]]
    x0 = x.copy()
    sts = m.NelderMead(obj, max_iter=200, params=rows).minimize(x)
    for b in range(B):
        assert sts[b].f_value == value(x[b], rows[b]), f"series {b}"
        assert sts[b].f_value < value(x0[b], rows[b])
    assert len({tuple(bits(x[b])) for b in range(B)}) == B


# ---- 12. state ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nm", "hyb"])
def test_call_order(m, kind):
    from nlsolver_amd import _capi
    Engine = m.NMEngine if kind == "nm" else m.NMPSOEngine
    x0 = x0_for(2)
    with Engine(objective(m, "one", 2), B, 2) as eng:
        calls = [lambda: eng.minimize(x0.copy()), lambda: eng.time_solve(x0)]
        if kind == "nm":
            calls.append(lambda: eng.phase_cycles(x0))
        for call in calls:
            with pytest.raises(m.NlsgError) as ei:
                call()
            assert ei.value.code == 6
        eng.set_params(rows_for("one", 2))
        eng.minimize(x0.copy())
    name = "nlsg_nm_set_params" if kind == "nm" else "nlsg_nmpso_set_params"
    for plain in ("rosenbrock", objective(m, "one", 2, [1.5])):
        with Engine(plain, B, 2) as eng:
            with pytest.raises(m.NlsgError) as ei:
                eng.set_params(np.zeros((B, 1)))
            assert ei.value.code == 1
            row = np.zeros(B)
            assert getattr(_capi.lib(), name)(eng._h, row.ctypes.data_as(_capi.pd)) == 1


# ---- 13. / 14. the drop-in classes and the C++ header ------------------------------------------------
DROP_ROW = (1.25, 2.5, 3.5)


@pytest.fixture(scope="module")
def drop_ins(m):
    """{("nm" | "nmpso", "params" | "baked"): (x, Status)} for x0 = (5, 7)"""
    out = {}
    for how in ("params", "baked"):
        obj = objective(m, "terms", 2, None if how == "params" else DROP_ROW)
        kw = dict(params=DROP_ROW) if how == "params" else {}
        for kind, solver in (("nm", m.NelderMead(obj, **kw)), ("nmpso", m.NelderMeadPSO(obj, m.XorShift(), **kw))):
            x = np.array([5.0, 7.0])
            out[kind, how] = (x, solver.minimize(x))
    return out


@pytest.mark.parametrize("kind", ["nm", "nmpso"])
def test_drop_in_with_params_equals_the_literal_objective(drop_ins, kind):
    (xp, sp), (xb, sb) = drop_ins[kind, "params"], drop_ins[kind, "baked"]
    assert same(xp, xb) and status_tuple(sp) == status_tuple(sb)
    assert sp.iteration > 0 and sp.done == 1


def test_drop_in_shows_one_row_to_every_start(m, drop_ins):
    obj = objective(m, "terms", 2)
    x = np.array([[5.0, 7.0], [5.0, 7.0]])
    sts = m.NelderMead(obj, params=DROP_ROW).minimize(x)
    xp, sp = drop_ins["nm", "params"]
    assert same(x[0], xp) and same(x[1], xp) and status_tuple(sts[1], 1) == status_tuple(sp)
    with pytest.raises(ValueError):
        m.NelderMead(obj, params=[DROP_ROW] * 3).minimize(x)


def test_header_params_equal_the_drop_ins(drop_ins, tmp_path):
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_nm_params")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_nm_params.cpp"), "-o", exe, "-ldl"])
    row = [float(v).hex() for v in DROP_ROW]
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    got = json.loads(subprocess.check_output([exe] + row, env=env, text=True, timeout=300))
    for kind in ("nm", "nmpso"):
        x, st = drop_ins[kind, "params"]
        g = got[kind]
        assert same([float.fromhex(v) for v in g["x"]], x), kind
        assert bits(float.fromhex(g["f"])) == bits(st.f_value), kind
        assert (g["iters"], g["fcalls"]) == (st.iteration, st.function_calls_used), kind
