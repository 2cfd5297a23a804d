"""Run-time objective parameters of the resident batch engines (CustomObjective(n_params=...),
DEBatchEngine / PSOBatchEngine.set_params): solve b of a parametrised batch must equal, bit for bit,
a batch-1 engine of the SAME objective with row b's numbers baked into its source as literals -- the
path that existed before parameters did. The literals are float.hex() in parentheses, and the bodies
let a parameter enter through + - * / only, so the compiler has nothing to fold differently.

Every engine here costs one run-time compilation, which dominates the time: the engines are made
once per module and shared (ENGINES), and the second set of rows of the replacement test is a
rotation of the first, so the literal engines serve both.

Shapes are one per lane mapping that can differ: D 2 (4 lanes per agent), D 9 (8 lanes, odd D), D 65
(one wave per agent); pop / particles 8, 12, 6 -- no multiple of the agents per pass."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 12374563468
B = 3
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


def status_tuple(st):
    """every Status field, the two doubles as their bit patterns"""
    return tuple(int(np.float64(getattr(st, f)).view(np.uint64)) if f in ("f_value", "std_err")
                 else int(getattr(st, f)) for f in STATUS_FIELDS)


def lit(v):
    return "(" + float(v).hex() + ")"


# ---- the objectives: p(k) and their twins with literals ---------------------------------------------
def n_params_of(form, D):
    return {"terms": 3, "chain": 2, "vector": 2 * D, "one": 1, "ends": 4096}[form]


def body(form, D, row=None):
    """row None: the parametrised body; else the same body with row's values as literals"""
    P = (lambda k: f"p({k})") if row is None else (lambda k: lit(row[k]))
    if form == "terms":
        return f"double r = xi - {P(0)}; return {P(1)} * r * r + r / {P(2)};"
    if form == "chain":
        return f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; return t1 * t1 + {P(1)} * t2 * t2;"
    if form == "one":
        return f"double r = xi - {P(0)}; return r * r;"
    if form == "ends":
        return f"double r = xi - {P(0)}; return {P(4095)} * r * r;"
    assert form == "vector"
    if row is None:
        return "return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return p(D + i) * r * r; });"
    table = ", ".join(lit(v) for v in row)
    return (f"const double q[{2 * D}] = {{{table}}}; "
            "return x.sum([&](double xi, uint64_t i) { double r = xi - q[i]; return q[D + i] * r * r; });")


def objective(m, form, D, row=None):
    return m.CustomObjective(body(form, D, row), chain=form == "chain", vector=form == "vector",
                             n_params=n_params_of(form, D) if row is None else 0)


def rows_for(form, D, salt=0):
    """[B, n_params]: distinct rows, weights positive, divisors away from zero"""
    rng = np.random.default_rng(1000 + 17 * D + salt)
    n = n_params_of(form, D)
    if form == "vector":
        return np.concatenate([rng.uniform(-1.0, 1.0, (B, D)), rng.uniform(0.5, 2.0, (B, D))], axis=1)
    if form == "ends":
        return np.concatenate([rng.uniform(-1.0, 1.0, (B, n - 1)), rng.uniform(0.5, 2.0, (B, 1))], axis=1)
    if form == "chain":
        return np.stack([rng.uniform(0.5, 1.5, B), rng.uniform(50.0, 150.0, B)], axis=1)
    return rng.uniform(0.5, 3.0, (B, n))


def seeds_for(salt=0):
    return [SEED0 + 7919 * b + 104729 * salt for b in range(B)]


def x0_for(D):
    return np.stack([(0.6 + 0.5 * b) * (1.0 + 0.001 * np.arange(D)) for b in range(B)])


def bounds_for(D):
    hi = np.stack([(2.0 + 0.25 * b) * (1.0 + 0.01 * np.arange(D)) for b in range(B)])
    return -0.5 * hi, hi


# ---- engines, made once ------------------------------------------------------------------------------
DE_ARGS = dict(CR=0.9, F=0.8, eps=10e-4, max_iter=40, best_val_no_change=50)
PSO_ARGS = dict(eps=10e-4, max_iter=40, best_val_no_change=50)


@contextlib.contextmanager
def engines(m):
    """(kind, form, n, D, extra, row or None, batch) -> engine; closed when the module is done"""
    made = {}

    def get(kind, form, n, D, extra=(), row=None):
        key = (kind, form, n, D, tuple(extra), None if row is None else tuple(float(v) for v in row))
        if key not in made:
            obj = objective(m, form, D, row)
            batch = B if row is None else 1
            if kind == "de":
                made[key] = m.DEBatchEngine(obj, batch, n, D, **dict(DE_ARGS, **dict(extra)))
            else:
                made[key] = m.PSOBatchEngine(obj, batch, n, D, **dict(PSO_ARGS, **dict(extra)))
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


def inputs(kind, D, salt=0):
    """the per-solve inputs besides the parameters: (x0, seeds) or (lower, upper, seeds)"""
    if kind == "de":
        return (x0_for(D), seeds_for(salt))
    lo, hi = bounds_for(D)
    return (lo, hi, seeds_for(salt))


def one(args, b):
    """solve b's inputs, shaped for a batch of one"""
    return tuple(a[b:b + 1] for a in args)


def solve(eng, args, params=None):
    x, sts = eng.minimize(*args, params=params)
    return x, [status_tuple(s) for s in sts]


def state_after(eng, args, b, turns):
    eng.init(*args)
    eng.step(turns)
    return [a for a in eng.download(b) if a is not None]


def assert_matches_baked(ENGINES, kind, form, n, D, extra, rows, salt=0, steps=True):
    """the parametrised engine under `rows` against the literal engines of each row"""
    par = ENGINES(kind, form, n, D, extra)
    args = inputs(kind, D, salt)
    par.set_params(rows)
    if steps:
        got = []
        par.init(*args)
        par.step(5)
        for b in range(B):
            got.append([a for a in par.download(b) if a is not None])
    x, sts = solve(par, args)
    for b in range(B):
        baked = ENGINES(kind, form, n, D, extra, rows[b])
        tag = f"{kind} {form} n {n} D {D}, solve {b}"
        if steps:
            want = state_after(baked, one(args, b), 0, 5)
            assert len(want) == len(got[b]) and all(same(u, v) for u, v in zip(got[b], want)), tag
        xb, sb = solve(baked, one(args, b))
        assert same(x[b], xb[0]), tag
        assert sts[b] == sb[0], tag
    return x, sts


# ---- 1. solve b is the literal engine of row b ------------------------------------------------------
DE_CASES = [("terms", 8, 2, ()), ("terms", 12, 9, ()), ("terms", 6, 65, ()),
            ("chain", 12, 9, (("minimize", False),)), ("vector", 8, 2, (("strategy", 0),)),
            ("vector", 6, 65, ())]
# (type 0 = Vanilla, 1 = Accelerated)
PSO_CASES = [("terms", 8, 2, (("type", 0),)), ("terms", 12, 9, (("type", 1), ("bounded", True))),
             ("terms", 6, 65, (("type", 0), ("bounded", True))),
             ("chain", 12, 9, (("type", 0), ("bounded", True), ("minimize", False))),
             ("vector", 8, 2, (("type", 1),)), ("vector", 6, 65, (("type", 0),))]


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}" + "".join(f"-{k}{int(v)}" for k, v in c[3])


@pytest.mark.parametrize("form,n,D,extra", DE_CASES, ids=[case_id(c) for c in DE_CASES])
def test_de_solves_equal_the_literal_engines(ENGINES, form, n, D, extra):
    x, sts = assert_matches_baked(ENGINES, "de", form, n, D, extra, rows_for(form, D))
    assert len({s for s in sts}) == B  # the rows and seeds do tell the solves apart


@pytest.mark.parametrize("form,n,D,extra", PSO_CASES, ids=[case_id(c) for c in PSO_CASES])
def test_pso_solves_equal_the_literal_engines(ENGINES, form, n, D, extra):
    x, sts = assert_matches_baked(ENGINES, "pso", form, n, D, extra, rows_for(form, D))
    assert len({s for s in sts}) == B


# ---- 2. odd and minimal sizes ------------------------------------------------------------------------
def test_pso_one_parameter_keeps_the_rows_aligned(ENGINES):
    """n_params 1 (and 3, in the cases above) in front of an even-stride swarm: the row is padded to 16
    bytes, or the swarm's 16-byte accesses would sit on odd doubles"""
    assert_matches_baked(ENGINES, "pso", "one", 8, 2, (("type", 0),), rows_for("one", 2))


@pytest.mark.parametrize("kind", ["de", "pso"])
def test_the_largest_row(ENGINES, kind):
    """4096 parameters (32 KiB of the workgroup's LDS), read at both ends"""
    assert_matches_baked(ENGINES, kind, "ends", 8, 2, (), rows_for("ends", 2), steps=False)


# ---- 3. launch cuts: the row is staged again by every launch -----------------------------------------
@pytest.mark.parametrize("kind", ["de", "pso"])
def test_launch_cuts_change_nothing(ENGINES, kind):
    rows, args = rows_for("terms", 2), inputs(kind, 2)
    whole = solve(ENGINES(kind, "terms", 8, 2, () if kind == "de" else (("type", 0),)), args, rows)
    extra = (("turns_per_launch", 3),) + (() if kind == "de" else (("type", 0),))
    cut = solve(ENGINES(kind, "terms", 8, 2, extra), args, rows)
    assert same(whole[0], cut[0]) and whole[1] == cut[1]
    assert max(s[1] for s in whole[1]) > 3  # more than one launch of three turns


# ---- 4. replacement without a rebuild ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["de", "pso"])
def test_rows_are_replaced_without_a_rebuild(ENGINES, kind):
    """one engine: set_params(A), minimize, set_params(B), minimize; B = A rotated, so that the literal
    engines of A's rows are B's too (with other seeds and starts)"""
    extra = () if kind == "de" else (("type", 1), ("bounded", True))
    A = rows_for("terms", 9)
    Bq = np.roll(A, 1, axis=0)
    first = assert_matches_baked(ENGINES, kind, "terms", 12, 9, extra, A, steps=False)
    second = assert_matches_baked(ENGINES, kind, "terms", 12, 9, extra, Bq, steps=False)
    assert not same(first[0], second[0])
    again = assert_matches_baked(ENGINES, kind, "terms", 12, 9, extra, A, steps=False)
    assert same(first[0], again[0]) and first[1] == again[1]


# ---- 5. independence ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["de", "pso"])
def test_permuting_the_solves_permutes_the_results(ENGINES, kind):
    eng = ENGINES(kind, "terms", 8, 2, () if kind == "de" else (("type", 0),))
    rows, args = rows_for("terms", 2), inputs(kind, 2)
    perm = [2, 0, 1]
    x, sts = solve(eng, args, rows)
    args_p = tuple([a[i] for i in perm] if isinstance(a, list) else a[perm] for a in args)
    xp, stsp = solve(eng, args_p, rows[perm])
    assert same(xp, x[perm]) and stsp == [sts[i] for i in perm]
    assert len(set(sts)) == B


# ---- 6. meaning --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["de", "pso"])
def test_the_value_is_the_rows_function_of_the_returned_point(ENGINES, kind):
    """terms at D = 2: both terms live in lane 0 and are added in order, (0.0 + t0) + t1"""
    eng = ENGINES(kind, "terms", 8, 2, () if kind == "de" else (("type", 0),))
    rows = rows_for("terms", 2)
    x, sts = eng.minimize(*inputs(kind, 2), params=rows)
    for b in range(B):
        p0, p1, p2 = (float(v) for v in rows[b])
        t = []
        for xi in (float(x[b, 0]), float(x[b, 1])):
            r = xi - p0
            t.append(p1 * r * r + r / p2)
        assert sts[b].f_value == (0.0 + t[0]) + t[1], f"solve {b}"


# ---- 7. state ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["de", "pso"])
def test_call_order(m, kind):
    from nlsolver_amd import _capi
    obj = objective(m, "one", 2)
    make = (lambda o: m.DEBatchEngine(o, B, 8, 2)) if kind == "de" else (lambda o: m.PSOBatchEngine(o, B, 8, 2))
    args = inputs(kind, 2)
    with make(obj) as eng:
        for call in (lambda: eng.init(*args), lambda: eng.minimize(*args), lambda: eng.time_solve(*args)):
            with pytest.raises(m.NlsgError) as ei:
                call()
            assert ei.value.code == 6
        eng.set_params(rows_for("one", 2))
        eng.init(*args)
    with make("rosenbrock") as eng:
        with pytest.raises(m.NlsgError) as ei:
            eng.set_params(np.zeros((B, 1)))
        assert ei.value.code == 1
        row = np.zeros(B)
        rc = getattr(_capi.lib(), f"nlsg_{kind}_batch_set_params")(eng._h, row.ctypes.data_as(_capi.pd))
        assert rc == 1


# ---- 8. / 9. the drop-in classes and the C++ header --------------------------------------------------
DROP_ROW = (1.25, 2.5, 3.5)


@pytest.fixture(scope="module")
def drop_ins(m):
    """{("de" | "pso", "params" | "baked"): (x, Status, driver_used)} for x0 = (5, 7)"""
    out = {}
    for how in ("params", "baked"):
        obj = objective(m, "terms", 2, None if how == "params" else DROP_ROW)
        kw = dict(params=DROP_ROW) if how == "params" else dict(driver="resident")
        for kind, solver in (("de", m.DE(obj, m.XorShift(), 0.9, 0.8, 10e-4, 40, **kw)),
                             ("pso", m.PSO(obj, m.XorShift(), 0.8, 1.8, 1.8, 10, 300, **kw))):
            x = np.array([5.0, 7.0])
            st = solver.minimize(x)
            out[kind, how] = (x, st, solver.driver_used)
    return out


@pytest.mark.parametrize("kind", ["de", "pso"])
def test_drop_in_with_params_equals_the_literal_objective(drop_ins, kind):
    (xp, sp, dp), (xb, sb, db) = drop_ins[kind, "params"], drop_ins[kind, "baked"]
    assert dp == "resident" and db == "resident"  # the default driver "turns" does not apply to params
    assert same(xp, xb) and status_tuple(sp) == status_tuple(sb)
    assert sp.iteration > 0 and sp.done == 1


def test_drop_in_rejects_a_shape_that_does_not_fit(m):
    obj = objective(m, "terms", 128)
    with pytest.raises(m.NlsgError) as ei:
        m.DE(obj, None, pop_size=1024, params=DROP_ROW).minimize(np.ones(128))
    assert ei.value.code == 2
    with pytest.raises(m.NlsgError) as ei:
        m.PSO(obj, None, n_particles=1024, params=DROP_ROW).minimize(np.ones(128))
    assert ei.value.code == 2
    with pytest.raises(m.NlsgError) as ei:   # an engine without parameters says so itself
        m.DEEngine(obj, 40, 2)
    assert ei.value.code == 2


def test_header_params_equal_the_drop_ins(drop_ins, tmp_path):
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_batch_params")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_batch_params.cpp"), "-o", exe, "-ldl"])
    row = [float(v).hex() for v in DROP_ROW]
    # the driver mode ("turns" is the default) does not apply to an objective with params
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH, NLSG_DE_DRIVER="turns", NLSG_PSO_DRIVER="turns")
    got = json.loads(subprocess.check_output([exe] + row, env=env, text=True, timeout=300))
    for kind in ("de", "pso"):
        x, st, _ = drop_ins[kind, "params"]
        g = got[kind]
        assert same([float.fromhex(v) for v in g["x"]], x), kind
        assert bits(float.fromhex(g["f"])) == bits(st.f_value), kind
        assert (g["iters"], g["fcalls"]) == (st.iteration, st.function_calls_used), kind
    bad = subprocess.run([exe, "sann"] + row, env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 3
    assert "nlsg error 2" in bad.stderr and "nlsg_de_batch_create_custom" in bad.stderr
