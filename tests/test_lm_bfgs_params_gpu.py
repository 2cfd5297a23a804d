"""Run-time objective parameters of Levenberg-Marquardt and BFGS (CustomObjective(n_params=...),
LMEngine / BFGSEngine.set_params): problem b of a parametrised batch must equal, bit for bit (x, every
Status field, LM's final lambda), a batch-1 engine of the SAME body with row b's numbers baked into
its source as literals -- the path that existed before these engines took parameters. The literals
are float.hex() in parentheses and the bodies let a parameter enter through + - * / only, so the
compiler has nothing to fold differently.

Every engine here costs one run-time compilation, which dominates the time: the engines are made
once per module and shared (ENGINES); the second set of rows of the replacement test is a rotation
of the first, so the literal engines serve both.

Shapes, LM (batch 3): n 2, 9, 33, 64 (the four lane-group widths of lm_fd_eval_groups and the narrow
kernel's limit), 65 and 130 (the wide kernels, one and two chunks; with batch 3 the tree-order kernel
runs 64 workgroups per problem and each stages the row). BFGS: dim 2, 9 (odd: scalar loads), 128 with
batch 6 (a full block of four waves with four rows, and a block whose last two waves leave at
pid >= batch), 130 with batch 5 in both orders and with the symmetric update, 600 in reference order
with 3072 parameters (eight chunks, the LDS budget's edge).

The starts and rows were chosen on the CPU, from the reference's own BFGS / LevenbergMarquardt on the
same functions (the reference-order device solves are its runs bit for bit): every solve iterates at
least three times, and in each BFGS batch of six two problems of one block stop at different
iteration counts, so a wave does leave while its neighbours go on."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    """every Status field, the two doubles as their bit patterns; best_index relative to the problem
    (b in the parametrised batch, 0 in the literal batch of one)"""
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
    if form.startswith("cends"):
        return int(form[5:])
    return {"terms": 3, "chain": 2, "vector": 2 * D, "one": 1, "chain3": 3, "quart": 3, "quart1": 1}[form]


def body(form, D, row=None):
    """row None: the parametrised body; else the same body with row's values as literals"""
    P = (lambda k: f"p({k})") if row is None else (lambda k: lit(row[k]))
    if form == "terms":
        return f"double r = xi - {P(0)}; return {P(1)} * r * r + r / {P(2)};"
    if form == "one":
        return f"double r = xi - {P(0)}; return r * r;"
    if form == "quart":  # (not a quadratic: BFGS would be done with one in a step or two)
        return f"double r = xi - {P(0)}; return {P(1)} * r * r * r * r + r * r / {P(2)};"
    if form == "quart1":
        return f"double r = xi - {P(0)}; return r * r * r * r + r * r;"
    if form == "chain":
        return f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; return t1 * t1 + {P(1)} * t2 * t2;"
    if form == "chain3":
        return (f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; "
                f"return t1 * t1 + {P(1)} * t2 * t2 + t1 / {P(2)};")
    if form.startswith("cends"):  # the chain form with its two parameters at the ends of a long row
        return (f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; "
                f"return t1 * t1 + {P(n_params_of(form, D) - 1)} * t2 * t2;")
    assert form == "vector"
    if row is None:
        return "return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return p(D + i) * r * r * r * r + r * r; });"
    table = ", ".join(lit(v) for v in row)
    return (f"const double q[{2 * D}] = {{{table}}}; "
            "return x.sum([&](double xi, uint64_t i) { double r = xi - q[i]; return q[D + i] * r * r * r * r + r * r; });")


def is_chain(form):
    return form.startswith(("chain", "cends"))


def objective(m, form, D, row=None):
    return m.CustomObjective(body(form, D, row), chain=is_chain(form), vector=form == "vector",
                             n_params=n_params_of(form, D) if row is None else 0)


def rows_for(form, D, B, salt=0):
    """[B, n_params]: distinct rows, weights positive, divisors away from zero. The chain forms'
    second weight (Rosenbrock's 100) spans two decades over the batch: the mild problems stop on the
    gradient norm long before the steep ones, which is what makes a BFGS wave leave early."""
    rng = np.random.default_rng(5000 + 17 * D + salt)
    n = n_params_of(form, D)
    steep = np.array([2.0, 100.0, 0.5, 30.0, 1.0, 60.0])[:B] * rng.uniform(0.9, 1.1, B)
    if form == "vector":
        return np.concatenate([rng.uniform(-1.0, 1.0, (B, D)), rng.uniform(0.5, 2.0, (B, D))], axis=1)
    if form.startswith("cends"):
        return np.concatenate([rng.uniform(0.8, 1.2, (B, 1)), rng.uniform(-1.0, 1.0, (B, n - 2)),
                               steep.reshape(B, 1)], axis=1)
    if form == "chain":
        return np.stack([rng.uniform(0.8, 1.2, B), steep], axis=1)
    if form == "chain3":
        return np.stack([rng.uniform(0.8, 1.2, B), steep, rng.uniform(2.0, 4.0, B)], axis=1)
    if form in ("one", "quart1"):
        return rng.uniform(0.5, 3.0, (B, 1))
    return rng.uniform(0.5, 3.0, (B, n))


def x0_for(D, B):
    """starts whose coordinates differ by up to 30 % in a pattern of period 11: along a uniform start a
    separable objective's gradient points straight at the minimum and BFGS is done in one step"""
    i = np.arange(D)
    return np.stack([(0.6 + 0.2 * b) * (1.0 + 0.06 * ((7 * i + 3 * b) % 11 - 5)) for b in range(B)])


# ---- engines, made once ------------------------------------------------------------------------------
def make_engine(m, kind, obj, batch, D, extra):
    from nlsolver_amd import _capi
    kw = dict(extra)
    if kind == "lm":
        ref = kw.pop("ref", False)
        solver = _capi.LM_CHOLESKY_REFERENCE_ORDER if ref else _capi.LM_CHOLESKY
        return m.LMEngine(obj, batch=batch, n=D, solver=solver, **kw)
    ref = kw.pop("ref", False)
    return m.BFGSEngine(obj, batch, dim=D, reference_order=ref, **kw)


@contextlib.contextmanager
def engines(m):
    """(kind, form, D, B, extra, row or None) -> engine; closed when the module is done"""
    made = {}

    def get(kind, form, D, B, extra=(), row=None):
        key = (kind, form, D, B if row is None else 1, tuple(extra),
               None if row is None else tuple(float(v) for v in row))
        if key not in made:
            made[key] = make_engine(m, kind, objective(m, form, D, row), B if row is None else 1, D, extra)
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


def solve(eng, kind, x0, params=None):
    """(x, [Status], lambda or None)"""
    if kind == "lm":
        return eng.minimize(x0.copy(), params=params)
    x, sts = eng.minimize(x0.copy(), params=params)
    return x, sts, None


def assert_matches_baked(ENGINES, kind, form, D, B, extra, rows, which=None):
    """the parametrised engine under `rows` against the literal engines of each row (`which`: only
    these problems have their literal twin built)"""
    x0 = x0_for(D, B)
    par = ENGINES(kind, form, D, B, extra)
    x, sts, lam = solve(par, kind, x0, rows)
    got = [status_tuple(s, b) for b, s in enumerate(sts)]
    for b in (range(B) if which is None else which):
        xb, sb, lb = solve(ENGINES(kind, form, D, B, extra, rows[b]), kind, x0[b:b + 1])
        tag = f"{kind} {form} n {D} {dict(extra)}, problem {b}"
        assert same(x[b], xb[0]), tag
        assert got[b] == status_tuple(sb[0]), tag
        if kind == "lm":
            assert same(lam[b], lb[0]), tag
    return x, got


def assert_meaningful(x, sts, B, least_iter=3):
    """at least three iterations each, and pairwise different end points"""
    assert all(s[1] >= least_iter for s in sts), [s[1] for s in sts]
    assert len({tuple(bits(x[b])) for b in range(B)}) == B


def extra_of(**kw):
    return tuple(sorted(kw.items()))


def case_id(c):
    return f"{c[0]}-n{c[1]}" + "".join(f"-{k}{v:g}" for k, v in c[-1])


# ---- 1. LM: problem b is the literal engine of row b -------------------------------------------------
LM_B = 3
T, R = dict(ref=False), dict(ref=True)
# (an LM engine compiles the whole LM kernel header, about 3 s, and a case makes four: one case per
# shape and order rather than every form at every shape)
LM_CASES = [
    ("one", 2, extra_of(max_iter=8, **R)), ("vector", 2, extra_of(max_iter=8, **T)),
    ("terms", 9, extra_of(max_iter=8, **T)), ("chain", 9, extra_of(max_iter=8, **R)),
    ("chain3", 33, extra_of(max_iter=8, **T)),
    ("vector", 64, extra_of(max_iter=8, **T)), ("terms", 64, extra_of(max_iter=8, **R)),
    ("chain", 65, extra_of(max_iter=8, **T)), ("terms", 65, extra_of(max_iter=8, **R)),
    ("vector", 130, extra_of(max_iter=8, **T)), ("chain", 130, extra_of(max_iter=8, **R)),
    ("cends4096", 9, extra_of(max_iter=8, **T)),
]


@pytest.mark.parametrize("form,D,extra", LM_CASES, ids=[case_id(c) for c in LM_CASES])
def test_lm_problems_equal_the_literal_engines(ENGINES, form, D, extra):
    x, sts = assert_matches_baked(ENGINES, "lm", form, D, LM_B, extra, rows_for(form, D, LM_B))
    assert_meaningful(x, sts, LM_B)
    assert all(s[1] <= dict(extra)["max_iter"] for s in sts)


# ---- 2. BFGS -----------------------------------------------------------------------------------------
BFGS6_CASES = [
    ("chain", 2, extra_of(max_iter=20, **R)), ("quart", 2, extra_of(max_iter=20, grad_eps=1e-7, **R)),
    ("vector", 2, extra_of(max_iter=20, grad_eps=1e-10, **T)),
    ("chain", 9, extra_of(max_iter=20, **T)), ("chain3", 9, extra_of(max_iter=20, **R)),
    ("vector", 9, extra_of(max_iter=20, grad_eps=1e-7, **T)), ("quart1", 9, extra_of(max_iter=20, grad_eps=1e-7, **R)),
    ("chain", 128, extra_of(max_iter=20, **R)), ("chain", 128, extra_of(max_iter=20, **T)),
    ("vector", 128, extra_of(max_iter=20, grad_eps=1e-7, **T)),
]
# (the smooth separable forms stop on the default gradient tolerance after one or two steps: theirs is
# tighter. Iteration counts of these cases in the reference's BFGS on the CPU, problems 0 .. 5:
# chain 2: 5 9 3 7 3 14; quart 2: 4 5 3 3 4 3; vector 2: 4 5 5 6 4 5; chain 9: 8 20 14 20 3 20;
# chain3 9: 20 20 6 16 18 11; vector 9: 5 5 6 5 6 6; quart1 9: 4 5 4 3 4 5; chain 128: 20 20 18 20 20 20;
# vector 128: 6 8 8 9 9 9.)


@pytest.mark.parametrize("form,D,extra", BFGS6_CASES, ids=[case_id(c) for c in BFGS6_CASES])
def test_bfgs_six_problems_equal_the_literal_engines(ENGINES, form, D, extra):
    """batch 6: waves 0 .. 3 of block 0 have a row each, waves 2 and 3 of block 1 leave at pid >= batch"""
    B = 6
    x, sts = assert_matches_baked(ENGINES, "bfgs", form, D, B, extra, rows_for(form, D, B))
    assert_meaningful(x, sts, B)
    iters = [s[1] for s in sts]  # a wave leaves while its neighbours of the same block go on
    assert len(set(iters[:4])) > 1 or len(set(iters[4:])) > 1, iters


BFGS5_CASES = [
    ("chain", 130, extra_of(max_iter=12, **T)), ("chain", 130, extra_of(max_iter=12, **R)),
    ("quart", 130, extra_of(max_iter=12, grad_eps=1e-7, symmetric=True, **T)),
]


@pytest.mark.parametrize("form,D,extra", BFGS5_CASES, ids=[case_id(c) for c in BFGS5_CASES])
def test_bfgs_two_chunks_equal_the_literal_engines(ENGINES, form, D, extra):
    B = 5
    x, sts = assert_matches_baked(ENGINES, "bfgs", form, D, B, extra, rows_for(form, D, B))
    assert_meaningful(x, sts, B)


def test_bfgs_at_the_budgets_edge(m, ENGINES):
    """dim 600 in reference order: 64 KiB of xs | ts buffers and four rows of 3072 parameters, read at
    both ends, fill the 160 KiB exactly; one more pair of parameters is refused by name"""
    form, D, B, extra = "cends3072", 600, 5, extra_of(max_iter=8, **R)
    assert m.BFGSEngine.fits(D, True, 3072) and not m.BFGSEngine.fits(D, True, 3073)
    assert m.BFGSEngine.lds_bytes(D, True, 3072) == 160 * 1024
    x, sts = assert_matches_baked(ENGINES, "bfgs", form, D, B, extra, rows_for(form, D, B))
    assert_meaningful(x, sts, B)
    with pytest.raises(m.NlsgError) as ei:
        m.BFGSEngine(objective(m, "cends3073", D), B, dim=D, reference_order=True)
    assert ei.value.code == 2 and "163840" in str(ei.value)


def test_bfgs_with_the_largest_rows(m, ENGINES):
    """dim 16 in tree order with 4096 parameters: 128 KiB of rows, past the static limit -- the
    dynamic-LDS attribute of the module kernels"""
    form, D, B, extra = "cends4096", 16, 6, extra_of(max_iter=12, **T)
    assert m.BFGSEngine.fits(D, False, 4096) and m.BFGSEngine.lds_bytes(D, False, 4096) == 128 * 1024
    x, sts = assert_matches_baked(ENGINES, "bfgs", form, D, B, extra, rows_for(form, D, B))
    assert_meaningful(x, sts, B)


# ---- 3. replacement without a rebuild ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lm", "bfgs"])
def test_rows_are_replaced_without_a_rebuild(ENGINES, kind):
    """one engine: rows A, A rotated, A again; the rotation's literal engines are A's"""
    form, D, B, extra = ("chain", 9, LM_B, extra_of(max_iter=8, **R)) if kind == "lm" else \
        ("chain", 9, 6, extra_of(max_iter=20, **T))
    x0 = x0_for(D, B)
    A = rows_for(form, D, B)
    first = assert_matches_baked(ENGINES, kind, form, D, B, extra, A)
    rot = np.roll(A, 1, axis=0)
    par = ENGINES(kind, form, D, B, extra)
    par.set_params(rot)
    x, sts, lam = solve(par, kind, x0)
    for b in range(B):  # problem b under row b - 1: the literal engine of that row from start b
        xb, sb, lb = solve(ENGINES(kind, form, D, B, extra, rot[b]), kind, x0[b:b + 1])
        assert same(x[b], xb[0]) and status_tuple(sts[b], b) == status_tuple(sb[0]), b
        if kind == "lm":
            assert same(lam[b], lb[0]), b
    assert not same(first[0], x)
    again = assert_matches_baked(ENGINES, kind, form, D, B, extra, A)
    assert same(first[0], again[0]) and first[1] == again[1]


# ---- 4. state ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lm", "bfgs"])
def test_call_order(m, ENGINES, kind):
    from nlsolver_amd import _capi
    B, D = 3, 2
    x0 = x0_for(D, B)
    eng = make_engine(m, kind, objective(m, "one", D), B, D, ())
    try:
        if kind == "lm":
            calls = [lambda: eng.minimize(x0.copy()), lambda: eng.time_solve(x0),
                     lambda: eng.time_eval_kernel(x0), lambda: eng.time_qr_kernel(x0)]
        else:
            calls = [lambda: eng.init(x0), lambda: eng.step(1), lambda: eng.minimize(x0.copy()),
                     lambda: eng.time_steps(1)]
        for call in calls:
            with pytest.raises(m.NlsgError) as ei:
                call()
            assert ei.value.code == 6
        eng.set_params(rows_for("one", D, B))
        eng.minimize(x0.copy())
    finally:
        eng.close()
    name = "nlsg_lm_set_params" if kind == "lm" else "nlsg_bfgs_set_params"
    for plain in ("rosenbrock", objective(m, "one", D, [1.5])):
        eng = make_engine(m, kind, plain, B, D, ())
        try:
            with pytest.raises(m.NlsgError) as ei:
                eng.set_params(np.zeros((B, 1)))
            assert ei.value.code == 1
            row = np.zeros(B)
            assert getattr(_capi.lib(), name)(eng._h, row.ctypes.data_as(_capi.pd)) == 1
        finally:
            eng.close()


# ---- 5. the drop-in classes and the C++ header -------------------------------------------------------
DROP_ROW = (1.25, 2.5, 3.5)


@pytest.fixture(scope="module")
def drop_ins(m):
    """{("bfgs" | "lm", "params" | "baked"): (x, Status)} for x0 = (5, 7)"""
    out = {}
    for how in ("params", "baked"):
        obj = objective(m, "terms", 2, None if how == "params" else DROP_ROW)
        kw = dict(params=DROP_ROW) if how == "params" else {}
        for kind, solver in (("bfgs", m.BFGS(obj, **kw)), ("lm", m.LevenbergMarquardt(obj, **kw))):
            x = np.array([5.0, 7.0])
            out[kind, how] = (x, solver.minimize(x))
    return out


@pytest.mark.parametrize("kind", ["bfgs", "lm"])
def test_drop_in_with_params_equals_the_literal_objective(drop_ins, kind):
    (xp, sp), (xb, sb) = drop_ins[kind, "params"], drop_ins[kind, "baked"]
    assert same(xp, xb) and status_tuple(sp) == status_tuple(sb)
    assert sp.iteration > 0 and sp.done == 1


@pytest.mark.parametrize("kind", ["bfgs", "lm"])
def test_drop_in_shows_one_row_to_every_start(m, drop_ins, kind):
    obj = objective(m, "terms", 2)
    cls = m.BFGS if kind == "bfgs" else m.LevenbergMarquardt
    x = np.array([[5.0, 7.0], [5.0, 7.0]])
    sts = cls(obj, params=DROP_ROW).minimize(x)
    xp, sp = drop_ins[kind, "params"]
    assert same(x[0], xp) and same(x[1], xp) and status_tuple(sts[1], 1) == status_tuple(sp)
    with pytest.raises(ValueError):
        cls(obj, params=[DROP_ROW] * 3).minimize(x)


def test_header_params_equal_the_drop_ins(drop_ins, tmp_path):
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_lm_bfgs_params")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_lm_bfgs_params.cpp"), "-o", exe, "-ldl"])
    row = [float(v).hex() for v in DROP_ROW]
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    got = json.loads(subprocess.check_output([exe] + row, env=env, text=True, timeout=300))
    for kind in ("bfgs", "lm"):
        x, st = drop_ins[kind, "params"]
        g = got[kind]
        assert same([float.fromhex(v) for v in g["x"]], x), kind
        assert bits(float.fromhex(g["f"])) == bits(st.f_value), kind
        assert (g["iters"], g["fcalls"]) == (st.iteration, st.function_calls_used), kind
