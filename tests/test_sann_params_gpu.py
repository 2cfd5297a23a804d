"""Run-time objective parameters of simulated annealing (CustomObjective(n_params=...),
SANNEngine.set_params): chain b of a parametrised batch must equal, bit for bit (x and every Status
field), a batch-1 engine of the SAME body with row b's numbers baked into its source as literals, the
same seed and chain_lo = b -- the path that existed before the engine took parameters. The literals
are float.hex() in parentheses and the bodies let a parameter enter through + - * / only, so the
compiler has nothing to fold differently.

Shapes: dim 2 (4 lanes per chain, 16 chains per wave), 9 (8 lanes, odd), 17 (16 lanes), 33 (32 lanes),
65 and 130 (one wave per chain, one and two chunks per lane), 1026 (the kernel that streams the chain
from memory). Below 65 coordinates every lane group of a wave has a row of its own in LDS; where those
rows do not fit the shape runs one chain per wave, with the same bits (test 3).

Not to be blind: a chain that never accepts a trial returns its start, and a row then only enters
the first score. The starts lie 4 + 3 sqrt(dim) and more from the parametrised centre (a trial moves
every coordinate by about 1.85 at first: it improves a quadratic bowl while the distance is well above
0.9 sqrt(dim)); `checked` asserts for every chain that x left x0, that the value fell, and that the
chains of a batch differ. The same starts, seeds, chain ids and schedules were run through
orc_sann_sync on the built-in sphere before any GPU time was spent: every chain moves there too.

Every engine costs one run-time compilation, which dominates the time: engines are made once per
module (ENGINES); engines of one source (the batch-1 parametrised engines of test 2, the literal
engines of the long schedule) load the code object the first of them compiled."""
import contextlib
import json
import os
import subprocess
import sys

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
    """every Status field, the two doubles as their bit patterns; best_index (the chain's index in its
    own batch) relative to the chain"""
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


# ---- the objectives: p(k) and their twins with literals (the bodies of tests/test_nm_params_gpu.py) ----
def n_params_of(form, D):
    if form.startswith("ends"):
        return int(form[4:])
    return {"terms": 3, "chain": 2, "vector": 2 * D, "sphere": 2}[form]


def body(form, D, row=None):
    """row None: the parametrised body; else the same body with row's values as literals"""
    P = (lambda k: f"p({k})") if row is None else (lambda k: lit(row[k]))
    if form == "terms":
        return f"double r = xi - {P(0)}; return {P(1)} * r * r + r / {P(2)};"
    if form == "chain":
        return f"double t1 = {P(0)} - xi, t2 = xn - xi * xi; return t1 * t1 + {P(1)} * t2 * t2;"
    if form == "sphere":
        return f"double r = xi - {P(0)}; return {P(1)} * r * r;"
    if form.startswith("ends"):  # two parameters, at the two ends of a long row
        return f"double r = xi - {P(0)}; return {P(n_params_of(form, D) - 1)} * r * r;"
    assert form == "vector"
    if row is None:
        return "return x.sum([&](double xi, uint64_t i) { double r = xi - p(i); return p(D + i) * r * r; });"
    table = ", ".join(lit(v) for v in row)
    return (f"const double q[{2 * D}] = {{{table}}}; "
            "return x.sum([&](double xi, uint64_t i) { double r = xi - q[i]; return q[D + i] * r * r; });")


def objective(m, form, D, row=None):
    return m.CustomObjective(body(form, D, row), chain=form == "chain", vector=form == "vector",
                             n_params=n_params_of(form, D) if row is None else 0)


def value(form, D, x, row):
    """the objective in host arithmetic (for `the value fell` only: never compared bit for bit)"""
    x, row = np.asarray(x, dtype=np.float64), np.asarray(row, dtype=np.float64)
    if form == "terms":
        r = x - row[0]
        return float(np.sum(row[1] * r * r + r / row[2]))
    if form == "chain":
        t1, t2 = row[0] - x[:-1], x[1:] - x[:-1] * x[:-1]
        return float(np.sum(t1 * t1 + row[1] * t2 * t2))
    if form == "vector":
        r = x - row[:D]
        return float(np.sum(row[D:] * r * r))
    r = x - row[0]                      # sphere, ends*
    return float(np.sum(row[-1] * r * r))


def rows_for(form, D, n=B, salt=0):
    """[n, n_params]: distinct rows, centres within [-1, 3], weights positive, divisors away from zero"""
    rng = np.random.default_rng(2000 + 17 * D + salt)
    k = n_params_of(form, D)
    if form == "vector":
        return np.concatenate([rng.uniform(-1.0, 1.0, (n, D)), rng.uniform(0.5, 2.0, (n, D))], axis=1)
    if form.startswith("ends") or form == "sphere":
        return np.concatenate([rng.uniform(-1.0, 1.0, (n, k - 1)), rng.uniform(0.5, 2.0, (n, 1))], axis=1)
    if form == "chain":
        return np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(50.0, 150.0, n)], axis=1)
    return rng.uniform(0.5, 3.0, (n, k))


def x0_for(D, n=B):
    """starts well outside the bowl (module docstring): 3 + (4 + 3 sqrt(D)) (1 + b / 4) and a ramp"""
    return np.stack([3.0 + (4.0 + 3.0 * np.sqrt(D)) * (1.0 + 0.25 * b) * (1.0 + 0.001 * np.arange(D))
                     for b in range(n)])


# ---- engines, made once ------------------------------------------------------------------------------
@contextlib.contextmanager
def engines(m):
    """(form, D, extra, row or None, chain_lo, batch) -> engine; closed when the module is done"""
    made = {}

    def get(form, D, extra=(), row=None, chain_lo=0, batch=None):
        batch = (B if row is None else 1) if batch is None else batch
        key = (form, D, tuple(extra), None if row is None else tuple(float(v) for v in row), chain_lo, batch)
        if key not in made:
            made[key] = m.SANNEngine(objective(m, form, D, row), batch, D, seed=SEED, chain_lo=chain_lo,
                                     **dict(extra))
        return made[key]

    try:
        yield get
    finally:
        for eng in made.values():
            eng.close()


@pytest.fixture(scope="module")
def ENGINES(m):
    with engines(m) as get:
        yield get


def sann_extra(max_iter, **kw):
    return tuple(sorted(dict(max_iter=max_iter, temperature_iter=10, **kw).items()))


def checked(form, D, extra, x0, rows, x, sts):
    """the condition of the module docstring, for every chain of a solve; returns the status tuples"""
    fmul = 1.0 if dict(extra).get("minimize", True) else -1.0
    got = [status_tuple(s, b) for b, s in enumerate(sts)]
    for b in range(len(sts)):
        tag = f"{form} dim {D} {dict(extra)}, chain {b}"
        assert not same(x[b], x0[b]), tag + ": no trial was ever accepted"
        assert sts[b].f_value < fmul * value(form, D, x0[b], rows[b]), tag
        assert sts[b].iteration == dict(extra)["max_iter"] and sts[b].done == 1, tag
        assert sts[b].function_calls_used == 1 + 9 * dict(extra)["max_iter"], tag
    assert len({tuple(bits(x[b])) for b in range(len(sts))}) == len(sts), f"{form} dim {D}: chains coincide"
    return got


def assert_matches_baked(get, form, D, extra, rows, x0=None):
    """the parametrised engine under `rows` against the literal engines of each row"""
    x0 = x0_for(D) if x0 is None else x0
    x, sts = get(form, D, extra).minimize(x0, params=rows)
    got = checked(form, D, extra, x0, rows, x, sts)
    for b in range(B):
        xb, sb = get(form, D, extra, rows[b], b).minimize(x0[b:b + 1])
        tag = f"{form} dim {D} {dict(extra)}, chain {b}"
        assert same(x[b], xb[0]), tag
        assert got[b] == status_tuple(sb[0]), tag
    return x, got


# ---- 1. chain b is the literal engine of row b -------------------------------------------------------
CASES = [("terms", 2, sann_extra(40)), ("chain", 9, sann_extra(40)),
         ("vector", 9, sann_extra(30, minimize=False)), ("vector", 33, sann_extra(30)),
         ("chain", 65, sann_extra(30)), ("terms", 130, sann_extra(30)), ("terms", 1026, sann_extra(30))]


def case_id(c):
    return f"{c[0]}-dim{c[1]}" + "".join(f"-{k}{int(v)}" for k, v in c[2])


@pytest.mark.parametrize("form,D,extra", CASES, ids=[case_id(c) for c in CASES])
def test_chains_equal_the_literal_engines(m, ENGINES, form, D, extra):
    n = n_params_of(form, D)
    assert m.SANNEngine.chains_per_wave(D, n) == {2: 16, 9: 8, 33: 2}.get(D, 1)
    x, sts = assert_matches_baked(ENGINES, form, D, extra, rows_for(form, D))
    assert len(set(sts)) == B


# ---- 2. every chain of a wide batch is its solo run --------------------------------------------------
WIDE = [(2, 18),   # a full wave of 16 groups and a wave with 2 live and 14 shadowing groups
        (17, 5),   # 16 lanes per chain: a wave of 4 groups and one with a single live group
        (65, 6)]   # one wave per chain: a block whose last two waves leave at once


@pytest.mark.parametrize("D,N", WIDE, ids=[f"dim{d}-batch{n}" for d, n in WIDE])
def test_every_chain_of_a_wide_batch_equals_its_solo_run(ENGINES, D, N):
    """the solo engines are parametrised too (batch 1, chain_lo = b, row b): one source, one compilation.
    With test 1 this pins that no group and no wave reads a neighbour's row."""
    form, extra = "terms", sann_extra(30)
    rows, x0 = rows_for(form, D, N), x0_for(D, N)
    x, sts = ENGINES(form, D, extra, batch=N).minimize(x0, params=rows)
    got = checked(form, D, extra, x0, rows, x, sts)
    for b in range(N):
        xb, sb = ENGINES(form, D, extra, chain_lo=b, batch=1).minimize(x0[b:b + 1], params=rows[b:b + 1])
        assert same(x[b], xb[0]), (D, b)
        assert got[b] == status_tuple(sb[0]), (D, b)


# ---- 3. rows too long for the packed layout: one chain per wave, the same bits -----------------------
@pytest.mark.parametrize("D", [2, 16])
def test_the_fallback_changes_no_bit(m, ENGINES, D):
    S = m.SANNEngine
    past = min(k for k in range(1, 4097) if S.chains_per_wave(D, k) == 1)
    assert past == {2: 311, 16: 623}[D]
    assert S.chains_per_wave(D, past - 1) == S.chains_per_wave(D, 2) == {2: 16, 16: 8}[D]
    extra, x0 = sann_extra(40), x0_for(D)
    long_rows = rows_for("ends4096", D)
    two = np.ascontiguousarray(long_rows[:, [0, 4095]])
    assert S.chains_per_wave(D, 2) > 1
    x, sts = ENGINES("ends2", D, extra).minimize(x0, params=two)
    want = checked("ends2", D, extra, x0, two, x, sts)
    for n in (past, 4096):
        assert S.chains_per_wave(D, n) == 1
        rows = np.ascontiguousarray(long_rows[:, :n])
        rows[:, n - 1] = long_rows[:, 4095]          # the body reads p(0) and p(n - 1)
        xn, stn = ENGINES(f"ends{n}", D, extra).minimize(x0, params=rows)
        assert same(xn, x), (D, n)
        assert [status_tuple(s, b) for b, s in enumerate(stn)] == want, (D, n)


# ---- 4. the parametrised sphere is the built-in sphere -----------------------------------------------
@pytest.mark.parametrize("D", [2, 130])
def test_the_parametrised_sphere_is_the_built_in_sphere(m, ENGINES, D):
    from tests import _oracle as O
    extra, x0 = sann_extra(40), x0_for(D)
    rows = np.tile([0.0, 1.0], (B, 1))
    x, sts = ENGINES("sphere", D, extra).minimize(x0, params=rows)
    got = checked("sphere", D, extra, x0, rows, x, sts)
    with m.SANNEngine("sphere", B, D, seed=SEED, **dict(extra)) as eng:
        xs, ss = eng.minimize(x0)
    assert same(x, xs) and got == [status_tuple(s, b) for b, s in enumerate(ss)]
    lib = O.load()
    for b in range(B):
        st, xo, _ = O.sann_sync(lib, "sphere", x0[b], SEED, b, max_iter=40, temp_iter=10, temp_max=10.0)
        assert same(x[b], xo), (D, b)
        assert bits(sts[b].f_value) == bits(st.f_value), (D, b)
        assert (sts[b].iteration, sts[b].function_calls_used) == (st.iteration, st.function_calls_used), (D, b)


# ---- 5. replacement without a rebuild ----------------------------------------------------------------
def test_rows_are_replaced_without_a_rebuild(ENGINES):
    """one engine: rows A, A rotated (chain b under row b - 1: new literal engines of A's sources, which
    load A's code), A again"""
    form, D, extra = CASES[0]
    A = rows_for(form, D)
    first = assert_matches_baked(ENGINES, form, D, extra, A)
    second = assert_matches_baked(ENGINES, form, D, extra, np.roll(A, 1, axis=0))
    assert not same(first[0], second[0])
    again = assert_matches_baked(ENGINES, form, D, extra, A)
    assert same(first[0], again[0]) and first[1] == again[1]


# ---- 6. a schedule cut into two launches -------------------------------------------------------------
def test_a_cut_schedule_stages_its_rows_again(ENGINES):
    """7300 x 9 = 65 700 trial points: more than the 65 536 of one launch, so a second launch picks the
    chains up from memory and must find its rows again"""
    form, D, extra = "terms", 2, sann_extra(7300)
    x, sts = assert_matches_baked(ENGINES, form, D, extra, rows_for(form, D))
    assert len(set(sts)) == B


# ---- 7. state ----------------------------------------------------------------------------------------
def test_call_order(m):
    from nlsolver_amd import _capi
    x0 = x0_for(2)
    with m.SANNEngine(objective(m, "sphere", 2), B, 2, max_iter=5) as eng:
        for call in (lambda: eng.minimize(x0), lambda: eng.time_solve(x0)):
            with pytest.raises(m.NlsgError) as ei:
                call()
            assert ei.value.code == 6
        eng.set_params(rows_for("sphere", 2))
        eng.minimize(x0)
    for plain in ("rosenbrock", objective(m, "sphere", 2, [0.5, 1.5])):
        with m.SANNEngine(plain, B, 2, max_iter=5) as eng:
            with pytest.raises(m.NlsgError) as ei:
                eng.set_params(np.zeros((B, 2)))
            assert ei.value.code == 1
            row = np.zeros(2 * B)
            assert _capi.lib().nlsg_sann_set_params(eng._h, row.ctypes.data_as(_capi.pd)) == 1


# ---- 8. the drop-in ----------------------------------------------------------------------------------
def test_drop_in_equals_the_engine(m):
    from nlsolver_amd.de import DEFAULT_SEED
    obj, D = objective(m, "terms", 2), 2
    rows, x0 = rows_for("terms", D), x0_for(D)
    with m.SANNEngine(obj, B, D, max_iter=40, seed=DEFAULT_SEED) as eng:
        x_one, st_one = eng.minimize(x0, params=np.tile(rows[1], (B, 1)))
        x_each, st_each = eng.minimize(x0, params=rows)
    # one row, one start: chain 0 under that row
    x = x0[0].copy()
    st = m.SANN(obj, None, 40, params=rows[1]).minimize(x)
    assert same(x, x_one[0]) and status_tuple(st) == status_tuple(st_one[0])
    # one row shown to every chain of a 2-D x
    x = x0.copy()
    sts = m.SANN(obj, None, 40, params=rows[1]).minimize(x)
    assert same(x, x_one) and [status_tuple(s) for s in sts] == [status_tuple(s) for s in st_one]
    # a row per chain
    x = x0.copy()
    sts = m.SANN(obj, None, 40, params=rows).minimize(x)
    assert same(x, x_each) and [status_tuple(s) for s in sts] == [status_tuple(s) for s in st_each]
    assert not same(x_each, x_one)
    with pytest.raises(ValueError):
        m.SANN(obj, None, 40, params=rows[:2]).minimize(x0.copy())   # 2 rows, 3 chains


def test_a_sweep_of_64_values_is_one_engine(m):
    """one start, one seed, 64 centres: 64 different answers from one compilation"""
    obj = objective(m, "sphere", 2)
    rows = np.stack([np.linspace(-1.0, 1.0, 64), np.full(64, 1.5)], axis=1)
    x = np.tile(x0_for(2)[0], (64, 1))
    x0 = x.copy()
    sts = m.SANN(obj, None, 40, params=rows).minimize(x)
    assert len({tuple(bits(x[b])) for b in range(64)} | {tuple(bits(x0[0]))}) == 65
    assert len({status_tuple(s, b)[0] for b, s in enumerate(sts)}) == 64
    assert all(s.f_value < value("sphere", 2, x0[b], rows[b]) for b, s in enumerate(sts))


# ---- 9. poisoned device memory -----------------------------------------------------------------------
POISON_CASES = [("terms", 2, sann_extra(40)), ("terms", 65, sann_extra(30))]   # (3 parameters: an odd row)


def poison_child():
    """runs in a child process under NLSG_POOL_POISON: the cases' results as JSON on stdout"""
    import nlsolver_amd as m
    out = []
    with engines(m) as get:
        for form, D, extra in POISON_CASES:
            x, sts = get(form, D, extra).minimize(x0_for(D), params=rows_for(form, D))
            out.append(dict(x=[int(v) for v in bits(x).ravel()], st=[status_tuple(s, b) for b, s in enumerate(sts)]))
    print("poison-json " + json.dumps(out))


CHILD_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
from nlsolver_amd import _capi
assert _capi.lib().nlsg_pool_poison() == %(byte)d, ("poison byte in force", _capi.lib().nlsg_pool_poison())
from tests import test_sann_params_gpu as T
T.poison_child()
"""


@pytest.mark.parametrize("pattern,byte", [("1", 0xFF), ("0xC0", 0xC0)])
def test_poisoned_blocks_change_no_bit(ENGINES, pattern, byte):
    """every block of the child's pool (the rows' device buffer among them) is filled with one byte
    before it is handed out; the row of 3 parameters leaves a padding double in LDS that nobody reads"""
    env = dict(os.environ, NLSG_POOL_POISON=pattern)
    r = subprocess.run([sys.executable, "-c", CHILD_SCRIPT % dict(root=ROOT, byte=byte)], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("poison-json "))
    got = json.loads(line[len("poison-json "):])
    for (form, D, extra), g in zip(POISON_CASES, got):
        x0, rows = x0_for(D), rows_for(form, D)
        x, sts = ENGINES(form, D, extra).minimize(x0, params=rows)
        want = checked(form, D, extra, x0, rows, x, sts)
        assert g["x"] == [int(v) for v in bits(x).ravel()], (form, D, pattern)
        assert [tuple(s) for s in g["st"]] == want, (form, D, pattern)
