"""The resident batch PSO engine (PSOBatchEngine / nlsg_pso_batch_*): every solve of a batch is the
keyed engine's solve of its seed and bounds, bit for bit -- against PSOEngine itself and against the
restatement orc_pso_sync_* (tests._oracle.PSOSyncRun), which shares no host code with either.

Sizes are the smallest at which a mapping, a pass boundary or a rule changes: one particle of one
coordinate, G = 4 / 8 / 16 / 32 lanes per particle with a ragged last pass and odd D (a padded LDS
row), the full group (64), the first one-wave-per-particle dimension (65), the full chunk (128) and
the largest swarm (1024: the full last stride of the 256-thread sums)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 12374563468
TYPES = [O.PSO_ACCELERATED, O.PSO_VANILLA]
TYPE_IDS = ["accelerated", "vanilla"]


def seeds_for(batch):
    return [SEED0 + 7919 * b for b in range(batch)]


@pytest.fixture(scope="module")
def m():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    from nlsolver_amd import _capi
    assert _capi.lib().nlsg_device_count() >= 1
    return nlsolver_amd


def bounds_for(batch, D):
    """distinct bounds per solve and per coordinate"""
    scale = (1.0 + 0.25 * np.arange(batch))[:, None]
    lo = -2.048 * (1 + 0.001 * np.arange(D))[None, :] * scale
    hi = 2.048 * (1 + 0.002 * np.arange(D))[None, :] * scale
    return lo, hi


STATUS_FIELDS = ("f_value", "iteration", "function_calls_used", "best_index", "val_no_change", "std_err",
                 "done")


def status_tuple(st):
    """the seven fields, the two doubles as their bit patterns (std_err is NaN when not evaluated)"""
    return tuple(int(np.float64(getattr(st, f)).view(np.uint64)) if f in ("f_value", "std_err")
                 else int(getattr(st, f)) for f in STATUS_FIELDS)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def assert_equals_engine(beng, b, one, tag, sts=None, best=None):
    """solve b of the batch engine against a PSOEngine after the same calls: download, status, best"""
    got, want = beng.download(b), one.download()
    for name, g, w in zip(("positions", "velocities", "pbest values", "last values"), got, want):
        assert same(g, w), f"{tag}: {name}"
    st = (sts or beng.status())[b]
    assert status_tuple(st) == status_tuple(one.status()), tag
    bx, bf, bi = best or beng.best()
    ox, of, oi = one.best()
    assert same(bx[b], ox) and same(bf[b], np.float64(of)) and int(bi[b]) == oi, f"{tag}: best"


# ---- 1. turn by turn against PSOEngine -----------------------------------------------------------
SHAPES = [(10, 2), (1, 1), (65, 5), (33, 9), (20, 17), (9, 33), (6, 64), (6, 65), (5, 128), (1024, 2)]


@pytest.mark.parametrize("n,D", SHAPES)
@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
def test_turns_equal_the_turn_engine(m, n, D, type_, bounded):
    batch, turns = 3, 5
    lo, hi = bounds_for(batch, D)
    seeds = seeds_for(batch)
    # eps > 0 but tiny: std_err is evaluated every turn and never stops the solve
    kw = dict(type=type_, bounded=bounded, eps=1e-300, max_iter=1000, best_val_no_change=1000)
    ones = [m.PSOEngine("rosenbrock", n, D, seed=s, **kw) for s in seeds]
    try:
        with m.PSOBatchEngine("rosenbrock", batch, n, D, **kw) as eng:
            eng.init(lo, hi, seeds)
            for b, one in enumerate(ones):
                one.init(lo[b], hi[b])
            moved = 0
            for t in range(turns + 1):
                if t:
                    before = [eng.download(b)[0] for b in range(batch)]
                    eng.step(1)
                    moved += sum(int(np.sum(eng.download(b)[0] != before[b])) for b in range(batch))
                sts, best = eng.status(), eng.best()
                for b, one in enumerate(ones):
                    if t:
                        one.step(1)
                    assert_equals_engine(eng, b, one, f"turn {t}, solve {b}", sts, best)
            assert moved > 0  # the swarm did move
            if n > 1:  # distinct seeds and bounds give distinct solves
                assert not same(eng.download(0)[0], eng.download(1)[0])
    finally:
        for one in ones:
            one.close()


# ---- 2. the same against the restatement ----------------------------------------------------------
def counters(st):
    return (st.iteration, st.function_calls_used, st.val_no_change, st.done)


@pytest.mark.parametrize("n,D", [(10, 2), (65, 5), (6, 65)])
@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_turns_follow_the_restatement(m, oracle, n, D, type_):
    batch, turns = 3, 5
    lo, hi = bounds_for(batch, D)
    seeds = seeds_for(batch)
    kw = dict(type=type_, bounded=True, eps=0.0, max_iter=1000, best_val_no_change=1000)
    refs = [O.PSOSyncRun(oracle, "rosenbrock", n, D, lo[b], hi[b], seed=s, **kw) for b, s in enumerate(seeds)]
    with m.PSOBatchEngine("rosenbrock", batch, n, D, **kw) as eng:
        eng.init(lo, hi, seeds)
        for t in range(turns + 1):
            if t:
                eng.step(1)
            sts = eng.status()
            bx, bf, bi = eng.best()
            for b, ref in enumerate(refs):
                if t:
                    ref.step(1)
                tag = f"turn {t}, solve {b}"
                pos, vel, pbest, cur = eng.download(b)
                assert np.array_equal(pos, ref.pos), f"{tag}: positions"
                assert np.array_equal(cur, ref.cur_val), f"{tag}: values of the last evaluation"
                assert np.array_equal(pbest, ref.pbest_val), f"{tag}: personal-best values"
                if vel is not None:
                    assert np.array_equal(vel, ref.vel), f"{tag}: velocities"
                assert counters(sts[b]) == (ref.s.iter, ref.s.fevals, ref.s.val_no_change, ref.s.done), tag
                if ref.s.fevals:
                    assert sts[b].f_value == ref.s.gbest_val and sts[b].best_index == ref.s.gbest_idx, tag
                    assert np.array_equal(bx[b], ref.gbest_x) and bf[b] == ref.s.gbest_val, tag
                    assert bi[b] == ref.s.gbest_idx, tag


# ---- 3. whole solves to each stop test, independently per solve ----------------------------------
STOPS = [dict(eps=10e-4), dict(eps=0.0, best_val_no_change=3), dict(eps=0.0, max_iter=9), dict(eps=50.0)]


@pytest.mark.parametrize("kw", STOPS, ids=["eps", "no_change", "max_iter", "eps_50"])
@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_whole_solves_stop_where_the_restatement_stops(m, oracle, kw, type_):
    n, D, batch = 10, 2, 8
    args = dict(eps=10e-4, max_iter=300, best_val_no_change=50, type=type_)
    args.update(kw)
    seeds = seeds_for(batch)
    refs = []
    for s in seeds:
        ref = O.PSOSyncRun(oracle, "rosenbrock", n, D, -3.0, 3.0, seed=s, **args)
        while not ref.s.done:
            ref.step()
        refs.append(ref)
    with m.PSOBatchEngine("rosenbrock", batch, n, D, **args) as eng:
        x, sts = eng.minimize(-3.0, 3.0, seeds)
        bx, bf, bi = eng.best()
    for b, ref in enumerate(refs):
        st, tag = sts[b], f"solve {b}"
        assert st.done == 1, tag
        assert (st.iteration, st.function_calls_used) == (ref.s.iter, ref.s.fevals), tag
        assert st.f_value == ref.s.gbest_val and st.best_index == ref.s.gbest_idx, tag
        assert np.array_equal(x[b], ref.gbest_x) and np.array_equal(bx[b], ref.gbest_x), tag
        if args["eps"] > 0:
            assert st.std_err == ref.s.std_err, tag
    if "max_iter" not in kw:  # a solve that is done stays frozen while its neighbours go on
        assert len({int(r.s.iter) for r in refs}) >= 4


# ---- 4. smaller checks ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(10, 2), (64, 16), (40, 128)])
@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_minimize_equals_the_turn_engine(m, n, D, type_):
    batch = 4
    lo, hi = bounds_for(batch, D)
    args = dict(type=type_, eps=10e-4, max_iter=60, best_val_no_change=50)
    seeds = seeds_for(batch)
    with m.PSOBatchEngine("rosenbrock", batch, n, D, **args) as eng:
        x, sts = eng.minimize(lo, hi, seeds)
    for b, s in enumerate(seeds):
        xe = np.zeros(D)
        with m.PSOEngine("rosenbrock", n, D, seed=s, **args) as one:
            ste = one.minimize(xe, lo[b], hi[b])
        assert same(x[b], xe), f"solve {b}"
        assert status_tuple(sts[b]) == status_tuple(ste), f"solve {b}"


@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_launch_cuts_change_nothing(m, type_):
    n, D, batch = 10, 2, 8
    seeds = seeds_for(batch)
    args = dict(type=type_, eps=10e-4, max_iter=300)
    outs = []
    for tpl in (1, 7, 1024, 0):
        with m.PSOBatchEngine("rosenbrock", batch, n, D, turns_per_launch=tpl, **args) as eng:
            x, sts = eng.minimize(-3.0, 3.0, seeds)
        outs.append((x, [status_tuple(s) for s in sts]))
    for x, sts in outs[1:]:
        assert same(x, outs[0][0]) and sts == outs[0][1]
    states = []
    for steps in ((3, 4), (7,)):
        with m.PSOBatchEngine("rosenbrock", batch, n, D, turns_per_launch=2, **args) as eng:
            eng.init(-3.0, 3.0, seeds)
            for t in steps:
                eng.step(t)
            states.append(([status_tuple(s) for s in eng.status()], [eng.download(b) for b in range(batch)],
                           eng.best()))
    (sa, da, ba), (sb, db, bb) = states
    assert sa == sb
    assert all(same(p, q) for one, two in zip(da, db) for p, q in zip(one, two))
    assert all(same(u, v) for u, v in zip(ba, bb))


def test_an_engine_repeats_itself_and_can_be_reinitialised(m):
    n, D, batch = 10, 2, 4
    seeds, others = seeds_for(batch), [s + 1 for s in seeds_for(batch)]
    with m.PSOBatchEngine("rosenbrock", batch, n, D, eps=10e-4, max_iter=300) as eng:
        x1, s1 = eng.minimize(-3.0, 3.0, seeds)
        x2, s2 = eng.minimize(-3.0, 3.0, seeds)
        x3, s3 = eng.minimize(-2.0, 3.0, others)
    assert same(x1, x2) and [status_tuple(s) for s in s1] == [status_tuple(s) for s in s2]
    with m.PSOBatchEngine("rosenbrock", batch, n, D, eps=10e-4, max_iter=300) as fresh:
        x4, s4 = fresh.minimize(-2.0, 3.0, others)
    assert same(x3, x4) and [status_tuple(s) for s in s3] == [status_tuple(s) for s in s4]
    assert not same(x1, x3)


@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_a_done_solve_is_a_no_op_under_further_steps(m, type_):
    n, D, batch = 10, 2, 8
    seeds = seeds_for(batch)
    with m.PSOBatchEngine("rosenbrock", batch, n, D, type=type_, eps=0.0, best_val_no_change=3,
                          max_iter=300) as eng:
        eng.init(-3.0, 3.0, seeds)
        snaps, at = {}, {}
        for t in range(16):
            eng.step(1)
            sts = eng.status()
            for b in range(batch):
                if sts[b].done and b not in snaps:
                    snaps[b], at[b] = (status_tuple(sts[b]), eng.download(b), eng.best()), t
        assert len(snaps) == batch and len(set(at.values())) >= 2  # they stopped at different turns
        eng.step(5)
        sts, best = eng.status(), eng.best()
        for b, (st, dl, (bx, bf, bi)) in snaps.items():
            assert status_tuple(sts[b]) == st, f"solve {b}"
            assert all(same(p, q) for p, q in zip(eng.download(b), dl)), f"solve {b}"
            assert same(best[0][b], bx[b]) and same(best[1][b], bf[b]) and best[2][b] == bi[b], f"solve {b}"


@pytest.mark.parametrize("obj,minimize", [("sphere", True), ("sphere", False), ("styblinski_tang", True),
                                          ("rastrigin", True)])
def test_other_objectives_and_maximize(m, oracle, obj, minimize):
    n, D, batch = 48, 20, 3
    seeds = seeds_for(batch)
    kw = dict(type=O.PSO_ACCELERATED, minimize=minimize, eps=0.0, max_iter=100, best_val_no_change=1000)
    with m.PSOBatchEngine(obj, batch, n, D, **kw) as eng:
        eng.init(-2.0, 3.0, seeds)
        eng.step(6)
        sts = eng.status()
        for b, s in enumerate(seeds):
            ref = O.PSOSyncRun(oracle, obj, n, D, -2.0, 3.0, seed=s, **kw)
            ref.step(6)
            pos, _, pbest, cur = eng.download(b)
            assert np.array_equal(pos, ref.pos) and np.array_equal(cur, ref.cur_val), f"solve {b}"
            assert np.array_equal(pbest, ref.pbest_val), f"solve {b}"
            assert sts[b].f_value == ref.s.gbest_val and sts[b].best_index == ref.s.gbest_idx, f"solve {b}"


def test_a_later_smaller_engine_does_not_lower_the_lds_opt_in(m):
    """The > 64 KiB dynamic-LDS opt-in belongs to the kernel instantiation (objective x lanes per
    particle x type), which every live engine of that class shares: an engine of 100 x 128
    (Accelerated, 106 KiB), then one of 5 x 128 in the same class, then the first one's solve --
    which must still be admitted and give the turn engine's bits."""
    D, batch, type_ = 128, 2, O.PSO_ACCELERATED
    args = dict(type=type_, eps=0.0, max_iter=4, best_val_no_change=1000)
    lo, hi = bounds_for(batch, D)
    seeds = seeds_for(batch)
    assert m.PSOBatchEngine.lds_bytes(100, D, type_) > 64 * 1024 > m.PSOBatchEngine.lds_bytes(5, D, type_)
    big = m.PSOBatchEngine("rosenbrock", batch, 100, D, **args)
    small = m.PSOBatchEngine("rosenbrock", batch, 5, D, **args)
    try:
        xs, ss = small.minimize(lo, hi, seeds)
        xb, sb = big.minimize(lo, hi, seeds)
    finally:
        small.close()
        big.close()
    for n, x, sts in ((100, xb, sb), (5, xs, ss)):
        for b, s in enumerate(seeds):
            xe = np.zeros(D)
            with m.PSOEngine("rosenbrock", n, D, seed=s, **args) as one:
                ste = one.minimize(xe, lo[b], hi[b])
            assert same(x[b], xe) and status_tuple(sts[b]) == status_tuple(ste), f"n {n}, solve {b}"


@pytest.mark.parametrize("batch,n,D,type_,code", [(3, 1025, 2, 1, 2), (3, 10, 129, 1, 2), (3, 0, 2, 1, 2),
                                                  (3, 10, 0, 1, 2), (0, 10, 2, 1, 1), (3, 10, 2, 5, 1),
                                                  (3, 1024, 8, 0, 2), (3, 1024, 128, 1, 2)])
def test_shapes_outside_the_ranges_are_rejected(m, batch, n, D, type_, code):
    with pytest.raises(m.NlsgError) as ei:
        m.PSOBatchEngine("rosenbrock", batch, n, D, type=type_)
    assert ei.value.code == code


# ---- 5. custom objectives --------------------------------------------------------------------------
ROSENBROCK_TERMS = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;"
HIMMELBLAU = "double a = x(0) * x(0) + x(1) - 11, b = x(0) + x(1) * x(1) - 7; return a * a + b * b;"


@pytest.mark.parametrize("n,D", [(10, 2), (37, 65), (40, 128)])
@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_custom_term_bodies_give_the_built_in_bits(m, n, D, type_):
    """Vanilla 40 x 128 takes 124 KiB: the opt-in above 64 KiB on the runtime-compiled kernel"""
    batch = 3
    lo, hi = bounds_for(batch, D)
    seeds = seeds_for(batch)
    kw = dict(type=type_, bounded=True, eps=0.0, max_iter=1000, best_val_no_change=1000)
    got = []
    for obj in (m.CustomObjective(ROSENBROCK_TERMS, chain=True), "rosenbrock"):
        with m.PSOBatchEngine(obj, batch, n, D, **kw) as eng:
            eng.init(lo, hi, seeds)
            eng.step(5)
            got.append(([eng.download(b) for b in range(batch)], eng.best(),
                        [status_tuple(s) for s in eng.status()]))
    (da, ba, sa), (db, bb, sb) = got
    assert all(same(p, q) for one, two in zip(da, db) for p, q in zip(one, two))
    assert all(same(u, v) for u, v in zip(ba, bb)) and sa == sb


@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
def test_custom_whole_vector_body_equals_the_turn_engine(m, type_):
    n, D, batch = 10, 2, 3
    obj = m.CustomObjective(HIMMELBLAU, vector=True)
    seeds = seeds_for(batch)
    args = dict(type=type_, eps=10e-4, max_iter=200, best_val_no_change=50)
    with m.PSOBatchEngine(obj, batch, n, D, **args) as eng:
        x, sts = eng.minimize(-5.0, 5.0, seeds)
    for b, s in enumerate(seeds):
        xe = np.zeros(D)
        with m.PSOEngine(obj, n, D, seed=s, **args) as one:
            ste = one.minimize(xe, -5.0, 5.0)
        assert same(x[b], xe) and status_tuple(sts[b]) == status_tuple(ste), f"solve {b}"


# ---- 6. the drop-in class and the C++ header -------------------------------------------------------
@pytest.mark.parametrize("type_", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("bounded", [False, True], ids=["unbounded", "bounded"])
def test_drop_in_resident_driver_equals_the_default(m, type_, bounded):
    xs, sts = [], []
    for driver in ("turns", "resident"):
        x = np.array([5.0, 7.0])
        solver = m.PSO("rosenbrock", None, type=type_, max_iter=300, driver=driver)
        st = solver.minimize(x, np.full(2, -3.0), np.full(2, 3.0)) if bounded else solver.minimize(x)
        sts.append(status_tuple(st))
        xs.append(x)
        assert solver.driver_used == driver
    assert same(xs[0], xs[1]) and sts[0] == sts[1]
    assert sts[0][1] > 0  # iterations


def test_drop_in_falls_back_when_the_swarm_does_not_fit(m):
    xs, sts = [], []
    for driver in ("turns", "resident"):
        x = 2.0 * (1.0 + 0.001 * np.arange(128))
        solver = m.PSO("rosenbrock", None, 0.8, 1.8, 1.8, 4096, 3, driver=driver)
        sts.append(status_tuple(solver.minimize(x)))
        xs.append(x)
        assert solver.driver_used == "turns"
    assert same(xs[0], xs[1]) and sts[0] == sts[1]


def test_header_resident_driver_equals_the_turn_driver(tmp_path):
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_pso_resident")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_pso_resident.cpp"), "-o", exe, "-ldl"])
    outs = {}
    for driver in ("resident", "turns"):
        env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH, NLSG_PSO_DRIVER=driver)
        outs[driver] = json.loads(subprocess.check_output([exe], env=env, text=True, timeout=300))
    assert outs["resident"] == outs["turns"]
    assert len(outs["turns"]["runs"]) == 4  # both types, both overloads
    for run in outs["turns"]["runs"]:
        assert run["iters"] > 0 and run["fcalls"] == 10 * (run["iters"] + 1)
    bad = subprocess.run([exe], env=dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH, NLSG_PSO_DRIVER="bogus"),
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0
    assert "NLSG_PSO_DRIVER must be turns or resident" in bad.stderr + bad.stdout
