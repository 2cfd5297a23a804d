"""The resident batch DE engine (DEBatchEngine / nlsg_de_batch_*): every solve of a batch is the
keyed engine's solve of its seed, bit for bit -- against the restatement orc_de_sync_*
(tests._oracle.DESyncRun) and against DEEngine itself.

Sizes are the smallest at which a mapping, a pass boundary or a rule changes: pop 4 (the slow donor
path), G = 4 / 8 / 16 / 32 lanes per agent and the first one-wave-per-agent dimension (65), odd D,
populations that are no multiple of the agents per pass, 1023 / 1024 (the ragged and the full last
stride of the 256-thread sums)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import _oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 12374563468
LDS_BUDGET = 160 * 1024


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


def x0_for(D, val=0.6):
    return val * (1.0 + 0.001 * np.arange(D))


STATUS_FIELDS = ("f_value", "iteration", "function_calls_used", "best_index", "val_no_change", "std_err",
                 "done")


def status_tuple(st):
    """the seven fields, std_err as its bit pattern (NaN when it was not evaluated)"""
    return tuple(np.float64(getattr(st, f)).view(np.uint64) if f in ("f_value", "std_err")
                 else int(getattr(st, f)) for f in STATUS_FIELDS)


def counters(st):
    return (st.iteration, st.function_calls_used, st.best_index, st.val_no_change)


def follow_restatement(m, oracle, obj, pop, D, batch, turns, *, x0, kw, label=""):
    """init and `turns` single turns: every solve's generation and counters equal its DESyncRun;
    one more turn, then best(). Returns the number of accepted trials over the run."""
    seeds = seeds_for(batch)
    refs = [O.DESyncRun(oracle, obj, pop, D, x0, seed=s, **kw) for s in seeds]
    accepted = 0
    with m.DEBatchEngine(obj, batch, pop, D, **kw) as eng:
        eng.init(np.tile(x0, (batch, 1)), seeds)
        sts = eng.status()
        for b, ref in enumerate(refs):
            P, S = eng.download(b)
            assert np.array_equal(P, ref.population), f"{label} init population, solve {b}"
            assert np.array_equal(S, ref.scores), f"{label} init scores, solve {b}"
            assert counters(sts[b]) == (ref.s.iter, ref.s.fcalls, ref.s.best_id, ref.s.val_no_change), \
                f"{label} init, solve {b}"
        for g in range(turns):
            before = [ref.scores.copy() for ref in refs]
            eng.step(1)
            sts = eng.status()
            for b, ref in enumerate(refs):
                ref.step(1)
                P, S = eng.download(b)
                assert np.array_equal(P, ref.population), f"{label} population gen {g}, solve {b}"
                assert np.array_equal(S, ref.scores), f"{label} scores gen {g}, solve {b}"
                assert counters(sts[b]) == (ref.s.iter, ref.s.fcalls, ref.s.best_id, ref.s.val_no_change), \
                    f"{label} gen {g}, solve {b}"
                accepted += int(np.sum(S != before[b]))
        eng.step(1)  # one more scan so best() reflects the last generation
        bx, bf, bi = eng.best()
        for b, ref in enumerate(refs):
            # best() is as of the head: the generation the head scanned, not the one the turn then made
            scanned_pop, scanned_scores = ref.population.copy(), ref.scores.copy()
            ref.step(1)
            assert bi[b] == ref.s.best_id and bf[b] == scanned_scores[bi[b]], f"{label} best, solve {b}"
            assert np.array_equal(bx[b], scanned_pop[bi[b]]), f"{label} best row, solve {b}"
    return accepted


# ---- 1. generations against the restatement ------------------------------------------------------
SHAPES = [(4, 1), (4, 3), (5, 3), (40, 2), (100, 5), (64, 16), (37, 64), (37, 65), (70, 128), (257, 8),
          (1023, 2), (1024, 4)]


@pytest.mark.parametrize("pop,D", SHAPES)
@pytest.mark.parametrize("strategy", [0, 1], ids=["best", "random"])
def test_generations_follow_the_restatement(m, oracle, pop, D, strategy):
    """The accepting regime of test_rows_longer_than_1024_coordinates_bit_exact (CR 0.2, F 0.5, a
    tight start): both the store of a trial and the copy of a surviving row run."""
    batch = 3
    kw = dict(strategy=strategy, CR=0.2, F=0.5, eps=0.0, max_iter=1000, best_val_no_change=1000)
    accepted = follow_restatement(m, oracle, "rosenbrock", pop, D, batch, 4, x0=x0_for(D), kw=kw)
    if D == 1:  # the Rosenbrock chain has no term in one dimension: f = 0 everywhere, nothing is '< 0'
        assert accepted == 0  # (4, 3) is the pop-4 shape whose population does move
    else:
        assert 0 < accepted < 4 * pop * batch


# ---- 2. other objectives and maximise -------------------------------------------------------------
@pytest.mark.parametrize("obj,minimize", [("sphere", True), ("sphere", False), ("styblinski_tang", True),
                                          ("rastrigin", True)])
def test_other_objectives_and_maximize(m, oracle, obj, minimize):
    pop, D, batch = 96, 48, 3
    x0 = x0_for(D, 3.0)
    kw = dict(minimize=minimize, eps=0.0, best_val_no_change=1000)
    seeds = seeds_for(batch)
    with m.DEBatchEngine(obj, batch, pop, D, **kw) as eng:
        eng.init(np.tile(x0, (batch, 1)), seeds)
        eng.step(6)
        for b, s in enumerate(seeds):
            ref = O.DESyncRun(oracle, obj, pop, D, x0, seed=s, **kw)
            ref.step(6)
            P, S = eng.download(b)
            assert np.array_equal(P, ref.population) and np.array_equal(S, ref.scores), f"solve {b}"


# ---- 3. whole solves to the stop, independently per solve ----------------------------------------
def restatement_to_done(oracle, obj, pop, D, x0, seed, **kw):
    ref = O.DESyncRun(oracle, obj, pop, D, x0, seed=seed, **kw)
    while not ref.s.done:
        ref.step()
    return ref


def assert_solve_is(ref, x, st, eps, tag):
    assert st.done == 1, tag
    assert (st.iteration, st.function_calls_used, st.best_index) == (ref.s.iter, ref.s.fcalls, ref.s.best_id), tag
    assert st.f_value == ref.scores[ref.s.best_id], tag
    assert np.array_equal(x, ref.best_x), tag
    if eps > 0:
        assert st.std_err == ref.s.std_err, tag


STOPS = [dict(eps=10e-4), dict(eps=0.0, max_iter=7), dict(eps=0.0, best_val_no_change=3), dict(eps=0.5)]


@pytest.mark.parametrize("kw", STOPS, ids=["eps", "max_iter", "no_change", "eps_at_once"])
@pytest.mark.parametrize("strategy", [0, 1], ids=["best", "random"])
def test_whole_solves_stop_where_the_restatement_stops(m, oracle, kw, strategy):
    pop, D, batch = 40, 2, 8
    args = dict(eps=10e-4, max_iter=1000, best_val_no_change=50, strategy=strategy)
    args.update(kw)
    x0 = np.array([5.0, 7.0])
    seeds = seeds_for(batch)
    refs = [restatement_to_done(oracle, "rosenbrock", pop, D, x0, s, **args) for s in seeds]
    with m.DEBatchEngine("rosenbrock", batch, pop, D, **args) as eng:
        x, sts = eng.minimize(np.tile(x0, (batch, 1)), seeds)
    for b, ref in enumerate(refs):
        assert_solve_is(ref, x[b], sts[b], args["eps"], f"solve {b}")
    if kw == dict(eps=10e-4):  # a solve that is done stays frozen while its neighbours go on
        assert len({int(r.s.iter) for r in refs}) >= 2


@pytest.mark.parametrize("obj,pop,D", [("sphere", 50, 8), ("styblinski_tang", 100, 5)])
def test_longer_solves_stop_where_the_restatement_stops(m, oracle, obj, pop, D):
    batch = 4
    args = dict(eps=10e-4, max_iter=1000, best_val_no_change=50)
    x0 = x0_for(D, 3.0)
    seeds = seeds_for(batch)
    with m.DEBatchEngine(obj, batch, pop, D, **args) as eng:
        x, sts = eng.minimize(np.tile(x0, (batch, 1)), seeds)
    for b, s in enumerate(seeds):
        assert_solve_is(restatement_to_done(oracle, obj, pop, D, x0, s, **args), x[b], sts[b], args["eps"],
                        f"solve {b}")


# ---- 4. equality with DEEngine itself --------------------------------------------------------------
@pytest.mark.parametrize("pop,D", [(40, 2), (64, 16), (70, 128)])
def test_minimize_equals_the_turn_engine(m, pop, D):
    batch = 4
    x0 = np.array([5.0, 7.0]) if D == 2 else x0_for(D, 2.0)
    args = dict(eps=10e-4, max_iter=60, best_val_no_change=50)
    seeds = seeds_for(batch)
    with m.DEBatchEngine("rosenbrock", batch, pop, D, **args) as eng:
        x, sts = eng.minimize(np.tile(x0, (batch, 1)), seeds)
    for b, s in enumerate(seeds):
        xe = x0.copy()
        with m.DEEngine("rosenbrock", pop, D, seed=s, **args) as one:
            ste = one.minimize(xe)
        assert np.array_equal(x[b], xe), f"solve {b}"
        assert status_tuple(sts[b]) == status_tuple(ste), f"solve {b}"


# ---- 5. launch cuts do not change anything ---------------------------------------------------------
def test_launch_cuts_change_nothing(m):
    pop, D, batch = 40, 2, 8
    x0 = np.tile([5.0, 7.0], (batch, 1))
    seeds = seeds_for(batch)
    outs = []
    for tpl in (1, 5, 0):
        with m.DEBatchEngine("rosenbrock", batch, pop, D, eps=10e-4, turns_per_launch=tpl) as eng:
            x, sts = eng.minimize(x0, seeds)
        outs.append((x, [status_tuple(s) for s in sts]))
    for x, sts in outs[1:]:
        assert np.array_equal(x, outs[0][0]) and sts == outs[0][1]
    states = []
    for steps in ((3, 4), (7,)):
        with m.DEBatchEngine("rosenbrock", batch, pop, D, eps=10e-4, turns_per_launch=2) as eng:
            eng.init(x0, seeds)
            for t in steps:
                eng.step(t)
            states.append(([status_tuple(s) for s in eng.status()], [eng.download(b) for b in range(batch)],
                           eng.best()))
    (sa, da, ba), (sb, db, bb) = states
    assert sa == sb
    assert all(np.array_equal(p, q) and np.array_equal(s, t) for (p, s), (q, t) in zip(da, db))
    assert all(np.array_equal(u, v) for u, v in zip(ba, bb))


# ---- 6. determinism and reuse ----------------------------------------------------------------------
def test_an_engine_repeats_itself_and_can_be_reused(m):
    pop, D, batch = 40, 2, 4
    x0 = np.tile([5.0, 7.0], (batch, 1))
    seeds, others = seeds_for(batch), [s + 1 for s in seeds_for(batch)]
    with m.DEBatchEngine("rosenbrock", batch, pop, D, eps=10e-4) as eng:
        x1, s1 = eng.minimize(x0, seeds)
        x2, s2 = eng.minimize(x0, seeds)
        x3, s3 = eng.minimize(x0, others)
    assert np.array_equal(x1, x2) and [status_tuple(s) for s in s1] == [status_tuple(s) for s in s2]
    with m.DEBatchEngine("rosenbrock", batch, pop, D, eps=10e-4) as fresh:
        x4, s4 = fresh.minimize(x0, others)
    assert np.array_equal(x3, x4) and [status_tuple(s) for s in s3] == [status_tuple(s) for s in s4]
    assert not np.array_equal(x1, x3)


# ---- 7. limits -------------------------------------------------------------------------------------
def test_the_largest_population_at_128_coordinates(m, oracle):
    D = 128
    fits = [pop for pop in range(4, 1025) if 0 < m.DEBatchEngine.lds_bytes(pop, D) <= LDS_BUDGET]
    pop = max(fits)
    assert fits == list(range(4, pop + 1))
    kw = dict(strategy=1, CR=0.2, F=0.5, eps=0.0, max_iter=1000, best_val_no_change=1000)
    follow_restatement(m, oracle, "rosenbrock", pop, D, 3, 2, x0=x0_for(D), kw=kw, label="largest")
    with pytest.raises(m.NlsgError) as ei:
        m.DEBatchEngine("rosenbrock", 3, pop + 1, D)
    assert ei.value.code == 2


@pytest.mark.parametrize("batch,pop,D", [(3, 1025, 2), (3, 40, 129), (3, 3, 2), (0, 40, 2)])
def test_shapes_outside_the_ranges_are_rejected(m, batch, pop, D):
    with pytest.raises(m.NlsgError) as ei:
        m.DEBatchEngine("rosenbrock", batch, pop, D)
    assert ei.value.code == (1 if batch == 0 else 2)


def test_a_later_smaller_engine_does_not_lower_the_lds_opt_in(m, oracle):
    """The > 64 KiB dynamic-LDS opt-in belongs to the kernel instantiation (objective x lanes per
    agent), which every live engine of that class shares: an engine of 70 x 128 (143 KiB), then one
    of 10 x 128 in the same class, then the first one's solve -- which must still be admitted and
    give the restatement's bits."""
    D, batch = 128, 2
    args = dict(CR=0.2, F=0.5, eps=0.0, max_iter=4, best_val_no_change=1000)
    x0 = x0_for(D)
    seeds = seeds_for(batch)
    assert m.DEBatchEngine.lds_bytes(70, D) > 64 * 1024 > m.DEBatchEngine.lds_bytes(10, D)
    big = m.DEBatchEngine("rosenbrock", batch, 70, D, **args)
    small = m.DEBatchEngine("rosenbrock", batch, 10, D, **args)
    try:
        xs, ss = small.minimize(np.tile(x0, (batch, 1)), seeds)
        xb, sb = big.minimize(np.tile(x0, (batch, 1)), seeds)
    finally:
        small.close()
        big.close()
    for pop, x, sts in ((70, xb, sb), (10, xs, ss)):
        for b, s in enumerate(seeds):
            assert_solve_is(restatement_to_done(oracle, "rosenbrock", pop, D, x0, s, **args), x[b], sts[b],
                            0.0, f"pop {pop}, solve {b}")


# ---- 8. custom objectives --------------------------------------------------------------------------
ROSENBROCK_TERMS = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;"
HIMMELBLAU = "double a = x(0) * x(0) + x(1) - 11, b = x(0) + x(1) * x(1) - 7; return a * a + b * b;"


@pytest.mark.parametrize("pop,D", [(40, 2), (37, 65), (70, 128)])
def test_custom_term_bodies_give_the_built_in_bits(m, pop, D):
    """(70, 128) takes 143 KiB: the opt-in above 64 KiB on the runtime-compiled kernel's function"""
    batch = 3
    x0 = np.tile(x0_for(D), (batch, 1))
    seeds = seeds_for(batch)
    kw = dict(CR=0.2, F=0.5, eps=0.0, max_iter=1000, best_val_no_change=1000)
    got = []
    for obj in (m.CustomObjective(ROSENBROCK_TERMS, chain=True), "rosenbrock"):
        with m.DEBatchEngine(obj, batch, pop, D, **kw) as eng:
            eng.init(x0, seeds)
            eng.step(5)
            got.append(([eng.download(b) for b in range(batch)], eng.best()))
    (da, ba), (db, bb) = got
    assert all(np.array_equal(p, q) and np.array_equal(s, t) for (p, s), (q, t) in zip(da, db))
    assert all(np.array_equal(u, v) for u, v in zip(ba, bb))


def test_custom_whole_vector_body_equals_the_turn_engine(m):
    pop, D, batch = 40, 2, 3
    obj = m.CustomObjective(HIMMELBLAU, vector=True)
    x0 = np.array([5.0, 7.0])
    seeds = seeds_for(batch)
    args = dict(eps=10e-4, max_iter=200, best_val_no_change=50)
    with m.DEBatchEngine(obj, batch, pop, D, **args) as eng:
        x, sts = eng.minimize(np.tile(x0, (batch, 1)), seeds)
    for b, s in enumerate(seeds):
        xe = x0.copy()
        with m.DEEngine(obj, pop, D, seed=s, **args) as one:
            ste = one.minimize(xe)
        assert np.array_equal(x[b], xe) and status_tuple(sts[b]) == status_tuple(ste), f"solve {b}"


# ---- 9. the drop-in class and the C++ header -------------------------------------------------------
def test_drop_in_resident_driver_equals_the_default(m):
    xs, sts = [], []
    for driver in ("turns", "resident"):
        x = np.array([5.0, 7.0])
        solver = m.DE("rosenbrock", None, 0.9, 0.8, 10e-4, 40, driver=driver)
        sts.append(status_tuple(solver.minimize(x)))
        xs.append(x)
        assert solver.driver_used == driver
    assert np.array_equal(xs[0], xs[1]) and sts[0] == sts[1]


def test_drop_in_falls_back_when_the_population_does_not_fit(m):
    xs, sts = [], []
    for driver in ("turns", "resident"):
        x = x0_for(128, 2.0)
        solver = m.DE("rosenbrock", None, 0.9, 0.8, 10e-4, 4096, max_iter=3, driver=driver)
        sts.append(status_tuple(solver.minimize(x)))
        xs.append(x)
        assert solver.driver_used == "turns"
    assert np.array_equal(xs[0], xs[1]) and sts[0] == sts[1]


def test_header_resident_driver_equals_the_turn_driver(tmp_path):
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_de_resident")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_de_resident.cpp"), "-o", exe, "-ldl"])
    outs = {}
    for driver in ("resident", "turns"):
        env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH, NLSG_DE_DRIVER=driver)
        outs[driver] = json.loads(subprocess.check_output([exe], env=env, text=True, timeout=300))
    assert outs["resident"] == outs["turns"]
    assert outs["turns"]["iters"] > 0 and outs["turns"]["fcalls"] == 40 * (outs["turns"]["iters"] + 1)
    bad = subprocess.run([exe], env=dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH, NLSG_DE_DRIVER="bogus"),
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0
    assert "NLSG_DE_DRIVER must be turns or resident" in bad.stderr + bad.stdout
