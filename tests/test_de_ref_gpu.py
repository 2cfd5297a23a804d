"""Reference-order DE on the device (nlsg_de_ref_*): the reference's own runs and the oracle's
orc_de_serial (the reference's DE restated in C, pinned to the goldens) bit for bit — x, f, the
counters and the generator's final state."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nlsolver_amd
from nlsolver_amd import DE_BEST, DE_RANDOM
from tests import _oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nlsolver_amd", "libnlsolver_hip.so")
OBJ = {"rosenbrock": 0, "sphere": 1, "styblinski_tang": 2}
_C1_X0 = {"c1_random_pop40_x0_5_7": [5, 7], "random_pop50_x0_5_7": [5, 7],
          "example_best_pop50_x0_2_7": [2, 7]}
_TRACE_X0 = {"pop8_D4": 2.5, "pop40_D2": [5, 7], "pop64_D16": 4.096, "pop256_D128": 4.096}
README_TERM = "double t1 = xi; double t2 = (xn - xi * xi); return t1 * t1 + 100 * t2 * t2;"


def hx(v):
    return float.fromhex(v)


def default_state():
    return nlsolver_amd.XorShift().state


def oracle_run(oracle, obj, x0, state, *, minimize=True, strategy=DE_RANDOM, CR=0.9, F=0.8,
               eps=10e-4, pop=50, max_iter=1000, bvnc=50, log_cap=0):
    x = np.array(x0, dtype=np.float64)
    D = x.size
    g = O.XorShift()
    g.x[0], g.x[1] = state
    lg = None
    if log_cap:
        lx, lf = np.zeros((log_cap, D)), np.zeros(log_cap)
        lg = O.EvalLog(lx.ctypes.data_as(O.pd), lf.ctypes.data_as(O.pd), log_cap, 0, D)
    st = oracle.orc_de_serial(obj, int(minimize), strategy, x.ctypes.data_as(O.pd), D, C.byref(g),
                              CR, F, eps, pop, max_iter, bvnc, C.byref(lg) if lg else None)
    return st, x, (int(g.x[0]), int(g.x[1])), ((lx[:lg.count], lf[:lg.count]) if lg else None)


def device_run(objective, x0s, states, **kw):
    x0s = np.atleast_2d(np.asarray(x0s, dtype=np.float64))
    B, D = x0s.shape
    pop = kw.pop("pop", 50)
    with nlsolver_amd.DERefEngine(objective, B, pop, D, **kw) as eng:
        return eng.minimize(x0s, states)


def assert_same(oracle_result, x, st, state):
    ost, ox, ostate, _ = oracle_result
    assert st.function_calls_used == ost.function_calls_used
    assert st.iteration == ost.iteration
    assert st.f_value == ost.f_value or (np.isnan(st.f_value) and np.isnan(ost.f_value))
    assert np.array_equal(x, ox)
    assert tuple(int(v) for v in state) == ostate
    assert st.done == 1 and st.reserved == 0


def _next_two(state):
    g = nlsolver_amd.XorShift(tuple(int(v) for v in state))
    return [g(), g()]


@pytest.mark.parametrize("name", sorted(_C1_X0))
def test_c1_runs_of_the_reference(golden, name):
    case = golden("de_c1.json")[name]
    x, st, states = device_run("rosenbrock", [_C1_X0[name]], [default_state()], pop=case["pop"],
                               strategy=DE_RANDOM if case["strategy"] == "random" else DE_BEST,
                               CR=hx(case["CR"]), F=hx(case["F"]), eps=hx(case["eps"]),
                               max_iter=case["max_iter"], best_val_no_change=case["no_change"])
    assert (st[0].function_calls_used, st[0].iteration) == (case["fcalls"], case["iters"])
    assert st[0].f_value == hx(case["f"])
    assert list(x[0]) == [hx(v) for v in case["x"]]
    assert _next_two(states[0]) == [hx(v) for v in case["rng_after"]]


def test_readme_objective_as_custom_chain(golden):
    case = golden("de_c1.json")["readme_objective_pop40"]
    obj = nlsolver_amd.CustomObjective(README_TERM, chain=True)
    x, st, _ = device_run(obj, [[5, 7]], [default_state()], pop=40)
    assert (st[0].function_calls_used, st[0].iteration) == (case["fcalls"], case["iters"])
    assert st[0].f_value == hx(case["f"])
    assert list(x[0]) == [hx(v) for v in case["x"]]


def _fnv(arr):
    h = 1469598103934665603
    for b in np.ascontiguousarray(arr, dtype=np.float64).tobytes():
        h = ((h ^ b) * 1099511628211) & (2**64 - 1)
    return h


@pytest.mark.parametrize("strategy", ["random", "best"])
@pytest.mark.parametrize("shape", sorted(_TRACE_X0))
def test_reference_traces(golden, strategy, shape):
    case = golden("de_trace.json")[f"{strategy}_{shape}"]
    D, pop = case["D"], case["pop"]
    x0 = _TRACE_X0[shape]
    x0 = x0 if isinstance(x0, list) else [x0] * D
    cap = pop * (case["max_iter"] + 1)
    with nlsolver_amd.DERefEngine("rosenbrock", 1, pop, D,
                                  strategy=DE_RANDOM if strategy == "random" else DE_BEST,
                                  CR=hx(case["CR"]), F=hx(case["F"]), eps=hx(case["eps"]),
                                  max_iter=case["max_iter"], best_val_no_change=case["no_change"],
                                  log_capacity=cap) as eng:
        x, st, states = eng.minimize([x0], [default_state()])
        lx, lf, n = eng.log(0)
    assert n == st[0].function_calls_used == case["fcalls"]
    assert list(lf) == [hx(v) for v in case["eval_f"]]
    assert _fnv(lx) == int(case["eval_x_fnv"])
    assert st[0].iteration == case["iters"] and st[0].f_value == hx(case["f"])
    assert list(x[0]) == [hx(v) for v in case["x"]]
    assert _next_two(states[0]) == [hx(v) for v in case["rng_after"]]


def _random_state(rs):
    return tuple(int(v) for v in rs.integers(1, 2**64, size=2, dtype=np.uint64))


# the shape matrix pop {4 .. 4096} x D {1 .. 1025}, pruned: every pop and every D appears, with
# strategies, objectives and minimize / maximize rotated through; a few generations each
_SHAPES = [(4, 1), (4, 65), (5, 2), (5, 1025), (40, 63), (40, 128), (63, 64), (63, 1),
           (64, 65), (64, 1000), (65, 2), (65, 64), (256, 128), (256, 63), (4096, 2), (4096, 128)]


def shape_case(oracle, rs, obj, pop, D, gens, strategy, minimize, *, batch=1, log=False):
    """`batch` solves of `gens` generations from starts and generator states drawn from `rs`: x, status
    and final state equal the serial oracle's; with `log`, every evaluation's point and value too."""
    x0s = rs.uniform(-3, 3, (batch, D))
    states = [_random_state(rs) for _ in range(batch)]
    kw = dict(minimize=minimize, strategy=strategy, CR=0.9, F=0.8, eps=0.0, max_iter=gens)
    cap = pop * (gens + 1) if log else 0
    with nlsolver_amd.DERefEngine(obj, batch, pop, D, best_val_no_change=1000, log_capacity=cap, **kw) as eng:
        x, st, out = eng.minimize(x0s, states)
        logs = [eng.log(b) for b in range(batch)] if log else None
    for b in range(batch):
        want = oracle_run(oracle, OBJ[obj], x0s[b], states[b], pop=pop, bvnc=1000, log_cap=cap, **kw)
        assert_same(want, x[b], st[b], out[b])
        if log:
            lx, lf, n = logs[b]
            olx, olf = want[3]
            assert n == st[b].function_calls_used == len(olf), (pop, D, b)
            assert np.array_equal(lx, olx) and np.array_equal(lf, olf), (pop, D, b)


@pytest.mark.parametrize("pop, D", _SHAPES)
def test_shape_matrix_against_oracle(oracle, pop, D):
    rs = np.random.default_rng(pop * 10007 + D)
    k = _SHAPES.index((pop, D))
    obj = ["rosenbrock", "sphere", "styblinski_tang"][k % 3]
    for strategy, minimize in ((DE_RANDOM, k % 2 == 0), (DE_BEST, k % 2 == 1)):
        shape_case(oracle, rs, obj, pop, D, 3 if pop * D >= 100_000 else 6, strategy, minimize)


@pytest.mark.parametrize("strategy", [DE_BEST, DE_RANDOM])
def test_accepting_regimes(oracle, strategy):
    # CR 0.1 under `best`: the regime where the reference collapses in its first generation by
    # reading rows replaced moments earlier
    pop, D = 1024, 128
    rs = np.random.default_rng(5 + strategy)
    state = _random_state(rs)
    kw = dict(strategy=strategy, CR=0.1, F=0.5, eps=0.0, max_iter=20)
    want = oracle_run(oracle, 0, np.full(D, 0.6), state, pop=pop, bvnc=1000, **kw)
    x, st, states = device_run("rosenbrock", [np.full(D, 0.6)], [state], pop=pop, best_val_no_change=1000, **kw)
    assert_same(want, x[0], st[0], states[0])


def test_batch_of_64_solves(oracle):
    rs = np.random.default_rng(64)
    B, pop, D = 64, 40, 8
    x0s = rs.uniform(-5, 5, (B, D))
    states = [_random_state(rs) for _ in range(B)]
    x, st, out_states = device_run("rosenbrock", x0s, states, pop=pop, max_iter=200)
    for b in range(B):
        want = oracle_run(oracle, 0, x0s[b], states[b], pop=pop, max_iter=200)
        assert_same(want, x[b], st[b], out_states[b])


def test_python_de_reference_generation_advances_the_generator(golden):
    case = golden("de_c1.json")["c1_random_pop40_x0_5_7"]
    gen = nlsolver_amd.XorShift()
    x = np.array([5.0, 7.0])
    st = nlsolver_amd.DE("rosenbrock", gen, 0.9, 0.8, 10e-4, 40, generation="reference").minimize(x)
    assert (st.function_calls_used, st.iteration, st.f_value) == (case["fcalls"], case["iters"], hx(case["f"]))
    assert list(x) == [hx(v) for v in case["x"]]
    assert [gen(), gen()] == [hx(v) for v in case["rng_after"]]


def test_maximize_and_custom_terms_against_oracle(oracle):
    # Styblinski-Tang as a CustomObjective of terms, maximised: f_multiplier -1 (nlsolver.h:2418)
    obj = nlsolver_amd.CustomObjective("double x2 = xi * xi; return x2 * x2 - 16 * x2 + 5 * xi;",
                                       finish_body="return s / 2.0;")
    state = (0x123456789ABCDEF, 0xFEDCBA987654321)
    x0 = np.linspace(-2, 2, 24)
    kw = dict(minimize=False, strategy=DE_BEST, eps=0.0, max_iter=30)
    want = oracle_run(oracle, 2, x0, state, pop=48, bvnc=1000, **kw)
    x, st, states = device_run(obj, [x0], [state], pop=48, best_val_no_change=1000, **kw)
    assert_same(want, x[0], st[0], states[0])


def test_degenerate_state_hits_the_donor_cap():
    # the all-zero xorshift state draws 0.0 forever: the reference's donor pick would spin; the
    # engine ends that solve with a flag, and the other solve of the batch is unaffected
    with nlsolver_amd.DERefEngine("sphere", 2, 8, 3, eps=0.0, max_iter=5) as eng:
        with pytest.raises(nlsolver_amd.NlsgError) as ei:
            eng.minimize(np.ones((2, 3)), [(0, 0), default_state()])
    assert ei.value.code == 2 and "solve 0" in str(ei.value)


def test_header_reference_generation_returns_c1(golden, tmp_path):
    exe = str(tmp_path / "header_de_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_de_ref.cpp"), "-o", exe, "-ldl"])
    env = dict(os.environ, NLSG_LIBRARY=LIB, NLSG_DE_GENERATION="reference")
    hiprtc = nlsolver_amd.de.rtc_library_path()
    if hiprtc:
        env["NLSG_HIPRTC"] = hiprtc
    out = json.loads(subprocess.check_output([exe, "c1"], env=env, text=True, timeout=300))
    gold = golden("de_c1.json")
    for name in sorted(_C1_X0):
        g, o = gold[name], out[name]
        assert (o["fcalls"], o["iters"], o["f"], o["x"]) == (g["fcalls"], g["iters"], g["f"], g["x"]), name
        assert o["rng_after"] == g["rng_after"], name
    g, o = gold["readme_objective_pop40"], out["readme_objective_pop40"]
    assert (o["fcalls"], o["iters"], o["f"], o["x"]) == (g["fcalls"], g["iters"], g["f"], g["x"])


_CHILD = r"""
import json, sys
import numpy as np
import nlsolver_amd
x0 = np.linspace(-1.5, 2.5, 33)
with nlsolver_amd.DERefEngine("rosenbrock", 2, 70, 33, eps=0.0, max_iter=15) as eng:
    x, st, states = eng.minimize(np.stack([x0, -x0]), [(11, 22), (33, 44)])
print(json.dumps({"x": [[v.hex() for v in r] for r in x], "f": [s.f_value.hex() for s in st],
                  "fc": [s.function_calls_used for s in st], "it": [s.iteration for s in st],
                  "st": [[int(v) for v in s] for s in states]}))
"""


def test_poisoned_pool_still_matches_oracle(oracle):
    out = json.loads(subprocess.check_output([sys.executable, "-c", _CHILD], cwd=ROOT, text=True, timeout=300,
                                             env=dict(os.environ, NLSG_POOL_POISON="1")))
    x0 = np.linspace(-1.5, 2.5, 33)
    for b, (xb, sb) in enumerate(((x0, (11, 22)), (-x0, (33, 44)))):
        ost, ox, ostate, _ = oracle_run(oracle, 0, xb, sb, pop=70, eps=0.0, max_iter=15)
        assert [hx(v) for v in out["x"][b]] == list(ox)
        assert hx(out["f"][b]) == ost.f_value
        assert (out["fc"][b], out["it"][b]) == (ost.function_calls_used, ost.iteration)
        assert tuple(out["st"][b]) == ostate
