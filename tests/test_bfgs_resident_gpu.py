"""NLSG_BFGS_RESIDENT on the device: the whole loop of a solve in one kernel, a workgroup per problem with
its inverse Hessian in LDS. Every comparison is BIT FOR BIT with the lock-step BFGSEngine of the same
configuration driven by the same calls — that engine is pinned to the oracle and to the reference
(test_bfgs_gpu, test_reference_order_gpu), so it is the yardstick here — and, for the reference's own runs,
with the committed fixtures directly.

The inverse Hessian is compared from the first update on: before it neither engine has written H (the
identity is synthesised, never stored), and download_state() returns whatever the pool's block held."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle as O
from tests.test_oracle_golden import hx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "rosenbrock", 1: "sphere", 2: "styblinski_tang"}
ROSEN_TERM = "double t1 = 1 - xi; double t2 = xn - xi * xi; return t1 * t1 + 100 * t2 * t2;"
ROSEN_GRAD = ("double g = 0.0; if (i + 1 < D) g = -2.0 * (1.0 - xi) - 400.0 * xi * (xn - xi * xi);"
              " if (i > 0) g = g + 200.0 * (xi - xm * xm); return g;")


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available()
    import nlsolver_amd
    return nlsolver_amd


# ---- helpers -----------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def status(st):
    """every field of every Status, the doubles as their bit patterns"""
    out = []
    for s in st:
        row = []
        for name, _ in type(s)._fields_:
            v = getattr(s, name)
            row.append(int(np.float64(v).view(np.uint64)) if isinstance(v, float) else int(v))
        out.append(tuple(row))
    return out


def starts(n, B):
    """every problem another start, no two neighbours alike"""
    return np.array([[(1 + 0.25 * b + 0.01 * ((7 * i + 3 * b) % 11)) * (-1.0 if i % 3 == 0 else 1.0)
                      for i in range(n)] for b in range(B)])


def spread_starts(n, B=6):
    """starts of very different sizes: their problems stop at different iterations"""
    return starts(n, B) * np.array([10.0 ** (b - 2) for b in range(B)])[:, None]


def objective(mod, name, n):
    """(objective, engine keywords)"""
    if name == "quad":
        d, b, c = O.quad_problem(n)
        return mod.QuadDiagRank1(d, b, c), {}
    return name, dict(dim=n)


def state(eng):
    x, st = eng.download()
    g, H = eng.download_state()
    return dict(x=x, g=g, H=H, status=status(st), identity=eng.identity_count(), open=eng.unfinished(),
                iters=[s.iteration for s in st])


def assert_same_state(a, b, what):
    assert same(a["x"], b["x"]), (what, "x")
    assert same(a["g"], b["g"]), (what, "g")
    assert a["status"] == b["status"], (what, "status")
    assert (a["identity"], a["open"]) == (b["identity"], b["open"]), (what, "identity_count / unfinished")
    if min(a["iters"]) >= 1:      # (see the module's text)
        assert same(a["H"], b["H"]), (what, "H")


def pair(mod, obj, batch, **kw):
    return mod.BFGSEngine(obj, batch, **kw), mod.BFGSEngine(obj, batch, resident=True, **kw)


def turns_case(mod, name, n, ref, calls=(1, 2, 4), B=5, **kw):
    """init and the step calls on both engines, the whole state compared after each"""
    obj, okw = objective(mod, name, n)
    x0 = starts(n, B)
    lock, res = pair(mod, obj, B, reference_order=ref, **okw, **kw)
    with lock, res:
        assert res.resident and not lock.resident
        lock.init(x0)
        res.init(x0)
        assert_same_state(state(lock), state(res), "init")
        for k in calls:
            lock.step(k)
            res.step(k)
            a = state(lock)
            assert_same_state(a, state(res), f"step({k})")
        assert max(a["iters"]) >= 1
    return a


# ---- 1: state after k turns ----------------------------------------------------------------------------
CASES_1 = [("quad", n, False) for n in (1, 2, 3, 33, 63, 64)] + \
          [("quad", n, True) for n in (1, 2, 31, 64)] + \
          [("rosenbrock", n, True) for n in (2, 3, 17, 64)] + \
          [("rosenbrock", n, False) for n in (2, 64)] + \
          [("sphere", 1, False), ("sphere", 1, True)]


@pytest.mark.parametrize("name,n,ref", CASES_1)
def test_state_after_k_turns_equals_the_lock_step_engines(mod, name, n, ref):
    turns_case(mod, name, n, ref)


def test_time_steps_is_unsupported_and_the_flag_is_set(mod):
    from nlsolver_amd import NlsgError
    obj, kw = objective(mod, "quad", 8)
    with mod.BFGSEngine(obj, 2, resident=True, **kw) as eng:
        assert eng.cfg.flags == 4
        eng.init(starts(8, 2))
        with pytest.raises(NlsgError) as err:
            eng.time_steps(1)
        assert err.value.code == 2
        eng.step(1)                                   # and the engine goes on
        assert [s.iteration for s in eng.download()[1]] == [1, 1]
    with pytest.raises(NlsgError) as err:
        mod.BFGSEngine(obj, 2, resident=True, symmetric=True, **kw)
    assert err.value.code == 1
    d, b, c = O.quad_problem(65)
    with pytest.raises(NlsgError) as err:
        mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), 2, resident=True)
    assert err.value.code == 2 and "64" in str(err.value)


# ---- 2: launch cuts do not show ------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,ref", [("quad", 33, False), ("rosenbrock", 5, True)])
def test_launch_cuts_do_not_show(mod, name, n, ref):
    obj, kw = objective(mod, name, n)
    x0 = starts(n, 5)
    max_iter = 300                                    # max_iter + 1 turns: past the cut of 256 turns per launch
    ekw = dict(reference_order=ref, resident=True, max_iter=max_iter, grad_eps=0.0, **kw)   # (no early stop)
    with mod.BFGSEngine(obj, 5, **ekw) as a, mod.BFGSEngine(obj, 5, **ekw) as b:
        a.init(x0)
        b.init(x0)
        for _ in range(7):
            a.step(1)
        b.step(7)
        assert_same_state(state(a), state(b), "7 x step(1) against step(7)")
        x, st = a.minimize(x0.copy())
        ma = state(a)
        b.init(x0)
        b.step(max_iter + 1)
        mb = state(b)
        assert_same_state(ma, mb, "minimize against init + step(max_iter + 1)")
        assert same(x, mb["x"]) and status(st) == mb["status"] and mb["open"] == 0


# ---- 3: whole solves -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [False, True])
@pytest.mark.parametrize("name,n", [("quad", 8), ("quad", 64), ("rosenbrock", 4)])
def test_whole_solves_equal_the_lock_step_engines(mod, name, n, ref):
    obj, kw = objective(mod, name, n)
    x0 = spread_starts(n)
    lock, res = pair(mod, obj, 6, reference_order=ref, **kw)
    with lock, res:
        xl, sl = lock.minimize(x0.copy())
        xr, sr = res.minimize(x0.copy())
        iters = [s.iteration for s in sl]
        print(name, n, ref, "iterations", iters)
        assert len(set(iters)) >= 2, iters            # the problems stop at different iterations
        assert all(s.done for s in sl)
        assert same(xl, xr) and status(sl) == status(sr)
        assert_same_state(state(lock), state(res), "after minimize")


# ---- 4: the reset guard and the identity shortcut inside the loop ----------------------------------------
# (from a scan of the lock-step engine: with d scaled by 100 and a first trial step of 4 every one of the five
# problems trips the guard in turn 15, on finite values; the test asserts that the guard fires)
RESET_CASE = dict(n=33, alpha=4.0, scale=100.0)


@pytest.mark.parametrize("ref", [False, True])
def test_reset_guard_inside_the_loop(mod, ref):
    n = RESET_CASE["n"]
    d, b, c = O.quad_problem(n)
    obj = mod.QuadDiagRank1(d * RESET_CASE["scale"], b, c)
    x0 = starts(n, 5)
    kw = dict(reference_order=ref, alpha=RESET_CASE["alpha"], max_iter=40)
    lock, res = pair(mod, obj, 5, **kw)
    with lock, res:
        lock.init(x0)
        k = None
        for turn in range(1, 31):
            lock.step(1)
            if turn >= 2 and lock.identity_count() > 0 and lock.unfinished() == 5:
                k = turn                              # the guard fired in turn k: k - 1 >= 1 updates came before
                break
        assert k is not None, "no reset in 30 turns: the case went stale"
        ak = state(lock)
        assert np.isfinite(ak["H"]).all() and np.isfinite(ak["g"]).all()
        res.init(x0)
        res.step(k)                                   # the reset happens INSIDE the launch's loop
        assert_same_state(ak, state(res), f"after turn {k}")
        lock.step(1)
        res.step(1)
        assert_same_state(state(lock), state(res), f"after turn {k + 1}")


# ---- 5: the reference's runs -----------------------------------------------------------------------------
def start(g):
    return hx(g["x0"]) + hx(g["x0_step"]) * np.arange(g["n"], dtype=np.float64)


@pytest.mark.parametrize("name", ["n8", "n64", "n64_default_stop"])
def test_analytic_gradient_runs_of_the_reference(mod, golden, name):
    g = golden("bfgs.json")[name]
    n = g["n"]
    assert n <= 64
    d, b, c = O.quad_problem(n)
    x = start(g).reshape(1, -1)
    with mod.BFGSEngine(mod.QuadDiagRank1(d, b, c), 1, max_iter=g["max_iter"], grad_eps=hx(g["grad_eps"]),
                        alpha=hx(g["alpha"]), reference_order=True, resident=True) as eng:
        x, st = eng.minimize(x)
    assert (st[0].iteration, st[0].function_calls_used, st[0].gradient_evals_used) == \
        (g["iters"], g["fcalls"], g["gcalls"])
    assert st[0].f_value == hx(g["f"])
    assert x[0][:8].tolist() == [hx(v) for v in g["x_head"]]
    h = 1469598103934665603  # FNV-1a over the bytes of the whole x, as the reference driver hashed it
    for byte in np.ascontiguousarray(x[0]).view(np.uint8).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert h == int(g["x_fnv"])


@pytest.mark.parametrize("name", ["rosenbrock_n2", "rosenbrock_n4", "rosenbrock_n16_default_stop", "sphere_n5",
                                  "styblinski_tang_n8"])
def test_default_gradient_runs_of_the_reference(mod, golden, name):
    g = golden("bfgs_fd.json")[name]
    assert g["n"] <= 64
    x = start(g).reshape(1, -1)
    with mod.BFGSEngine(NAMES[g["objective"]], 1, dim=g["n"], max_iter=g["max_iter"], grad_eps=hx(g["grad_eps"]),
                        alpha=hx(g["alpha"]), reference_order=True, resident=True) as eng:
        x, st = eng.minimize(x)
    assert (st[0].iteration, st[0].function_calls_used, st[0].gradient_evals_used) == \
        (g["iters"], g["fcalls"], g["gcalls"])
    assert st[0].f_value == hx(g["f"])
    assert x[0].tolist() == [hx(v) for v in g["x"]]


# ---- 6: compiled objectives ------------------------------------------------------------------------------
def rosen_starts(D, B):
    return np.array([[-1.2 + 0.1 * b + 0.125 * ((5 * i + 3 * b) % 17) for i in range(D)] for b in range(B)])


def custom_case(mod, obj, n, ref, x0, rows=None, resident_first=False, steps=(1, 2, 4), **kw):
    """the states after init and the step calls, then a whole solve; rows: one [batch, n_params] array per
    round, the second replacing the first without a rebuild"""
    B = x0.shape[0]
    made = []
    for resident in ((True, False) if resident_first else (False, True)):
        made.append(mod.BFGSEngine(obj, B, dim=n, reference_order=ref, resident=resident, **kw))
    lock, res = (made[1], made[0]) if resident_first else (made[0], made[1])
    with lock, res:
        assert lock.gradient_used == res.gradient_used
        for r in ([None] if rows is None else rows):
            if r is not None:
                lock.set_params(r)
                res.set_params(r)
            lock.init(x0)
            res.init(x0)
            assert_same_state(state(lock), state(res), "init")
            for k in steps:
                lock.step(k)
                res.step(k)
                assert_same_state(state(lock), state(res), f"step({k})")
            xl, sl = lock.minimize(x0.copy())
            xr, sr = res.minimize(x0.copy())
            assert same(xl, xr) and status(sl) == status(sr)
            assert max(s.iteration for s in sl) >= 2
            assert_same_state(state(lock), state(res), "after minimize")
    return res.gradient_used


@pytest.mark.parametrize("ref", [False, True])
def test_custom_objective_with_finite_differences(mod, ref):
    obj = mod.CustomObjective(ROSEN_TERM, chain=True)
    assert custom_case(mod, obj, 5, ref, rosen_starts(5, 5), resident_first=ref) == "finite_difference"


@pytest.mark.parametrize("ref", [False, True])
def test_custom_objective_with_its_gradient_body(mod, ref):
    obj = mod.CustomObjective(ROSEN_TERM, chain=True, grad_body=ROSEN_GRAD)
    assert custom_case(mod, obj, 16, ref, rosen_starts(16, 5), resident_first=not ref) == "analytic"


def test_whole_vector_body(mod):
    obj = mod.CustomObjective("return x.sum([](double xi, uint64_t i) { double r = xi - 0.25 * (double)(i % 3);"
                              " return r * r * r * r + r * r; });", vector=True)
    custom_case(mod, obj, 7, False, starts(7, 5))


def params_case(mod, ref=False):
    """a coefficient as p(0): a different row per problem, the rows replaced once without a rebuild"""
    obj = mod.CustomObjective("double q = xi * xi; return 0.5 * (q * q - p(0) * q + 5.0 * xi);", n_params=1)
    rows = [np.array([[16.0 + b] for b in range(5)]), np.array([[9.0 - b] for b in range(5)])]
    custom_case(mod, obj, 6, ref, starts(6, 5), rows=rows)


def test_a_coefficient_as_a_parameter_row_per_problem(mod):
    params_case(mod)


def test_the_largest_lds_need_4096_parameters_at_64_coordinates(mod):
    """reference order, n = 64, n_params = 4096: 8 KiB of buffers and vectors, the 32 KiB row, 64 rows of 65"""
    assert mod.BFGSEngine.lds_bytes(64, True, 4096, resident=True) > 64 * 1024
    obj = mod.CustomObjective("double r = xi - p(4095); return p(0) * r * r + p(2047) * r * r * r * r;",
                              n_params=4096)
    rows = np.zeros((3, 4096))
    for b in range(3):
        rows[b, 0], rows[b, 2047], rows[b, 4095] = 1.0 + b, 0.5, 0.25 * b
    custom_case(mod, obj, 64, True, starts(64, 3), rows=[rows], steps=(1, 2))


# ---- 7: reuse ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [False, True])
def test_second_solve_equals_a_fresh_engines(mod, ref):
    n = 33
    obj, kw = objective(mod, "quad", n)
    xa, xb = spread_starts(n, 5), starts(n, 5)[::-1].copy()
    with mod.BFGSEngine(obj, 5, reference_order=ref, resident=True, **kw) as used, \
            mod.BFGSEngine(obj, 5, reference_order=ref, resident=True, **kw) as fresh:
        _, sa = used.minimize(xa.copy())
        assert all(s.done for s in sa)
        x1, s1 = used.minimize(xb.copy())
        x2, s2 = fresh.minimize(xb.copy())
        assert same(x1, x2) and status(s1) == status(s2)
        assert_same_state(state(used), state(fresh), "B after A against B alone")
        used.init(xb)                                # and turn by turn: stale done flags, H and dir are A's
        fresh.init(xb)
        used.step(2)
        fresh.step(2)
        assert_same_state(state(used), state(fresh), "two turns of B")


# ---- 8: poisoned pool --------------------------------------------------------------------------------------
PATTERNS = {"1": 0xFF, "0xC0": 0xC0}
CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
from nlsolver_amd import _capi
assert _capi.lib().nlsg_pool_poison() == %(byte)d, ("poison byte in force", _capi.lib().nlsg_pool_poison())
import nlsolver_amd
from tests import test_bfgs_resident_gpu as T
T.poisoned_cases(nlsolver_amd)
print("poison-ok %(byte)d")
"""


def poisoned_cases(mod):
    for n in (3, 64):
        for ref in (False, True):
            turns_case(mod, "quad", n, ref)
    turns_case(mod, "rosenbrock", 3, True)
    params_case(mod, ref=False)
    params_case(mod, ref=True)


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_on_poisoned_blocks(pattern):
    byte = PATTERNS[pattern]
    env = dict(os.environ, NLSG_POOL_POISON=pattern)
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, byte=byte)], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and f"poison-ok {byte}" in r.stdout, r.stderr[-3000:]


# ---- 9: drop-ins -------------------------------------------------------------------------------------------
def drop_in(mod, f, x0, driver, **kw):
    solver = mod.BFGS(f, driver=driver, **kw)
    x = x0.copy()
    st = solver.minimize(x)
    return x, status([st] if x.ndim == 1 else st), solver.driver_used


@pytest.mark.parametrize("name", ["quad", "rosenbrock"])
def test_drop_in_driver_resident_equals_turns(mod, name):
    for n, want in ((8, "resident"), (64, "resident"), (65, "turns")):
        f, _ = objective(mod, name, n)
        for x0 in (starts(n, 1)[0], starts(n, 4)):
            kw = dict(max_iter=12) if name == "rosenbrock" else {}
            xt, st, used_t = drop_in(mod, f, x0, "turns", **kw)
            xr, sr, used_r = drop_in(mod, f, x0, "resident", **kw)
            assert (used_t, used_r) == ("turns", want), n
            assert same(xt, xr) and st == sr, n
    f, _ = objective(mod, "quad", 8)
    assert drop_in(mod, f, starts(8, 2), "resident", symmetric=True)[2] == "turns"
    with pytest.raises(ValueError):
        mod.BFGS(f, driver="resdient")


def test_header_driver_resident_equals_turns_and_the_python_drop_in(mod, tmp_path):
    from nlsolver_amd import _capi
    exe = str(tmp_path / "header_bfgs_resident")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_bfgs_resident.cpp"), "-o", exe, "-ldl"])
    D = 16
    x0 = rosen_starts(D, 1)[0]
    argv = [float(v).hex() for v in x0]
    env = dict(os.environ, NLSG_LIBRARY=_capi.LIB_PATH)
    env.pop("NLSG_SUMMATION", None)   # (the header's default order is the drop-in's: reference)

    def run(driver, *args):
        e = dict(env, NLSG_BFGS_DRIVER=driver)
        return json.loads(subprocess.check_output([exe] + list(args), env=e, text=True, timeout=300))

    def check(got, x, st, what):
        assert same([float.fromhex(v) for v in got["x"]], x), what
        assert bits(float.fromhex(got["f"]))[0] == bits(st.f_value)[0], what
        assert (got["iters"], got["fcalls"], got["gcalls"]) == \
            (st.iteration, st.function_calls_used, st.gradient_evals_used), what

    for mode, grad in (("analytic", ROSEN_GRAD),):     # (the default gradient: the batch form below)
        solver = mod.BFGS(mod.CustomObjective(ROSEN_TERM, chain=True, grad_body=grad), driver="resident")
        x = x0.copy()
        st = solver.minimize(x)
        assert solver.driver_used == "resident" and st.iteration >= 1
        got = {d: run(d, mode, *argv) for d in ("resident", "turns")}
        assert got["resident"] == got["turns"], mode
        check(got["resident"], x, st, mode)
    xb = rosen_starts(5, 3)
    solver = mod.BFGS(mod.CustomObjective(ROSEN_TERM, chain=True), driver="resident")
    want = xb.copy()
    stb = solver.minimize(want)
    flat = [float(v).hex() for v in xb.ravel()]
    got = {d: run(d, "batch", "5", *flat) for d in ("resident", "turns")}
    assert got["resident"] == got["turns"] and len(got["resident"]) == 3
    for b in range(3):
        check(got["resident"][b], want[b], stb[b], b)
    r = subprocess.run([exe, "default"] + argv, env=dict(env, NLSG_BFGS_DRIVER="resdient"), text=True,
                       capture_output=True, timeout=300)
    assert r.returncode == 3 and "NLSG_BFGS_DRIVER" in r.stderr and "resdient" in r.stderr
