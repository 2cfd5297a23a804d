"""Reference-order DE, the parts that need no GPU: the pure-Python XorShift, the M^64 jump table
the engine advances its lanes with, the donor pick's guard rails, and every refusal that must come
before the device is touched (pop < 4, Rastrigin, a whole-vector body, an unknown
NLSG_DE_GENERATION)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nlsolver_amd
from nlsolver_amd import de as nde
from tests import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nlsolver_amd", "libnlsolver_hip.so")


def test_xorshift_default_stream_matches_reference(golden):
    g = golden("rng.json")
    xs = nlsolver_amd.XorShift()
    assert [xs() for _ in g["xorshift_double"]] == [float.fromhex(v) for v in g["xorshift_double"]]


def test_xorshift_matches_oracle_from_random_states(oracle):
    rs = np.random.default_rng(7)
    for _ in range(10):
        s0, s1 = (int(v) for v in rs.integers(0, 2**64, size=2, dtype=np.uint64))
        py = nlsolver_amd.XorShift((s0, s1))
        ref = O.XorShift()
        ref.x[0], ref.x[1] = s0, s1
        got = [py() for _ in range(10_000)]
        want = [oracle.orc_xorshift_next(C.byref(ref)) for _ in range(10_000)]
        assert got == want
        assert py.state == (ref.x[0], ref.x[1])


def test_xorshift_state_roundtrip():
    a = nlsolver_amd.XorShift()
    a()
    b = nlsolver_amd.XorShift(a.state)
    assert [a() for _ in range(5)] == [b() for _ in range(5)]
    b.state = (2**64 - 1, 0)
    assert b.state == (2**64 - 1, 0)


def _apply_table(t, s0, s1):
    r0 = r1 = 0
    for j in range(16):
        e = t[j, (s0 >> (4 * j)) & 15]
        r0 ^= int(e[0])
        r1 ^= int(e[1])
    for j in range(16):
        e = t[16 + j, (s1 >> (4 * j)) & 15]
        r0 ^= int(e[0])
        r1 ^= int(e[1])
    return r0, r1


def test_jump_table_is_64_steps(oracle):
    t = nde.jump_table()
    assert t.shape == (32, 16, 2) and not t[:, 0].any()  # the zero nibble maps to 0
    rs = np.random.default_rng(11)
    for _ in range(1000):
        s0, s1 = (int(v) for v in rs.integers(0, 2**64, size=2, dtype=np.uint64))
        ref = O.XorShift()
        ref.x[0], ref.x[1] = s0, s1
        for _ in range(64):
            oracle.orc_xorshift_next(C.byref(ref))
        assert _apply_table(t, s0, s1) == (ref.x[0], ref.x[1])


def test_donor_pick_matches_oracle(oracle):
    fn = oracle.orc_de_serial_proposal_from_draws
    fn.restype = C.c_size_t
    fn.argtypes = [O.pd, O.sz, O.sz, O.sz, O.f64, O.f64, O.pd, O.sz, O.pd, O.pu, O.pu, O.pd]
    rs = np.random.default_rng(3)
    for pop in (4, 5, 9, 40):
        agents = np.zeros((pop, 2))
        for fixed in range(pop):
            draws = rs.random(64)
            ids, used, flag = nde.pick_donors(draws, fixed, pop)
            want, wused = np.zeros(4, dtype=np.uint64), C.c_size_t()
            prop = np.zeros(2)
            fn(agents.ctypes.data_as(O.pd), pop, 2, fixed, 0.5, 0.5, draws.ctypes.data_as(O.pd), 64,
               np.zeros(3).ctypes.data_as(O.pd), want.ctypes.data_as(O.pu), C.byref(wused),
               prop.ctypes.data_as(O.pd))
            assert flag == 0 and ids == [int(v) for v in want] and used == wused.value


def test_donor_pick_flags_a_draw_of_one():
    # generate_index(pop) of a draw of exactly 1.0 is pop: the reference would read row pop
    ids, used, flag = nde.pick_donors([0.3, 1.0, 0.6, 0.9], 0, 4)
    assert flag == 1 and used == 2
    # ... also where it would be the first donor, and under any pop
    assert nde.pick_donors([1.0], 7, 50)[2] == 1
    # a draw just below 1.0 is an index like any other
    below = float(np.nextafter(1.0, 0.0))
    assert nde.pick_donors([below, 0.3, 0.6], 0, 4) == ([0, 3, 1, 2], 3, 0)


def test_donor_pick_rejection_cap():
    # a degenerate stream (the all-zero xorshift state draws 0.0 forever): index 0 again and again
    n = 2**20 + 8
    ids, used, flag = nde.pick_donors(np.zeros(n), 1, 4)
    assert flag == 2 and used == 2**20 and ids[:2] == [1, 0]


@pytest.mark.parametrize("kw, code", [
    (dict(objective="rosenbrock", pop=3), 1),
    (dict(objective="rosenbrock", pop=0), 1),
    (dict(objective="rastrigin", pop=40), 2),
])
def test_refused_before_the_device(kw, code):
    with pytest.raises(nlsolver_amd.NlsgError) as ei:
        nlsolver_amd.DERefEngine(kw["objective"], 1, kw["pop"], 2)
    assert ei.value.code == code
    assert ("pop" in str(ei.value)) if code == 1 else ("Rastrigin" in str(ei.value))


def test_whole_vector_body_refused_before_the_device():
    obj = nlsolver_amd.CustomObjective("return x(0) * x(0);", vector=True)
    with pytest.raises(nlsolver_amd.NlsgError) as ei:
        nlsolver_amd.DERefEngine(obj, 1, 40, 2)
    assert ei.value.code == 2 and "whole-vector" in str(ei.value)


def test_python_de_reference_needs_xorshift():
    with pytest.raises(TypeError):
        nlsolver_amd.DE("rosenbrock", None, generation="reference")
    with pytest.raises(ValueError):
        nlsolver_amd.DE("rosenbrock", nlsolver_amd.XorShift(), generation="sync")


@pytest.fixture(scope="module")
def header_prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("de_ref") / "header_de_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "header_de_ref.cpp"), "-o", out, "-ldl"])
    return out


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k != "NLSG_DE_GENERATION"}
    env["NLSG_LIBRARY"] = LIB
    env.update(kw)
    return env


def test_header_generation_selector(header_prog):
    run = lambda **kw: subprocess.run([header_prog, "mode"], env=_env(**kw), capture_output=True, text=True)
    assert run().stdout.strip() == "keyed"  # default: the keyed engine
    assert run(NLSG_DE_GENERATION="keyed").stdout.strip() == "keyed"
    assert run(NLSG_DE_GENERATION="reference").stdout.strip() == "reference"
    r = run(NLSG_DE_GENERATION="refrence")
    assert r.returncode == 3 and "NLSG_DE_GENERATION must be keyed or reference" in r.stdout


@pytest.mark.parametrize("case, why", [("reject-rng", "rng::xorshift<double>"),
                                       ("reject-rastrigin", "Rastrigin"),
                                       ("reject-vector", "whole-vector")])
def test_header_reference_mode_refusals(header_prog, case, why):
    # thrown before the library or a device is asked for anything: no GPU needed
    r = subprocess.run([header_prog, case], env=_env(NLSG_DE_GENERATION="reference",
                                                     NLSG_LIBRARY="/nonexistent/lib.so"),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("device_error:") and why in r.stdout


def test_capi_declares_reference_order_de():
    with open(os.path.join(ROOT, "include", "nlsg_c_api.h")) as fh:
        h = fh.read()
    for name in ("nlsg_de_ref_create", "nlsg_de_ref_create_custom", "nlsg_de_ref_destroy",
                 "nlsg_de_ref_minimize", "nlsg_de_ref_log", "nlsg_de_ref_time_solve"):
        assert name + "(" in h
    assert "#define NLSG_ABI_VERSION 1" in h
