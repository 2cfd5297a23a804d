"""What include/nlsolver_mi/nlsolver.h and tinyqr.h ask of libnlsolver_hip.so, pinned without a GPU.

tests/cpp/header_calls.cpp takes every device branch of the headers against a stand-in library
(tests/cpp/stub_nlsg.cpp: the headers' entry points with the prototypes of nlsg_c_api.h, no HIP) that
logs each call with its arguments and answers deterministically. For every case below the call log,
what the class printed, the exit status and the exception text must equal
tests/golden/header_calls/<case>.txt, and no engine may be left undestroyed.

The golden files were recorded from the header as it stood before its device paths were moved onto
shared helpers, so they hold the order of calls and every config byte of that header. To record a
new case:  python -m tests.test_header_calls_cpu CASE...  (or `all`)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "header_calls")
ENV_NAMES = ("NLSG_LIBRARY", "NLSG_STUB_LOG", "NLSG_STUB_FAIL", "NLSG_DEVICE", "NLSG_HIPRTC", "NLSG_SUMMATION",
             "NLSG_DE_GENERATION", "NLSG_DE_DRIVER", "NLSG_PSO_DRIVER", "NLSG_BFGS_DRIVER")

CASES = {}


def case(arg, tag="", old=False, fail=None, **env):
    """`arg` is the driver's case; `tag` names the environment it runs in; old: the library without
    the optional entry points; fail: the symbol that answers an error."""
    if fail:
        env["NLSG_STUB_FAIL"] = fail
        tag = tag + ("+" if tag else "") + "fail_" + fail[len("nlsg_"):]
    if old:
        tag = tag + ("+" if tag else "") + "old"
    name = arg.replace(":", "-") + ("@" + tag if tag else "")
    assert name not in CASES, name
    CASES[name] = (arg, old, env)


RESIDENT_DE = dict(tag="resident", NLSG_DE_DRIVER="resident")
REFERENCE_DE = dict(tag="reference", NLSG_DE_GENERATION="reference")
RESIDENT_PSO = dict(tag="resident", NLSG_PSO_DRIVER="resident")
RESIDENT_BFGS = dict(tag="resident", NLSG_BFGS_DRIVER="resident")
TREE = dict(tag="tree", NLSG_SUMMATION="tree")

# DE: built-in, Custom, Custom with params; turns, resident, reference generation; both strategies and senses
DE = ["de:rosenbrock:random:min", "de:rosenbrock:best:max", "de:custom:random:min", "de:custom:best:max",
      "de:params:random:min", "de:params:best:max"]
for a in DE:
    case(a)
    case(a, **RESIDENT_DE)
    case(a, **REFERENCE_DE)
case("de:rosenbrock:random:min:big", **RESIDENT_DE)  # does not fit the resident engine: the turn engine
case("de:params:random:min:big")                     # parameters that do not fit: an error
case("de:rastrigin:random:min", **REFERENCE_DE)      # refused before any call
case("de:vector:random:min", **REFERENCE_DE)
case("de:custom:random:min", tag="device3", NLSG_DEVICE="3", NLSG_HIPRTC="/opt/somewhere/libhiprtc.so")

# PSO: turns and resident, free and bounded, both types
PSO = ["pso:rosenbrock:vanilla:free:min", "pso:rosenbrock:accel:bounded:max", "pso:custom:accel:free:min",
       "pso:custom:vanilla:bounded:max", "pso:params:vanilla:free:min", "pso:params:accel:bounded:max"]
for a in PSO:
    case(a)
    case(a, **RESIDENT_PSO)
case("pso:rosenbrock:vanilla:free:min:big", **RESIDENT_PSO)
case("pso:params:accel:free:min:big")

# NelderMead: free and bounded, built-in and Custom, with and without params, both summation orders
for a in ["nm:rosenbrock:free:min", "nm:rosenbrock:bounded:max", "nm:rastrigin:free:min", "nm:custom:free:min",
          "nm:custom:bounded:min", "nm:vector:free:min", "nm:params:free:min", "nm:params:bounded:max"]:
    case(a)
    case(a, **TREE)

# BFGS
for kind in ["quad", "rosenbrock", "custom", "params", "grad", "gradparams"]:
    case(f"bfgs:{kind}:one")
    case(f"bfgs:{kind}:batch")
    case(f"bfgs:{kind}:one", **TREE)
case("bfgs:gradempty:one")  # throws before any call
for a in ["bfgs:quad:one", "bfgs:rosenbrock:batch", "bfgs:custom:one", "bfgs:params:batch", "bfgs:grad:one",
          "bfgs:quad:one:n65", "bfgs:rosenbrock:batch:n65"]:
    case(a, **RESIDENT_BFGS)

# LevenbergMarquardt: B = 1 (lambda written back), B = 2, B != problems()
for kind in ["tanh", "link", "curve", "rosenbrock", "custom", "params"]:
    case(f"lm:{kind}:one")
    case(f"lm:{kind}:batch")
case("lm:tanh:mismatch")
case("lm:vector:one")
for a in ["lm:rosenbrock:one", "lm:custom:one", "lm:tanh:one"]:
    case(a, **TREE)

# SANN and NelderMeadPSO
for a in ["sann:rosenbrock:one:min", "sann:rosenbrock:batch:max", "sann:custom:one:max", "sann:custom:batch:min",
          "sann:params:one:min", "sann:params:batch:min",
          "nmpso:rosenbrock:one:min", "nmpso:rosenbrock:bounded:max", "nmpso:rosenbrock:batch:min",
          "nmpso:custom:one:max", "nmpso:custom:bounded:min", "nmpso:custom:batch:min",
          "nmpso:params:one:min", "nmpso:params:bounded:max", "nmpso:params:batch:min"]:
    case(a)

case("tinyqr")

# failures: every set_params; minimize once per class and engine; create; rtc_load; the data uploads
for a in ["de:params:random:min", "de:params:best:max"]:
    case(a, fail="nlsg_de_batch_set_params")
    case(a, fail="nlsg_de_batch_set_params", **RESIDENT_DE)
for a in ["pso:params:vanilla:free:min", "pso:params:accel:bounded:max"]:
    case(a, fail="nlsg_pso_batch_set_params")
    case(a, fail="nlsg_pso_batch_set_params", **RESIDENT_PSO)
for a in ["nm:params:free:min", "nm:params:bounded:max"]:
    case(a, fail="nlsg_nm_set_params")
    case(a, fail="nlsg_nm_set_params", **TREE)
for a in ["nmpso:params:one:min", "nmpso:params:bounded:max", "nmpso:params:batch:min"]:
    case(a, fail="nlsg_nmpso_set_params")
for kind in ["params", "gradparams"]:
    case(f"bfgs:{kind}:one", fail="nlsg_bfgs_set_params")
    case(f"bfgs:{kind}:batch", fail="nlsg_bfgs_set_params")
    case(f"bfgs:{kind}:one", fail="nlsg_bfgs_set_params", **TREE)
case("bfgs:params:batch", fail="nlsg_bfgs_set_params", **RESIDENT_BFGS)
case("lm:params:one", fail="nlsg_lm_set_params")
case("lm:params:batch", fail="nlsg_lm_set_params")
case("de:rosenbrock:random:min", fail="nlsg_de_minimize")
case("de:custom:random:min", fail="nlsg_de_batch_minimize", **RESIDENT_DE)
case("de:rosenbrock:best:max", fail="nlsg_de_ref_minimize", **REFERENCE_DE)
case("pso:custom:accel:free:min", fail="nlsg_pso_minimize")
case("pso:rosenbrock:vanilla:free:min", fail="nlsg_pso_batch_minimize", **RESIDENT_PSO)
case("nm:custom:bounded:min", fail="nlsg_nm_minimize")
case("bfgs:quad:batch", fail="nlsg_bfgs_minimize")
case("lm:tanh:one", fail="nlsg_lm_minimize")
case("lm:tanh:one", fail="nlsg_lm_set_data")
case("lm:curve:batch", fail="nlsg_lm_set_curve_data")
case("sann:custom:batch:min", fail="nlsg_sann_minimize")
case("nmpso:rosenbrock:one:min", fail="nlsg_nmpso_minimize")
case("tinyqr", fail="nlsg_tinyqr_lm")
case("de:rosenbrock:random:min", fail="nlsg_de_create")
case("de:custom:best:max", fail="nlsg_de_ref_create_custom", **REFERENCE_DE)
case("pso:params:vanilla:free:min", fail="nlsg_pso_batch_create_custom")
case("nm:params:free:min", fail="nlsg_nm_create_params")
case("bfgs:params:one", fail="nlsg_bfgs_create_params")
case("bfgs:grad:one", fail="nlsg_bfgs_create_gradient")
case("lm:link:one", fail="nlsg_lm_create_link")
case("sann:rosenbrock:one:min", fail="nlsg_sann_create")
case("nmpso:custom:one:max", fail="nlsg_nmpso_create_custom")
case("de:custom:random:min", fail="nlsg_rtc_load")
case("lm:curve:one", fail="nlsg_rtc_load")
case("bfgs:grad:one", fail="nlsg_rtc_load")

# a library that predates the optional entry points
for a in ["de:params:random:min", "pso:params:vanilla:free:min", "nm:params:free:min", "nmpso:params:one:min",
          "sann:params:one:min", "bfgs:params:one", "lm:params:one", "lm:link:one", "lm:curve:one", "bfgs:grad:one",
          "bfgs:gradparams:one", "de:custom:random:min", "nm:custom:free:min"]:
    case(a, old=True)
case("de:rosenbrock:random:min", old=True, **RESIDENT_DE)
case("de:rosenbrock:random:min", old=True, **REFERENCE_DE)
case("pso:rosenbrock:vanilla:free:min", old=True, **RESIDENT_PSO)
case("bfgs:quad:one", old=True, **RESIDENT_BFGS)

# an allocation that throws between create and minimize: the engine is destroyed all the same
for a in ["bfgs:rosenbrock:alloc", "lm:tanh:alloc", "sann:custom:alloc", "nmpso:params:alloc"]:
    case(a)

# a misspelt mode is an error, by name
case("nm:rosenbrock:free:min", tag="summation_automatic", NLSG_SUMMATION="automatic")
case("de:rosenbrock:random:min", tag="generation_refrence", NLSG_DE_GENERATION="refrence")
case("de:rosenbrock:random:min", tag="driver_resdent", NLSG_DE_DRIVER="resdent")
case("pso:rosenbrock:vanilla:free:min", tag="driver_resdent", NLSG_PSO_DRIVER="resdent")
case("bfgs:quad:one", tag="driver_resdent", NLSG_BFGS_DRIVER="resdent")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp")])
    return BIN


def run_case(name, log_path):
    arg, old, extra = CASES[name]
    env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    env.update(extra, NLSG_STUB_LOG=log_path,
               NLSG_LIBRARY=os.path.join(BIN, "libnlsg_stub_old.so" if old else "libnlsg_stub.so"))
    if os.path.exists(log_path):
        os.remove(log_path)
    r = subprocess.run([os.path.join(BIN, "header_calls"), arg], env=env, capture_output=True, text=True)
    calls = open(log_path).read() if os.path.exists(log_path) else ""
    return f"exit {r.returncode}\n-- printed\n{r.stdout}-- stderr\n{r.stderr}-- calls\n{calls}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_calls_match_the_recorded_ones(built, tmp_path, name):
    got = run_case(name, str(tmp_path / "calls.log"))
    with open(os.path.join(GOLDEN, name + ".txt")) as fh:
        assert got == fh.read()
    # (a case that fails before the library is loaded has no log at all)
    assert got.endswith("-- calls\n") or got.endswith("\nlive_engines 0\n"), got


def test_every_golden_file_is_a_case():
    assert sorted(f[:-4] for f in os.listdir(GOLDEN)) == sorted(CASES)


if __name__ == "__main__":
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp")])
    os.makedirs(GOLDEN, exist_ok=True)
    for name in (sorted(CASES) if sys.argv[1:] == ["all"] else sys.argv[1:]):
        with open(os.path.join(GOLDEN, name + ".txt"), "w") as fh:
            fh.write(run_case(name, os.path.join(BIN, "calls.log")))
