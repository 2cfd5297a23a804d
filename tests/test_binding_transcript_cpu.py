"""The Python binding makes the C calls it made before the engine classes shared one base: every case of
tests/_binding_transcript.py replayed on a fake library and compared, entry by entry, with
tests/golden/binding_transcript.json.gz (scripts/record_binding_transcript.py wrote it on the commit the
file names, the one before nlsolver_amd/_engine.py existed). Needs neither a device nor the library."""
import gzip
import inspect
import json
import os

import pytest

import nlsolver_amd
from nlsolver_amd import _capi
from tests import _binding_transcript as T

with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_transcript.json.gz"),
               "rt") as _f:
    GOLD = json.load(_f)
CASES = {c.id: c for c in T.cases()}

# entry points no engine class reaches: the process-wide ones, the host allocator, the communicator's
# set-up (dist.py), the device-resident tinyqr entry and the pure rule helpers the tests call directly
NOT_ENGINE_CALLS = ["nlsg_abi_version", "nlsg_device_count", "nlsg_call_timing", "nlsg_release_cached",
                    "nlsg_cached_bytes", "nlsg_pool_poison", "nlsg_comm_load", "nlsg_comm_unique_id",
                    "nlsg_host_alloc", "nlsg_host_free", "nlsg_tinyqr_lm_device", "nlsg_de_bound_gate",
                    "nlsg_de_screen_gate", "nlsg_de_screen_env", "nlsg_de_screen_rule"]


def _replay(monkeypatch, case):
    fake = T.FakeLibrary(case.missing, case.fail)
    monkeypatch.setattr(_capi, "_lib", fake)
    return json.loads(json.dumps(T.record(case, fake)))  # (tuples -> lists, as the file has them)


def test_the_case_list_is_the_recorded_one():
    assert sorted(CASES) == sorted(GOLD["cases"])


@pytest.mark.parametrize("id", sorted(GOLD["cases"]))
def test_case_makes_the_recorded_calls(monkeypatch, id):
    got, want = _replay(monkeypatch, CASES[id]), GOLD["cases"][id]
    assert got["error"] == want["error"]
    assert len(got["calls"]) == len(want["calls"]), [c[0] for c in got["calls"]]
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {k}"
    assert got["result"] == want["result"]
    assert got["unraisable"] == want["unraisable"] == []


@pytest.mark.parametrize("id", sorted(i for i in CASES if i.startswith("missing:")))
def test_missing_entry_point_is_code_2_before_any_call(monkeypatch, id):
    got = _replay(monkeypatch, CASES[id])
    assert got["error"]["type"] == "NlsgError" and got["error"]["code"] == _capi.NLSG_ERR_UNSUPPORTED
    assert got["error"]["text"] == GOLD["cases"][id]["error"]["text"]
    assert got["calls"] == [] and got["unraisable"] == []


@pytest.mark.parametrize("id", sorted(i for i in CASES if ":fails:" in i))
def test_failed_create_leaves_nothing_to_destroy(monkeypatch, id):
    got = _replay(monkeypatch, CASES[id])
    assert got["error"]["type"] == "NlsgError" and got["error"]["code"] == 2
    assert got["unraisable"] == []
    destroys = [c[0] for c in got["calls"] if c[0].endswith("_destroy")]
    # a create that fails hands no handle over; set_data failing after a create leaves one, closed once
    assert len(destroys) == (0 if "_create" in id.split(":fails:")[1] else 1)


@pytest.mark.parametrize("symbol", sorted(_capi.OPTIONAL_SYMBOLS))
def test_require_message(monkeypatch, symbol):
    got = _replay(monkeypatch, CASES[f"require:{symbol}"])
    assert got["error"] == GOLD["cases"][f"require:{symbol}"]["error"] and got["error"]["code"] == 2


def test_cases_reach_every_entry_point():
    reached = {c[0] for case in GOLD["cases"].values() for c in case["calls"]}
    assert set(_capi.SYMBOLS) - reached == set(NOT_ENGINE_CALLS)
    source = "".join(inspect.getsource(c) for cls in T.ENGINE_CLASSES for c in getattr(nlsolver_amd, cls).__mro__[:-1])
    for name in NOT_ENGINE_CALLS:
        assert name not in source, f"{name} has an engine-class caller: the case list is short"


def test_public_surface_is_kept():
    now = T.surface()
    for cls, sigs in GOLD["surface"]["classes"].items():
        for name, sig in sigs.items():
            assert now["classes"][cls].get(name) == sig, f"{cls}.{name}"
    for module, names in GOLD["surface"]["modules"].items():
        assert set(names) <= set(now["modules"][module]), (module, sorted(set(names) - set(now["modules"][module])))
    assert set(GOLD["surface"]["package"]) <= set(now["package"])
