"""Every call the engines reject before a device is touched — each create door with one thing wrong,
every handle-taking entry point on a null handle, the handle-less tinyqr entries — returns the code
and says the text recorded in tests/golden/engine_doors.json (scripts/record_engine_doors.py, at the
commit named in the file), and the pure size functions return the recorded values. The table is
tests/_engine_doors.py; no expectation is computed from the library under test."""
from nlsolver_amd import _capi
from tests import _engine_doors as D
from tests import _engine_lifecycle as L

# exported functions with a handle parameter that no rejected-call case can cover (none today)
NOT_NULL_CHECKED = ()


def test_case_list_is_the_recorded_one():
    gold = D.golden()
    ids = [cid for cid, _ in D.cases()]
    assert len(set(ids)) == len(ids)
    assert sorted(ids) == sorted(gold["cases"])
    assert sorted(cid for cid, _ in D.pure()) == sorted(gold["pure"])
    assert len(gold["commit"]) == 40


def test_every_rejected_call_answers_as_recorded():
    lib = _capi.lib()
    gold = D.golden()["cases"]
    wrong = []
    for cid, call in D.cases():
        got = list(call(lib))
        if got != gold[cid]:
            wrong.append((cid, got, gold[cid]))
    assert not wrong, "\n".join(f"{cid}: {got} != recorded {want}" for cid, got, want in wrong)


def test_no_case_is_a_success_but_a_destroy_or_a_query():
    """a table entry that returned NLSG_OK would pin nothing: only destroy(NULL) and the value-returning
    queries (record_doubles, can_speculate) may answer 0"""
    for cid, (code, text) in D.golden()["cases"].items():
        if code == 0:
            assert cid.startswith("null_handle/") and cid.split("/")[1].endswith(
                ("_destroy", "_record_doubles", "_can_speculate")), cid
        else:
            assert text, cid


def test_pure_functions_at_their_boundaries():
    lib = _capi.lib()
    gold = D.golden()["pure"]
    wrong = [(cid, call(lib), gold[cid]) for cid, call in D.pure() if call(lib) != gold[cid]]
    assert not wrong, wrong


def test_every_handle_entry_point_has_a_null_handle_case():
    names = D.handle_symbols()
    assert len(names) >= 90 and "nlsg_de_step" in names and "nlsg_pso_batch_time_solve" in names
    recorded = D.golden()["cases"]
    for name in names:
        if name in NOT_NULL_CHECKED:
            continue
        assert f"null_handle/{name}" in recorded, f"{name} takes a handle and has no null-handle case"
    # and the scan misses no exported function whose ctypes signature starts with a handle
    by_signature = sorted(n for n, (_, args) in _capi.SYMBOLS.items()
                          if args and args[0] is _capi._H and n not in ("nlsg_host_free", "nlsg_tinyqr_lm_device"))  # (plain pointers)
    assert by_signature == names


def test_doors_build_on_the_lifecycle_configs():
    # one config per kind, the lifecycle file's: the two tables cannot drift apart
    for kind, doors in D.DOORS.items():
        cfg = doors["plain"].cfg()
        assert type(cfg) is type(L.ENGINES[kind][2]), kind
