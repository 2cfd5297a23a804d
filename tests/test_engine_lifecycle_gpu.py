"""What an engine takes from the device pool it gives back, on every path (nlsolver_amd/csrc/
nlsg_engine.h): the bytes parked after a create / destroy cycle, after a create that fails in the
run-time compiler, and after NM's lazily allocated phase buffer, and the "parameters not set"
texts, all compared with tests/golden/engine_cached_bytes.json (scripts/
record_engine_cached_bytes.py wrote it on the commit before the engines shared one owner)."""
import pytest

from tests import _engine_lifecycle as L

pytestmark = pytest.mark.gpu

GOLD = L.golden()


@pytest.fixture(scope="module")
def lib():
    from nlsolver_amd import _capi
    lib = _capi.lib()
    yield lib
    lib.nlsg_release_cached()


@pytest.mark.parametrize("name", sorted(L.ENGINES))
def test_create_destroy_cycle_parks_the_recorded_bytes(lib, name):
    L.emptied(lib)
    assert L.cycle(lib, name) == GOLD["cycle"][name]
    # every block recycled: none leaked, none parked twice
    assert L.cycle(lib, name) == GOLD["cycle"][name]


@pytest.mark.parametrize("name", sorted(L.RTC_FAILURES))
def test_create_that_fails_after_its_allocations(lib, name):
    L.emptied(lib)
    code, parked = L.failed_create(lib, name)
    assert "does not compile" in L.last_error(lib)
    assert code == GOLD["rtc_failure"][name]["code"]
    assert parked == GOLD["rtc_failure"][name]["bytes"]
    good = L.RTC_FAILURES[name][3]
    L.emptied(lib)
    assert L.cycle(lib, good) == GOLD["cycle"][good]


def test_nm_phase_buffer_goes_back_with_the_engine(lib):
    L.emptied(lib)
    assert L.nm_phase_cycle(lib) == GOLD["nm_phase"]
    assert L.nm_phase_cycle(lib) == GOLD["nm_phase"]


def test_tinyqr_calls_park_the_recorded_bytes(lib):
    L.emptied(lib)
    assert list(L.tinyqr_calls(lib)) == [GOLD["tinyqr_lm"], GOLD["tinyqr_qr"]]


@pytest.mark.parametrize("kind", sorted(L.PARAM_KINDS))
def test_parameter_messages(lib, kind):
    assert L.param_messages(lib, kind) == GOLD["messages"][kind]
