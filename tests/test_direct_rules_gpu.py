"""The decision rules of the three direct-search solvers on the device (nm_solve_kernel,
nm_solve_driver_kernel; the hybrid's rank sort and its no-change rule; SANN's acceptance test in its
three layouts) against the independent Python references of tests/_direct_ref.py, on hostile user
objectives given as source text (tests/_hostile.py): plateaus (ties everywhere), constant 0, NaN
regions, all NaN, +-inf walls, huge steps that overflow std_err, signed zeros. The case list is
tests/_direct_cases.py; tests/test_direct_rules_cpu.py holds the references to the oracle, to the
reference's own runs and to the unmodified reference on the same hostile families, and asserts
that this case list reaches every action, scan category, SANN outcome and sort condition in every
kernel class.

Compared per start: x bit for bit (NaN equal to NaN), f_value by value (a sum that starts from +0.0
and a lane tree padded with +0.0 agree on a signed zero only by value), iteration,
function_calls_used, and Nelder-Mead's mutated eps.

Mutation checks run on an MI355X. Each library was built with that one change to the headers the
run-time compiler embeds (wrong answers only: the `== ~0` guards and `frozen` stayed), and each failed
the named test by comparison with the Python reference; the unchanged library passes every case.
Case names are this module's ids (batch-order-driver); the list has 58 Nelder-Mead, 14 hybrid and 18 SANN cases.
  argmax_combine: an equal value keeps the HIGHER index     test_nelder_mead_follows_the_reference, every
      case that runs nm_solve_kernel and no other: the 18 driver0 cases but n1_min's, n129 / n257 in both
      orders, n129_max_bounded (24 cases; the driver kernel does not call it and passes)
  first_holder takes the highest set bit                    the same test, every driver1 case at n <= 128 (32:
      n1 .. n128 in both orders, bounded, restarts, the literal and the whole-vector body)
  the second-worst pass runs to nv instead of worst_i       the same test, all 58 cases (the B3 quirk)
  `rs >= scores[best]` -> `>`                                the same test, 52 of 58 (all but n1_min, where a
      reflection never equals the best, and the whole-vector batches)
  the sort's `r + u < q` -> `>`                              test_hybrid_follows_the_reference, all 14 batches
  hyb_key(NaN) = 0                                          the same test, the 12 batches with NaN keys (not
      the whole-vector ones, which have none): e.g. n2_min/3 returns x untouched with f = NaN
  SANN `difference <= 0.0` -> `<`                            test_sann_follows_the_reference[D2_zero_t,
      D130_zero_t, D1026_zero_t], one per layout. At every other temperature exp(-0 / t) = 1 accepts an
      equal trial whichever comparison is written: the two rules differ only where t = 0 (or NaN)
  SANN `current_val <= best` -> `<`                          the same test, 16 of 18 (not D16_literal and
      D2_negative_t_finite, which have no equal trial)
  sann_sure_reject without `t > 0.0`                        D130_negative_t and D2_negative_t_finite (in
      D2_negative_t a chain with a NaN difference shares the wave, the ballot is never empty and the
      full test runs for every lane: the shortcut is not consulted there)
"""
import numpy as np
import pytest

from tests import _direct_cases as Cs
from tests import _direct_ref as R
from tests import _hostile as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    return nlsolver_amd


def custom(mod, source):
    if source == "literal":
        return mod.CustomObjective(H.LITERAL_SRC)
    if source == "vector":
        return mod.CustomObjective(H.VECTOR_SRC, vector=True, n_params=H.N_PARAMS)
    return mod.CustomObjective(H.TERM_SRC, n_params=H.N_PARAMS)


def params_of(batch):
    if batch.source == "literal":
        return None
    return np.array([[r.family, r.a, r.b] for r in batch.rows], dtype=np.float64)


def starts_of(batch, n):
    return np.array([Cs.start(r, n) for r in batch.rows], dtype=np.float64)


def compare(tag, x, st, want, bad, eps=None):
    """one start of a batch against its reference Result"""
    if not all(R.same_bits(a, b) for a, b in zip(x, want.x)):
        k = next(i for i, (a, b) in enumerate(zip(x, want.x)) if not R.same_bits(a, b))
        bad.append(f"{tag}: x[{k}] {x[k]!r} != reference {want.x[k]!r}")
    if not R.same_value(st.f_value, want.f_value):
        bad.append(f"{tag}: f_value {st.f_value!r} != reference {want.f_value!r}")
    if (st.iteration, st.function_calls_used) != (want.iteration, want.function_calls_used):
        bad.append(f"{tag}: (iteration, calls) {(st.iteration, st.function_calls_used)} != reference "
                   f"{(want.iteration, want.function_calls_used)}")
    if eps is not None and not R.same_value(eps, want.eps):
        bad.append(f"{tag}: eps {eps!r} != reference {want.eps!r}")


def row_tag(batch, r):
    row = batch.rows[r]
    return f"{batch.name}/{r} {H.FAMILY_NAMES.get(row.family, batch.source)}({row.a}, {row.b}) x0 {row.x0} dx {row.dx}"


# ---- Nelder-Mead ------------------------------------------------------------------------------------
NM = {b.name: b for b in Cs.nm_batches()}


# nm_solve_kernel at n <= 128 with restarts and an explicit step, and bounded while maximising
NM_ALSO_DRIVER0 = ("n16_restarts_step", "n128_restarts_step", "n64_max_bounded")


def nm_modes(batch):
    """(reference_order, NLSG_NM_DRIVER): every size in both orders; n <= 128 also on the
    phase-per-barrier kernel (the main batches and NM_ALSO_DRIVER0; a whole-vector body has no reference order)"""
    orders = (False,) if batch.source == "vector" else (False, True)
    out = [(o, "1") for o in orders]
    if batch.n <= 128 and (batch.name.endswith("_min") or batch.name in NM_ALSO_DRIVER0):
        out += [(o, "0") for o in orders]
    return out


@pytest.mark.parametrize("name,ref_order,driver", [
    pytest.param(b.name, o, d, id=f"{b.name}-{'ref' if o else 'tree'}-driver{d}")
    for b in Cs.nm_batches() for o, d in nm_modes(b)])
def test_nelder_mead_follows_the_reference(mod, golden, monkeypatch, name, ref_order, driver):
    batch = NM[name]
    monkeypatch.setenv("NLSG_NM_DRIVER", driver)
    want = Cs.nm_reference(batch, not ref_order)
    assert mod.NMEngine.fits(batch.n, ref_order, H.N_PARAMS)
    with mod.NMEngine(custom(mod, batch.source), len(batch.rows), batch.n, minimize=batch.minimize,
                      bounded=batch.bounded, step=batch.step, eps=batch.eps, max_iter=batch.max_iter,
                      no_change_best_tol=batch.no_change, restarts=batch.restarts,
                      reference_order=ref_order) as eng:
        x, st, eps = eng.minimize(starts_of(batch, batch.n), batch.upper if batch.bounded else None,
                                  batch.lower if batch.bounded else None, params=params_of(batch))
    bad = []
    for r in range(len(batch.rows)):
        compare(row_tag(batch, r), x[r], st[r], want[r][0], bad, eps=eps[r])
    if ref_order:  # the unmodified reference's own bits, where it ran this start
        runs = golden("nm_hostile.json")["runs"]
        for r in range(len(batch.rows)):
            run = runs.get(f"{batch.name}/{r}")
            if run is None:
                continue
            gx = [float.fromhex(v) for v in run["x"]]
            if not (all(R.same_bits(a, b) for a, b in zip(x[r], gx)) and
                    R.same_value(st[r].f_value, float.fromhex(run["f"])) and
                    (st[r].iteration, st[r].function_calls_used) == (run["iters"], run["fcalls"])):
                bad.append(f"{row_tag(batch, r)}: differs from the reference's own run")
    assert not bad, "\n".join(bad[:20])


# ---- the NM / PSO hybrid -----------------------------------------------------------------------------
HYB = {b.name: b for b in Cs.hyb_batches()}


@pytest.mark.parametrize("name", list(HYB))
def test_hybrid_follows_the_reference(mod, name):
    batch = HYB[name]
    want = Cs.hyb_reference(batch)
    assert mod.NMPSOEngine.fits(batch.n, H.N_PARAMS)
    with mod.NMPSOEngine(custom(mod, batch.source), len(batch.rows), batch.n, minimize=batch.minimize,
                         bounded=batch.bounded, eps=batch.eps, max_iter=batch.max_iter,
                         no_change_best_iter=batch.no_change, seed=batch.seed, inst_lo=batch.inst_lo) as eng:
        x, st = eng.minimize(starts_of(batch, batch.n), batch.lower if batch.bounded else None,
                             batch.upper if batch.bounded else None, params=params_of(batch))
    bad = []
    for r in range(len(batch.rows)):
        compare(row_tag(batch, r), x[r], st[r], want[r][0], bad)
    assert not bad, "\n".join(bad[:20])


# ---- SANN ----------------------------------------------------------------------------------------------
SANN = {b.name: b for b in Cs.sann_batches()}


@pytest.mark.parametrize("name", list(SANN))
def test_sann_follows_the_reference(mod, name):
    batch = SANN[name]
    want = Cs.sann_reference(batch)
    packed = mod.SANNEngine.chains_per_wave(batch.D, 0 if batch.source == "literal" else H.N_PARAMS)
    assert (packed > 1) == (batch.D <= 64), "the layout this case was written for"
    with mod.SANNEngine(custom(mod, batch.source), len(batch.rows), batch.D, minimize=batch.minimize,
                        max_iter=batch.max_iter, temperature_iter=batch.temp_iter,
                        temperature_max=batch.temp_max, seed=batch.seed, chain_lo=batch.chain_lo) as eng:
        x, st = eng.minimize(starts_of(batch, batch.D), params=params_of(batch))
    bad = []
    for r in range(len(batch.rows)):
        compare(row_tag(batch, r), x[r], st[r], want[r][0], bad)
    assert not bad, "\n".join(bad[:20])
