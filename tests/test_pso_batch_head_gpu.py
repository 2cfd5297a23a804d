"""The head inside the resident batch PSO kernel (pso_batch_head: scan of the last evaluation,
swarm-best rule, std_err of the personal bests, no-change counter, stop tests) against the
independent references of tests/_head_ref.py -- not only against the turn engine it restates. The
scheme of test_pso_head_follows_the_reference: whole-vector objectives that score ties, NaN and
+inf, three turns; before each, the downloaded positions give f and RefPSOHead takes the turn on
them. Every solve of the batch (its own seed) is followed by its own reference.

n = 1: std_err divides by n - 1 = 0. The sum of squared deviations is 0 (or NaN where the one
personal best is still +inf), so the statistic is NaN in IEEE arithmetic whatever the order of the
sums; NaN < eps is false and the test never stops the solve. The literal Python formula raises on
the integer zero instead, so the reference is handed that NaN."""
import math

import numpy as np
import pytest

from tests import _head_common as H
from tests import _head_ref as R

pytestmark = pytest.mark.gpu

OBJECTIVES = {
    "ties": ("return floor(x(0) * 8);", lambda P: np.floor(P[:, 0] * 8)),
    "nan": ('return x(1) > 0.5 ? __builtin_nan("") : x(0);',
            lambda P: np.where(P[:, 1] > 0.5, np.nan, P[:, 0])),
    "inf": ("return x(1) > 0.5 ? __builtin_inf() : x(0);",
            lambda P: np.where(P[:, 1] > 0.5, np.inf, P[:, 0])),
}


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    return nlsolver_amd


def same_array(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("n", [1, 255, 1023, 1024])
@pytest.mark.parametrize("ptype", [0, 1], ids=["vanilla", "accelerated"])
@pytest.mark.parametrize("eps", [0.0, R.EPS_TINY], ids=["eps0", "eps"])
@pytest.mark.parametrize("objective", sorted(OBJECTIVES))
def test_resident_pso_head_follows_the_reference(mod, objective, eps, ptype, n):
    body, f = OBJECTIVES[objective]
    obj = mod.CustomObjective(body, vector=True)
    B = 3
    seeds = [12374563468 + 7919 * b for b in range(B)]
    refs = [R.RefPSOHead(n, max_iter=5000, best_val_no_change=2, eps=eps) for _ in range(B)]
    best_pos, updates = [None] * B, 0  # swarm_best_position = positions[best] at the last update, :2736
    with mod.PSOBatchEngine(obj, B, n, 2, type=ptype, eps=eps, max_iter=5000, best_val_no_change=2) as eng:
        eng.init(-1.0, 1.0, seeds)
        for turn in range(3):
            was_done = []
            for b, ref in enumerate(refs):
                pos, _, pbest, cur = eng.download(b)
                vals = f(pos)
                assert same_array(cur, vals), f"turn {turn} solve {b}: the device's f differs from numpy's"
                was_done.append(ref.done)
                old_best = ref.swarm_best_value
                ref.turn(vals, std_err=math.nan if n == 1 else None)
                if not was_done[b]:
                    assert same_array(pbest, np.array(ref.particle_best_values)), f"turn {turn} solve {b}: pbest"
                    if ref.swarm_best_value < old_best:
                        best_pos[b] = pos[ref.swarm_best_index].copy()
                        updates += 1
            eng.step(1)
            sts = eng.status()
            bx, bf, bi = eng.best()
            for b, ref in enumerate(refs):
                st, tag = sts[b], f"turn {turn} solve {b}"
                assert (st.val_no_change, bool(st.done), st.iteration) == \
                    (ref.val_no_change, ref.done, ref.iter), tag
                assert R.same_double(st.f_value, ref.swarm_best_value), tag
                assert R.same_double(bf[b], ref.swarm_best_value), tag
                if best_pos[b] is not None:
                    assert st.best_index == bi[b] == ref.swarm_best_index, tag
                    assert same_array(bx[b], best_pos[b]), f"{tag}: best position {bx[b]} != {best_pos[b]}"
                if eps > 0 and not was_done[b]:
                    if n == 1:
                        assert st.std_err != st.std_err, f"{tag}: std_err {st.std_err!r} of one value is not NaN"
                    else:
                        pb = np.array(ref.particle_best_values)
                        ok, _, text = R.judge_std_err(st.std_err, pb, H.L_UNSHARDED)
                        assert ok, f"{tag}: std_err {text}"
    if n > 1:
        assert updates >= 1  # the swarm best was copied at least once
