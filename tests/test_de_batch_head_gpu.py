"""The head inside the resident batch DE kernel (de_batch_head: best scan, incumbent rule, std_err,
counter, stop tests) against the independent references of tests/_head_ref.py -- not only against
the turn engine it restates. One case of R.cases(n) per solve of a batch, the comparisons of
test_de_head_follows_the_reference: row i of every population is filled with i, turn 1 scans a
vector whose unique minimum places the incumbent, turn 2 scans the hostile vector (an upload
overwrites what the generation between them did)."""
import math

import numpy as np
import pytest

from tests import _head_common as H
from tests import _head_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import nlsolver_amd
    return nlsolver_amd


def tree_std_err(oracle, vec):
    v = np.ascontiguousarray(vec, dtype=np.float64)
    m2 = oracle.orc_tiled_m2_merged(H.O._ptr(v), v.size, None)
    return math.sqrt(m2 / (v.size - 1)) if m2 == m2 else math.nan


@pytest.mark.parametrize("n", [4, 5, 255, 256, 257, 1023, 1024])
@pytest.mark.parametrize("strategy", [1, 0], ids=["random", "best"])
def test_resident_head_follows_the_reference(mod, oracle, n, strategy):
    D = 2
    cs = R.cases(n)
    B = len(cs)
    rows = np.broadcast_to(np.arange(n, dtype=np.float64)[None, :, None], (B, n, D))
    with mod.DEBatchEngine("sphere", B, n, D, strategy=strategy, eps=R.EPS_TINY, max_iter=1000,
                           best_val_no_change=10 ** 6) as eng:
        eng.init(np.ones((B, D)), [12374563468 + 7919 * b for b in range(B)])
        eng.upload(rows, np.stack([c.place for c in cs]))
        eng.step(1)
        eng.upload(rows, np.stack([c.vec for c in cs]))
        eng.step(1)
        sts = eng.status()
        bx, bf, bi = eng.best()
    bad = []
    for b, c in enumerate(cs):
        tag, st = f"{c.name} inc {c.inc}", sts[b]
        got = (st.best_index, st.val_no_change, st.iteration, bool(st.done))
        if got != c.want:
            bad.append(f"{tag}: (best, vnc, iter, done) {got} != reference {c.want}")
        if not R.same_double(st.f_value, c.f_value) or not R.same_double(bf[b], c.f_value):
            bad.append(f"{tag}: f_value {st.f_value!r} / {bf[b]!r} != reference {c.f_value!r}")
        if bi[b] != c.want[0] or not np.all(bx[b] == float(c.want[0])):
            bad.append(f"{tag}: best() gives agent {bi[b]} row {bx[b]}, reference agent {c.want[0]}")
        want_bits = tree_std_err(oracle, c.vec)
        if not R.same_double(st.std_err, want_bits):
            bad.append(f"{tag}: std_err {st.std_err!r} != restatement {want_bits!r}")
        if c.judge:
            ok, _, text = R.judge_std_err(st.std_err, c.vec, H.L_UNSHARDED)
            if not ok:
                bad.append(f"{tag}: std_err {text}")
    assert not bad, f"n {n}: {len(bad)} mismatches\n" + "\n".join(bad[:40])
