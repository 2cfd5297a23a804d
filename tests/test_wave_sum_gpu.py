"""wave_sum on the device (NLSG_PROBE_WAVE_SUM: every lane returns the sum over its wave's 64
inputs) against the numpy restatement of the xor butterfly (tests/_wave_sum.py, itself checked
against math.fsum in tests/test_wave_sum_cpu.py): all 64 lanes bit for bit where the result is not
NaN; where it is, every lane is NaN and lane 0 — the lane the kernels read, and the one whose
operand order (own first) every level keeps — holds the restatement's bits. 4 096 waves: random
normals; magnitudes over 600 binades with cancellation; +-0, subnormals, +-inf; one NaN per wave."""
import numpy as np
import pytest

from tests import _wave_sum as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available()
    from nlsolver_amd import _capi
    return _capi.probe_math


def test_wave_sum_bit_exact_in_every_lane(probe):
    v = W.all_inputs()
    assert v.shape == (4096, 64)
    ref = W.butterfly(v)
    dev = probe("wave_sum", v.view(np.uint64).ravel()).reshape(v.shape)
    ref_bits = ref.view(np.uint64)
    nan = np.isnan(ref)
    assert nan[3072:].all() and not nan[:3072].any()  # exactly the waves that were given a NaN
    bad = np.argwhere((dev != ref_bits) & ~nan)
    assert bad.size == 0, (bad[:5], [(hex(dev[w, l]), hex(ref_bits[w, l])) for w, l in bad[:5]])
    assert np.isnan(dev.view(np.float64)[nan]).all()
    bad0 = np.flatnonzero((dev[:, 0] != ref_bits[:, 0]) & nan[:, 0])
    assert bad0.size == 0, (bad0[:5], [(hex(dev[w, 0]), hex(ref_bits[w, 0])) for w in bad0[:5]])


def test_wave_sum_probe_takes_whole_waves(probe):
    with pytest.raises(Exception):
        probe("wave_sum", np.zeros(65, dtype=np.uint64))
