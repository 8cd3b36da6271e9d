"""The stem on values and BatchNorm parameters beyond the synthetic ones, and the edges of its range flag.

scale_imagenet_amd/csrc/stem.hip promises any float32 input with pooled |x| < 4094, any BatchNorm whose folded shift fits
the shift row, and one power-of-two prescale for the whole folded weight tensor.  The cases of tests/_stem_cases.py --
full mantissas, inputs x 100 / x 1500 / x 1e-4, an offset of 300, BatchNorm scales 2^12 apart with a negative and a
zero gamma, running statistics that spread the scales and blow up the shift -- run here on TT-small p = 64 at n = 19
with two lanes (128 workgroups, runs of one and two items) and n = 8 with one lane.  Every bit outside the band
tau(o) = NEAR_TIE * max(1, E(o) / E0) equals (pre >= 0) of the float64 oracle; tests/test_stem_split_bound_cpu.py pins
the band on the CPU (the split arithmetic stays within half of it) -- what is measured only here is the float32
accumulation inside the MFMAs.  The range flag stays down in every case.
"""
import numpy as np
import pytest
import torch

import _stem_cases as SC
from _util import args_for, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import _lib, synth, ttnet

pytestmark = pytest.mark.gpu

N2, N1 = 19, 8                # two lanes: 133 items on 128 workgroups; one lane: 56 items on 56 workgroups


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def _small(dev, lanes, n_max):
    _, st = spec_and_state("small")
    m = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(n_max)
    if lanes > 1:
        m.set_lanes(lanes)
    return m


@pytest.fixture(scope="module")
def two_lanes(dev):
    return _small(dev, 2, N2)


@pytest.fixture(scope="module")
def one_lane(dev):
    return _small(dev, 1, N1)


@pytest.fixture(scope="module")
def synthetic():
    """(images, pre, E) of the synthetic case, computed once and only read."""
    x = SC.case_images("synthetic", N2)
    pre, E = OB.stem_pre64_cond(x, SC.case_state("synthetic"))
    for a in (x, pre, E):
        a.setflags(write=False)
    return x, pre, E


def _compare(rows, pre, E, what):
    """Every differing bit lies inside the band; prints their count and the largest |pre| / tau among them."""
    bad = OB.unpack_rows(rows, 56) != (pre >= 0).astype(np.uint8)
    ratio = np.abs(pre[bad]) / SC.tau(E[bad])
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{what}: {int(bad.sum())} of {bad.size} bits differ from float64, largest |pre| / tau among them {worst:.3f} "
          f"(max E / E0 {float(E.max()) / SC.e0():.3g})")
    assert worst < 1.0, f"{what}: a bit differs at |pre| = {worst:.3g} tau"
    return worst


@pytest.mark.parametrize("case", SC.CASES)
def test_values_and_batchnorm_cases(two_lanes, one_lane, synthetic, dev, case):
    st = SC.case_state(case)
    if case == "synthetic":
        x, pre, E = synthetic
    else:
        x = SC.case_images(case, N2)
        pre, E = OB.stem_pre64_cond(x, st)
    xd = torch.from_numpy(x.copy()).to(dev)
    reload = case in SC.BN_CASES
    try:
        for m, n, what in ((two_lanes, N2, "two lanes"), (one_lane, N1, "one lane")):
            if reload:
                m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
            with torch.no_grad():
                m(xd[:n])
                rows = m.read_stage("features.3", n).copy()
            _compare(rows, pre[:n], E[:n], f"{case}, n = {n}, {what}")
            assert m._any_plan().query("range_overflow") == 0, f"{case}, n = {n}: range flag raised"
    finally:
        if reload:
            base = spec_and_state("small")[1]
            for m in (two_lanes, one_lane):
                m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in base.items()}, strict=True)


# The last item of the last workgroup at n = 19 is the last row block (output rows 48 .. 55) of image 18: pooled rows 93 .. 111.
LAST = N2 - 1


def _with_block(x, value):
    """A 4 x 4 block of raw pixels (2 x 2 pooled ones) in the last image's last rows."""
    x = x.copy()
    x[LAST, 1, 220:224, 100:104] = value
    return x


def test_pooled_value_just_inside_the_range(two_lanes, synthetic, dev):
    """Pooled 4090 (x 16 = 65440, the fp16 maximum is 65504): no flag, and the image's bits match under the band."""
    x0, pre0, E0 = synthetic
    x = _with_block(x0, 4090.0)
    pre, E = OB.stem_pre64_cond(x[LAST:], SC.case_state("synthetic"))
    assert E.max() > 10 * SC.e0()                     # (the band is wider there, and only there)
    with torch.no_grad():
        two_lanes(torch.from_numpy(x).to(dev))
        rows = two_lanes.read_stage("features.3", N2).copy()
    assert two_lanes._any_plan().query("range_overflow") == 0
    _compare(rows[LAST:], pre, E, "pooled 4090 in the last item")
    _compare(rows[:LAST], pre0[:LAST], E0[:LAST], "the other images")


def test_single_pixels_outside_the_range_pool_inside(two_lanes, synthetic, dev):
    """Pixels of +-6000 whose 2 x 2 mean is 250: the range is a range of POOLED values, so no flag, and the bits match."""
    x0, pre0, E0 = synthetic
    x = x0.copy()
    quad = np.array([[6000.0, -6000.0], [6000.0, -5000.0]], dtype=np.float32)       # ((a + b) + c) + d = 1000 exactly
    where = [(0, 0, 0, 0), (0, 2, 222, 222), (9, 1, 100, 60), (LAST, 0, 222, 0), (LAST, 2, 110, 222)]
    for i, c, y, xx in where:
        x[i, c, y:y + 2, xx:xx + 2] = quad
    touched = sorted({w[0] for w in where})
    pre, E = OB.stem_pre64_cond(x[touched], SC.case_state("synthetic"))
    pooled = 0.25 * x[:, :, 0::2, 0::2].astype(np.float64) + 0.25 * x[:, :, 0::2, 1::2] + 0.25 * x[:, :, 1::2, 0::2] + 0.25 * x[:, :, 1::2, 1::2]
    assert np.abs(pooled).max() == 250.0 and np.abs(x).max() == 6000.0
    with torch.no_grad():
        two_lanes(torch.from_numpy(x).to(dev))
        rows = two_lanes.read_stage("features.3", N2).copy()
    assert two_lanes._any_plan().query("range_overflow") == 0
    _compare(rows[touched], pre, E, f"pixels of +-6000 pooling to 250 in images {touched}")
    rest = [i for i in range(N2) if i not in touched]
    _compare(rows[rest], pre0[rest], E0[rest], "the other images")


def test_pooled_value_just_outside_the_range_is_loud(two_lanes, synthetic, dev):
    """Pooled 4100 (x 16 = 65600: fp16 infinity) in the last item of the last workgroup: the flag is raised, reads 1 and
    then 0, and the next forward of clean images is bit-identical to the one before."""
    x0 = synthetic[0]
    clean = torch.from_numpy(x0.copy()).to(dev)
    bad = torch.from_numpy(_with_block(x0, 4100.0)).to(dev)
    plan_of = two_lanes._any_plan
    with torch.no_grad():
        y0 = two_lanes(clean).clone()
        rows0 = two_lanes.read_stage("features.3", N2).copy()
        assert plan_of().query("range_overflow") == 0
        two_lanes(bad)                               # asynchronous: returns before the kernel has run
        torch.cuda.synchronize()
        with pytest.raises(_lib.TTNetError) as ei:
            two_lanes(clean)
        assert ei.value.status == -6 and b"range" in _lib.load().ttnet_last_error()
        assert plan_of().query("range_overflow") == 1     # read and clear
        assert plan_of().query("range_overflow") == 0
        y1 = two_lanes(clean).clone()
        rows1 = two_lanes.read_stage("features.3", N2).copy()
    assert torch.equal(y1, y0) and np.array_equal(rows1, rows0)
    assert plan_of().query("range_overflow") == 0
