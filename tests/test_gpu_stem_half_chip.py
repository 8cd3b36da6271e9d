"""The float32 stem where the headline runs it: 128 persistent workgroups (a plan with two lanes), runs of one to
three items per workgroup.  The consumer waves carry the sign word of an item's last unit across the item barrier and
finish its transpose under the next item's MFMAs, and the producers emit an item's row words two periods after it from
three stage buffers (scale_imagenet_amd/csrc/stem.hip, "Hand-off").  Every case checks the bits against the float64
oracle outside the near-tie band and, where two grids exist, that the two grids pack identical rows."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from _util import args_for, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import synth, ttnet
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

N_MAX = 37          # the largest case; the smaller ones use its first images and its oracle rows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def _small(dev, lanes):
    spec, st = spec_and_state("small")
    m = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(N_MAX)
    if lanes > 1:
        m.set_lanes(lanes)
    return m


@pytest.fixture(scope="module")
def two_lanes(dev):
    """Two lanes: the plan launches the float32 stem on 128 workgroups."""
    return _small(dev, 2)


@pytest.fixture(scope="module")
def one_lane(dev):
    """The single-lane twin: 256 workgroups."""
    return _small(dev, 1)


@pytest.fixture(scope="module")
def images():
    return synth.synth_images(N_MAX)


@pytest.fixture(scope="module")
def pre64(images):
    """Float64 pre-activations of all N_MAX images, computed once and only read."""
    _, st = spec_and_state("small")
    pre = OB.stem_pre64(images, st)
    pre.setflags(write=False)
    return pre


def _check_bits(rows, pre, what):
    bits = OB.unpack_rows(rows, 56)
    bad = np.argwhere(bits != (pre >= 0).astype(np.uint8))
    worst = max((abs(pre[tuple(d)]) for d in bad), default=0.0)
    print(f"{what}: {len(bad)} of {bits.size} bits differ from float64, largest |pre| there {worst:.2e}")
    assert worst < OB.NEAR_TIE, what


# n = 1: 7 items on 7 workgroups, one period each, nothing carried.
# n = 19: 133 items on 128 workgroups: runs of one and two items -- a sign word that crosses exactly one barrier, a last
#         item with nothing after it, rows emitted after the last barrier only.
# n = 37: 259 items: runs of two and three -- both tile buffers and all three stage buffers reused, runs that start
#         mid-image (halo copy) and runs that cross an image boundary (whole tile).
@pytest.mark.parametrize("n", [1, 19, 37])
def test_half_chip_bits_and_rows(two_lanes, one_lane, images, pre64, dev, n):
    x = torch.from_numpy(images[:n]).to(dev)
    with torch.no_grad():
        two_lanes(x)
        rows2 = two_lanes.read_stage("features.3", n).copy()
        one_lane(x)
        rows1 = one_lane.read_stage("features.3", n).copy()
    _check_bits(rows2, pre64[:n], f"n = {n}, 128 workgroups")           # (i)
    assert np.array_equal(rows2, rows1), f"n = {n}: the rows of the 128- and the 256-workgroup launch differ"      # (ii)


def test_half_chip_second_lane_and_replay(two_lanes, images, pre64, dev):
    """The same on lane 1 and over repeated calls (plain launches, then the lane's captured graph)."""
    n = 19
    x = torch.from_numpy(images[:n]).to(dev)
    with torch.no_grad():
        for _ in range(4):
            two_lanes(x, lane=1)
        rows = two_lanes.read_stage("features.3", n).copy()
    _check_bits(rows, pre64[:n], "n = 19, lane 1, fourth call")


@pytest.mark.parametrize("nfilter", [4, 16])
def test_half_chip_other_widths(dev, images, nfilter):
    """One and four M-tiles (p = 32, 128) share the consumer loop and the hand-off: two lanes, bits of the float64 oracle."""
    n = 10
    spec = make_spec("small", nfilter, 8, 1)
    st = synth.synth_state_dict(spec, calibrated=False)
    m = ttnet.TT_vf_19lv3_imgnet_small(Namespace(nfilter=nfilter, tfilter=8, layers=1, groups=[1, None, 4, None]))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(N_MAX).set_lanes(2)
    with torch.no_grad():
        m(torch.from_numpy(images[:n]).to(dev))
        rows = m.read_stage("features.3", n).copy()
    _check_bits(rows, OB.stem_pre64(images[:n], st), f"p = {8 * nfilter}, n = {n}, two lanes")
    # beyond the oracle's reach in a quick test: runs of two and three items (n = 37) against the one-item runs of
    # the same images taken ten at a time (70 items on 70 workgroups each)
    with torch.no_grad():
        m(torch.from_numpy(images).to(dev))
        rows37 = m.read_stage("features.3", N_MAX).copy()
        parts = []
        for a in range(0, N_MAX, 10):
            k = min(10, N_MAX - a)
            m(torch.from_numpy(images[a:a + k]).to(dev))
            parts.append(m.read_stage("features.3", k).copy())
    assert np.array_equal(rows37, np.concatenate(parts)), f"p = {8 * nfilter}: runs of items differ from single items"


def test_half_chip_uint8_rows(two_lanes, one_lane, dev):
    """forward_u8: the uint8 instantiation shares the loop and the hand-off; rows with two lanes equal rows with one."""
    n = 19
    u8 = synth.synth_images_u8(n)
    x8 = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev)
    with torch.no_grad():
        two_lanes.forward_u8(x8)
        rows2 = two_lanes.read_stage("features.3", n).copy()
        one_lane.forward_u8(x8)
        rows1 = one_lane.read_stage("features.3", n).copy()
    assert np.array_equal(rows2, rows1)
    _, st = spec_and_state("small")
    _check_bits(rows2, OB.stem_pre64(synth.normalize_u8(u8), st), "uint8 input, n = 19, two lanes")
