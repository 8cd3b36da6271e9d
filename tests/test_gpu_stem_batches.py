"""The stem at real batch sizes: every bit of every image of every batch against the float64 oracle.

What a persistent workgroup of scale_imagenet_amd/csrc/stem.hip does with its run of items -- the tile double buffer, the
three stage buffers whose rows are emitted two periods late, the sign word carried across the item barrier, the halo
copy against a whole-tile load -- only does anything when runs are several items long.  The sizes come from
tests/_stem_partition.py (tests/test_stem_batch_sizes_cpu.py asserts on the CPU what they reach: run lengths 1 to 9,
unequal runs, runs that start mid-image, image boundaries inside a run, runs that hold a whole image, a grid smaller than
the chip), and run on plans reserved for the largest one, with one lane (256 workgroups) and with two (128), in an order
that goes up, down and up again.  Before each size a forward of N_max other images overwrites every row, so a row that
the kernel fails to write cannot read back an earlier right answer.  The oracle (oracle/ttnet_bits.py: stem_pre64_cond)
evaluates the N_max images once per module; a batch of n is the prefix.  Nothing is sampled.

The channel-word output (CP = true), which only the two-launch gate plans read, is compared with the channel words that
launch_rp_to_cp derives from the stem's own rows: a full forward against forward_from_stem_bits(rows of that forward),
every stage and the logits identical.
"""
import time
from argparse import Namespace

import numpy as np
import pytest
import torch

import _stem_cases as SC
import _stem_partition as SP
from _gate_partition import run_order
from _util import spec_and_state
from scale_imagenet_amd import synth, ttnet
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

N_MAX = SP.N_MAX
N_MID = 74                    # runs of 4 and 5 items on 128 workgroups, 2 and 3 on 256, image boundaries inside runs
PATH_TWO_LAUNCH, PATH_FUSED = 0, 1
STEM_KEYS = ("features.1.weight", "features.2.weight", "features.2.bias", "features.2.running_mean", "features.2.running_var")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def _model(dev, nfilter=8, layers=1, lanes=1, n_max=N_MAX, st=None):
    if st is None:
        st = synth.synth_state_dict(make_spec("small", nfilter, 8, layers), calibrated=False)
    m = ttnet.TT_vf_19lv3_imgnet_small(Namespace(nfilter=nfilter, tfilter=8, layers=layers, groups=[1, None, 4, None]))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(n_max)
    if lanes > 1:
        m.set_lanes(lanes)
    return m, st


@pytest.fixture(scope="module")
def one_lane(dev):
    """256 workgroups."""
    return _model(dev, st=spec_and_state("small")[1])[0]


@pytest.fixture(scope="module")
def two_lanes(dev):
    """128 workgroups for float32 input."""
    return _model(dev, st=spec_and_state("small")[1], lanes=2)[0]


@pytest.fixture(scope="module")
def images():
    x = synth.synth_images(N_MAX)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def x_dev(images, dev):
    return torch.from_numpy(images.copy()).to(dev)


@pytest.fixture(scope="module")
def scrub_dev(dev):
    """N_max images none of which is an image of the sweep."""
    return torch.from_numpy(synth.synth_images(N_MAX, first=1000)).to(dev)


@pytest.fixture(scope="module")
def oracle(images):
    """Packed oracle rows and near-tie mask of all N_max images at p = 64, computed once and only read."""
    t0 = time.time()
    want, band = SC.oracle_rows(images, spec_and_state("small")[1])
    print(f"float64 oracle over {N_MAX} images: {time.time() - t0:.1f} s, {SC.count_bits(band)} outputs inside the near-tie band")
    return want, band


def _rows(m, x, scrub, n, lane=0, u8=False):
    with torch.no_grad():
        m(scrub, lane=lane)
        (m.forward_u8 if u8 else m)(x[:n], lane=lane)
        return m.read_stage("features.3", n).copy()


def test_float32_sweep_both_grids(one_lane, two_lanes, x_dev, scrub_dev, oracle):
    want, band = oracle
    order = run_order(SP.SIZES)
    assert order[0] == min(SP.SIZES) and order[1] == order[-1] == N_MAX
    t0 = time.time()
    for n in order:
        rows2 = _rows(two_lanes, x_dev, scrub_dev, n)
        rows1 = _rows(one_lane, x_dev, scrub_dev, n)
        for rows, G in ((rows2, 128), (rows1, 256)):
            inside = SC.check_rows(rows, want[:n], band[:n], f"n = {n} on {G} workgroups (runs of {SP.run_lengths(n, G)} items)")
            print(f"n = {n}, {G} workgroups, runs of {SP.run_lengths(n, G)}: {inside} bits differ, all inside the band")
        assert np.array_equal(rows2, rows1), f"n = {n}: the rows of the 128- and the 256-workgroup launch differ"
        assert one_lane._any_plan().query("range_overflow") == 0 and two_lanes._any_plan().query("range_overflow") == 0
    assert one_lane._any_plan().query("lanes") == 1 and two_lanes._any_plan().query("lanes") == 2
    assert one_lane._any_plan().query("max_batch") == two_lanes._any_plan().query("max_batch") == N_MAX
    print(f"sizes {order}: {2 * sum(order)} images compared with the oracle, {time.time() - t0:.1f} s")


def test_second_lane_and_graph_replay(two_lanes, x_dev, scrub_dev, oracle):
    """n = 74 on lane 1; the fourth call of one batch size on a lane is the replay of its captured graph."""
    want, band = oracle
    for call in range(4):
        with torch.no_grad():
            two_lanes(scrub_dev, lane=1)
            plan = two_lanes._any_plan()
            before = plan.query("graph_replays")
            two_lanes(x_dev[:N_MID], lane=1)
            replayed = plan.query("graph_replays") - before
            rows = two_lanes.read_stage("features.3", N_MID).copy()
        SC.check_rows(rows, want[:N_MID], band[:N_MID], f"n = {N_MID}, lane 1, call {call + 1}")
    assert plan.query("graphs_enabled") == 1 and replayed == 1, "the fourth call did not replay a captured graph"
    assert plan.query("range_overflow") == 0


def _u8_specials():
    """[4,3,224,224] uint8: all 0, all 255, an image with bright and dark borders (the border-class corrections of the
    uint8 kernel), a checkerboard of 0 / 255 in cells of 2 x 2 pixels (pooled values alternate between the extremes)."""
    out = np.zeros((4, 3, 224, 224), dtype=np.uint8)
    out[1] = 255
    out[2] = synth.synth_images_u8(1, first=2000)[0]
    out[2, :, :4, :] = 255
    out[2, :, -4:, :] = 3
    out[2, :, :, :4] = 200
    out[2, :, :, -4:] = 17
    yy, xx = np.mgrid[0:224, 0:224]
    out[3] = (((yy >> 1) + (xx >> 1)) & 1).astype(np.uint8) * 255
    return out


def test_uint8_sweep(one_lane, scrub_dev, dev):
    """forward_u8 over the same sizes (always 256 workgroups), the oracle on normalize_u8.  Four images of every batch
    are replaced by constant and border images, at the indices tests/_stem_partition.py names: the first image, the last
    one, one with a run start inside it and one that begins in the middle of a run."""
    st = spec_and_state("small")[1]
    u8 = np.concatenate([synth.synth_images_u8(N_MAX), _u8_specials()])
    t0 = time.time()
    want_all, band_all = SC.oracle_rows(synth.normalize_u8(u8), st)
    print(f"float64 oracle over {len(u8)} uint8 images: {time.time() - t0:.1f} s")
    hwc = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev)
    for n in run_order(SP.SIZES):
        edges = SP.edge_images(n, SP.GRID_U8)
        x = hwc[:n].clone()
        want, band = want_all[:n].copy(), band_all[:n].copy()
        for k, i in enumerate(edges):
            x[i] = hwc[N_MAX + k]
            want[i], band[i] = want_all[N_MAX + k], band_all[N_MAX + k]
        rows = _rows(one_lane, x, scrub_dev, n, u8=True)
        inside = SC.check_rows(rows, want, band, f"uint8 input, n = {n} (runs of {SP.run_lengths(n, SP.GRID_U8)} items, constant images at {edges})")
        print(f"uint8 n = {n}, constant images at {edges}: {inside} bits differ, all inside the band")
    assert one_lane._any_plan().query("range_overflow") == 0


@pytest.mark.parametrize("nfilter", [4, 16])
def test_other_widths_at_run_lengths_four_and_five(dev, images, x_dev, scrub_dev, nfilter):
    """One and four M-tiles (p = 32, 128) with two lanes at n = 74 against the oracle."""
    m, st = _model(dev, nfilter=nfilter, lanes=2, n_max=N_MID)
    want, band = SC.oracle_rows(images[:N_MID], st)
    rows = _rows(m, x_dev, scrub_dev[:N_MID], N_MID)
    assert rows.shape == (N_MID, 8 * nfilter, 56)
    inside = SC.check_rows(rows, want, band, f"p = {8 * nfilter}, n = {N_MID}, two lanes")
    print(f"p = {8 * nfilter}, n = {N_MID}, 128 workgroups: {inside} bits differ, all inside the band")
    assert m._any_plan().query("range_overflow") == 0


def _stages(spec):
    out = ["features.3"]
    for b in spec.blocks:
        out += [f"{b.name}.out{k}" for k in (1, 2, 3, 4)]
        if not b.last:
            out.append(b.name)
    return out + ["flatten"]


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("layers,unfused", [(3, False), (1, True)])
def test_channel_words_of_multi_item_runs(dev, monkeypatch, x_dev, scrub_dev, oracle, layers, unfused, lanes):
    """The two-launch gate plans read the stem's channel words.  A full forward (channel words from the stem's own
    epilogue, runs of 2 .. 5 items) against forward_from_stem_bits on the rows of that forward (channel words derived
    from the rows): every stage and the logits identical; the rows themselves against the oracle."""
    n = N_MID
    spec = make_spec("small", 8, 8, layers)
    if unfused:
        monkeypatch.setenv("TTNET_GATE_UNFUSED", "1")         # read at plan creation
    m, st = _model(dev, layers=layers, lanes=lanes, n_max=n)
    for k in STEM_KEYS:                                        # the stem of every depth is the stem of the oracle fixture
        assert np.array_equal(st[k], spec_and_state("small")[1][k]), k
    with torch.no_grad():
        m(scrub_dev[:n])                                       # creates the plan
    if unfused:
        monkeypatch.delenv("TTNET_GATE_UNFUSED")
    plan = m._any_plan()
    assert plan.query("gate_path") == PATH_TWO_LAUNCH and plan.query("lanes") == lanes
    with torch.no_grad():
        y = m(x_dev[:n]).clone()
        full = {s: m.read_stage(s, n).copy() for s in _stages(spec)}
    want, band = oracle
    SC.check_rows(full["features.3"], want[:n], band[:n], f"--layers {layers}, {lanes} lane(s), n = {n}")
    with torch.no_grad():
        m(scrub_dev[:n])
        y2 = m.forward_from_stem_bits(torch.from_numpy(full["features.3"].view(np.int64)).to(dev)).clone()
        again = {s: m.read_stage(s, n).copy() for s in _stages(spec)}
    for s in full:
        wrong = np.flatnonzero((full[s] != again[s]).reshape(n, -1).any(axis=1))
        assert wrong.size == 0, (f"--layers {layers}, {lanes} lane(s): stage {s} of the full forward differs from the forward from its own "
                                 f"stem rows in {wrong.size} of {n} images (first {wrong[:8].tolist()}): the stem's channel words "
                                 f"are not the channel words of its rows")
    assert torch.equal(y, y2)
    assert plan.query("range_overflow") == 0
