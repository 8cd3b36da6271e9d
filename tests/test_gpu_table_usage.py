"""GPU: truth-table usage counts (ttnet_plan_table_usage_enable / _reset / ttnet_table_usage_add / ttnet_plan_get_table_usage).

The expected value of every check is ``np.bincount(oracle.ttnet_bits.window_index(...))`` per group: the bit oracle
(``multihead_block_bits`` with ``taps``) runs from the device's own ``features.3`` stage on the device's own tables
(``get_table``), so stem near ties cannot enter, and every comparison is exact int64 equality for every ``Block_TT`` of the
model, the float last block included."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from _util import args_for, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import _lib, synth, ttnet
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

CLASSES = {"small": ttnet.TT_vf_19lv3_imgnet_small, "xsmall": ttnet.TT_vf_19lv3_imgnet_xsmall, "full": ttnet.TT_vf_19lv3_imgnet}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def make_model(dev, variant="small", nfilter=8, tfilter=8, layers=1, reserve=64):
    if (nfilter, tfilter, layers) == (8, 8, 1):
        spec, st = spec_and_state(variant)
        args = args_for(variant)
    else:
        spec = make_spec(variant, nfilter, tfilter, layers)
        st = synth.synth_state_dict(spec, calibrated=False)
        args = Namespace(nfilter=nfilter, tfilter=tfilter, layers=layers, groups=[1, None, 4, None])
    m = CLASSES[variant](args)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(reserve)
    with torch.no_grad():
        m(torch.from_numpy(synth.synth_images(1)).to(dev))          # builds the plan and the tables
    torch.cuda.synchronize()
    return m


_SMALL = {}


@pytest.fixture
def small(dev):
    """TT-small p = 64 --layers 1 with counting on (built once, its tables read back once), counters zeroed per test."""
    if "m" not in _SMALL:
        m = make_model(dev, reserve=64)
        m.count_table_usage(True)
        _SMALL["m"], _SMALL["luts"] = m, device_tables(m)
    m = _SMALL["m"]
    m.set_lanes(1)
    m.reset_table_usage()
    return m, _SMALL["luts"]


def device_tables(m):
    return {b.name: m.get_table(b.name) for b in m.spec.block_tts()}


def bincount_groups(idx, b):
    """uint32 [N, G, Ho, Wo] canonical indices -> int64 [G, 2^n]."""
    size = 1 << b.fan_in_bits
    return np.stack([np.bincount(idx[:, g].ravel(), minlength=size) for g in range(b.groups)]).astype(np.int64)


def expected_usage(stem_rows, spec, luts):
    """The definition, on the bit oracle: from row-packed stem bits [N, p, 56]."""
    x = OB.unpack_rows(stem_rows, 56)
    want = {}
    for blk in spec.blocks:
        taps = {}
        y = OB.multihead_block_bits(x, luts, blk, spec.variant, taps)
        for b in (blk.conv1, blk.conv2, blk.conv3):
            want[b.name] = bincount_groups(OB.window_index(x, b), b)
        outs = [taps[f"{blk.name}.out{k}"] for k in (1, 2, 3, 4)]
        n_, c, hh, ww = outs[0].shape
        outf = np.stack(outs, axis=2).reshape(n_, 4 * c, hh, ww)     # channel 4c + branch, after the branch padding
        want[blk.convf.name] = bincount_groups(OB.window_index(outf, blk.convf), blk.convf)
        x = y
    return want


def assert_usage_equal(got, want, tag=""):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == np.int64 and got[name].shape == want[name].shape, (tag, name)
        if not np.array_equal(got[name], want[name]):
            d = np.argwhere(got[name] != want[name])
            raise AssertionError(f"{tag} {name}: {len(d)} counters differ, first (group, index) {d[:4].tolist()}: got "
                                 f"{[int(got[name][tuple(i)]) for i in d[:4]]}, want {[int(want[name][tuple(i)]) for i in d[:4]]}")


def assert_row_sums(m, usage, images):
    for blk in m.spec.blocks:
        h, w = blk.in_hw
        for b in (blk.conv1, blk.conv2, blk.conv3):
            ho, wo = b.out_hw(h, w)
            assert (usage[b.name].sum(axis=1) == images * ho * wo).all(), b.name
        ho, wo = blk.out_hw
        assert (usage[blk.convf.name].sum(axis=1) == images * ho * wo).all(), blk.convf.name


def forward_and_add(m, x, lane=0):
    with torch.no_grad():
        y = m(x, lane=lane)
    m.add_table_usage(lane)
    return y


def sum_usage(*parts):
    return {k: sum(p[k] for p in parts) for k in parts[0]}


def check_against_oracle(m, luts, x, tag):
    m.reset_table_usage()
    forward_and_add(m, x)
    rows = m.read_stage("features.3", x.shape[0])
    got = m.table_usage()
    assert_usage_equal(got, expected_usage(rows, m.spec, luts), tag)
    assert_row_sums(m, got, x.shape[0])
    return got


def test_small_p64_golden_images(small, dev):
    m, luts = small
    got = check_against_oracle(m, luts, torch.from_numpy(synth.synth_images(8)).to(dev), "small p=64")
    assert m._any_plan().query("usage_bytes") >= sum(a.nbytes for a in got.values())


@pytest.mark.parametrize("variant,nfilter,tfilter,layers", [("small", 4, 8, 1), ("small", 8, 8, 0), ("small", 8, 8, 2),
                                                            ("small", 8, 8, 3), ("xsmall", 8, 8, 1)])
def test_other_geometries(dev, variant, nfilter, tfilter, layers):
    """p = 32, --layers 0 and 2 (block-fused geometries), --layers 3 (two-launch path), x-small."""
    m = make_model(dev, variant, nfilter, tfilter, layers, reserve=8)
    m.count_table_usage(True)
    check_against_oracle(m, device_tables(m), torch.from_numpy(synth.synth_images(8)).to(dev), f"{variant} p={nfilter * tfilter} l={layers}")
    m.count_table_usage(False)


@pytest.mark.parametrize("n", [1, 37])
def test_batch_sizes(small, dev, n):
    m, luts = small
    check_against_oracle(m, luts, torch.from_numpy(synth.synth_images(n, first=11)).to(dev), f"n={n}")


def test_large_batch_equals_the_sum_of_its_parts(dev):
    """600 images walk several rounds inside a workgroup of the block-fused kernel (and the grid-stride loop of the
    counting kernels): the counts equal those of the same images run 200 at a time."""
    m = make_model(dev, reserve=600)
    m.count_table_usage(True)
    base = torch.from_numpy(synth.synth_images(200)).to(dev)
    x = torch.cat([base, base.flip(0), base.roll(7, 0)])
    forward_and_add(m, x)
    whole = m.table_usage()
    m.reset_table_usage()
    forward_and_add(m, base)
    part = m.table_usage()
    assert_usage_equal(whole, {k: 3 * v for k, v in part.items()}, "600 vs 3 x 200")
    assert_row_sums(m, whole, 600)
    m.count_table_usage(False)


def test_five_adds_and_graph_replay(small, dev):
    m, luts = small
    x = torch.from_numpy(synth.synth_images(24, first=40)).to(dev)
    forward_and_add(m, x)
    one = m.table_usage()
    m.reset_table_usage()
    plan = m._any_plan()
    before = plan.query("graph_replays")
    for _ in range(5):
        forward_and_add(m, x)
    got = m.table_usage()
    assert plan.query("graphs_enabled") == 1, _lib.load().ttnet_last_error()
    assert plan.query("graph_replays") > before
    assert_usage_equal(got, {k: 5 * v for k, v in one.items()}, "5 x")


def test_two_lanes_two_streams(small, dev):
    m, luts = small
    xa = torch.from_numpy(synth.synth_images(16, first=0)).to(dev)
    xb = torch.from_numpy(synth.synth_images(16, first=300)).to(dev)
    alone = []
    for x in (xa, xb):
        m.reset_table_usage()
        forward_and_add(m, x)
        alone.append(m.table_usage())
    m.reset_table_usage()
    torch.cuda.synchronize()
    m.set_lanes(2)
    assert m._any_plan().query("lanes") == 2
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    for rep in range(4):                                 # plain launches first, then replayed graphs per lane
        for lane, x in enumerate((xa, xb)):
            with torch.cuda.stream(streams[lane]):
                forward_and_add(m, x, lane)
    torch.cuda.synchronize()
    assert_usage_equal(m.table_usage(), {k: 4 * v for k, v in sum_usage(*alone).items()}, "two lanes")


def test_u8_and_stem_bits_entry_points(small, dev):
    m, luts = small
    g = torch.Generator().manual_seed(5)
    x8 = torch.randint(0, 256, (6, 224, 224, 3), dtype=torch.uint8, generator=g).to(dev)
    with torch.no_grad():
        m.forward_u8(x8)
    m.add_table_usage(0)
    rows = m.read_stage("features.3", 6)
    assert_usage_equal(m.table_usage(), expected_usage(rows, m.spec, luts), "forward_u8")
    m.reset_table_usage()
    rng = np.random.default_rng(3)
    bits = (rng.random((5, m.spec.p, 56, 56)) < 0.3).astype(np.uint8)
    rows = OB.pack_rows(bits)
    with torch.no_grad():
        m.forward_from_stem_bits(torch.from_numpy(rows.view(np.int64)).to(dev))
    m.add_table_usage(0)
    assert_usage_equal(m.table_usage(), expected_usage(rows, m.spec, luts), "from_stem_bits")


def test_logits_do_not_change_and_reset_zeroes(dev):
    m = make_model(dev, reserve=16)
    x = torch.from_numpy(synth.synth_images(16, first=70)).to(dev)
    with torch.no_grad():
        off = [m(x).clone() for _ in range(4)]
    m.count_table_usage(True)
    on = [forward_and_add(m, x).clone() for _ in range(4)]
    torch.cuda.synchronize()
    for a, b in zip(off, on):
        assert torch.equal(a, b)
    assert all(v.sum() > 0 for v in m.table_usage().values())
    m.reset_table_usage()
    assert all(not v.any() for v in m.table_usage().values())
    m.count_table_usage(False)
    assert m._any_plan().query("usage_bytes") == 0
    with torch.no_grad():
        assert torch.equal(m(x), off[0])


def test_error_contract(dev):
    lib = _lib.load()
    m = make_model(dev, reserve=4)
    plan = m._any_plan()
    buf = np.empty((4, 65536), dtype=np.int64)
    name = b"features.4.Block_conv3"
    assert lib.ttnet_table_usage_add(plan.handle, 0, None) == -2                       # TTNET_E_STATE
    assert lib.ttnet_plan_get_table_usage(plan.handle, name, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -2
    assert lib.ttnet_plan_table_usage_reset(plan.handle, None) == -2
    m.count_table_usage(True)
    assert lib.ttnet_plan_get_table_usage(plan.handle, name, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 8) == -1      # TTNET_E_INVALID
    assert lib.ttnet_plan_get_table_usage(plan.handle, b"features.9.Block_conv3", buf.ctypes.data_as(C.c_void_p), buf.nbytes) == -1
    assert lib.ttnet_table_usage_add(plan.handle, 3, None) == -1
    assert lib.ttnet_plan_get_table_usage(plan.handle, name, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    m.count_table_usage(False)
    spec, st = spec_and_state("full")
    f = ttnet.TT_vf_19lv3_imgnet(args_for("full"))
    f.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    f = f.to(dev).eval().reserve(2)
    with torch.no_grad():
        f(torch.from_numpy(synth.synth_images(1)).to(dev))
    with pytest.raises(_lib.TTNetError) as e:
        f.count_table_usage(True)
    assert e.value.status == -4 and "fan-in 30" in str(e.value)                         # TTNET_E_UNSUPPORTED


def test_evaluate_table_usage(dev):
    from scale_imagenet_amd.evaluate import evaluate
    m = make_model(dev, reserve=16)
    batches = [(torch.from_numpy(synth.synth_images(n, first=20 * i)), torch.from_numpy(synth.synth_targets(n, first=20 * i)))
               for i, n in enumerate((16, 16, 16, 16, 9))]
    plain = evaluate(m, batches, dev, inflight=2, metrics="device")
    assert plain.table_usage is None
    res = evaluate(m, batches, dev, inflight=2, metrics="device", table_usage=True)
    assert (res.loss, res.top1, res.top5, res.images) == (plain.loss, plain.top1, plain.top5, plain.images)
    parts = []
    m.set_lanes(1)
    for x, _ in batches:
        m.reset_table_usage()
        forward_and_add(m, x.to(dev))
        parts.append(m.table_usage())
    assert_usage_equal(res.table_usage, sum_usage(*parts), "evaluate")
    assert_row_sums(m, res.table_usage, 73)
    again = evaluate(m, batches, dev, inflight=1, table_usage=True)      # resets first; serial loop, torch metrics
    assert_usage_equal(again.table_usage, res.table_usage, "evaluate again")
    m.count_table_usage(False)


def test_constant_images_skew(small, dev):
    """Every pixel of an image equal (several grey levels): whole rows of lookups fall on one counter, the input that
    breaks a wrong duplicate merge."""
    m, luts = small
    levels = torch.tensor([-2.0, -0.7, -0.1, 0.0, 0.2, 0.9, 2.2, -2.0, 0.0, 2.2, 1.1, -1.3])
    x = levels.reshape(-1, 1, 1, 1).expand(-1, 3, 224, 224).contiguous().to(dev)
    got = check_against_oracle(m, luts, x, "constant images")
    name = m.spec.blocks[0].conv1.name
    assert (np.sort(got[name], axis=1)[:, -1] >= got[name].sum(axis=1) // 4).all()      # it is skewed: one entry holds >= 1/4
