"""GPU: care-set misses (ttnet_plan_set_care / _clear_care / ttnet_care_misses) and what they promise.

The expected rows come from the bit oracle (tests/_care_util.py): ``multihead_block_bits`` with ``taps`` runs from the
device's own ``features.3`` stage on the device's own tables, ``window_index`` gives the canonical index of every lookup,
the care bit is looked up and summed per image.  Every comparison is exact int32 or bitwise equality.

Covered images come from duplication: a care set is made from the lookups of some images, and the same images, at other
batch positions, stay inside it; random synthetic images almost never stay inside another image's care set."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from _care_util import expected_rows, lookup_indices, usage_of
from _util import args_for, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import _lib, minimise, synth, ttnet
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

CLASSES = {"small": ttnet.TT_vf_19lv3_imgnet_small, "xsmall": ttnet.TT_vf_19lv3_imgnet_xsmall}


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


def device_tables(m):
    return {b.name: m.get_table(b.name) for b in m.spec.block_tts()}


def images(first, n=1):
    return torch.from_numpy(synth.synth_images(n, first=first))


def mixed_batch():
    """[img5, img0, img6, img2, constant-0 image, img0]: with a care set made from images 0..3, positions 1, 3 and 5
    are covered and 0 and 2 are not."""
    return torch.cat([images(5), images(0), images(6), images(2), torch.zeros((1, 3, 224, 224)), images(0)])


def forward_rows(m, x, lane=0):
    with torch.no_grad():
        y = m(x, lane=lane)
    return y, m.care_misses(lane)


def care_from_images(m, luts, x):
    """The care set made of every entry the forward of ``x`` reads (from the oracle's indices of the device's stage)."""
    with torch.no_grad():
        m(x)
    return minimise.care_masks(usage_of(lookup_indices(m.read_stage("features.3", x.shape[0]), m.spec, luts), m.spec))


def oracle_rows(m, luts, n, masks):
    return expected_rows(lookup_indices(m.read_stage("features.3", n), m.spec, luts), m.spec, masks)


def assert_rows_equal(got, want, tag=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.int32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError(f"{tag}: {len(d)} of {want.size} row entries differ, first (image, block) {d[:6].tolist()}: got "
                             f"{[int(got[tuple(i)]) for i in d[:6]]}, want {[int(want[tuple(i)]) for i in d[:6]]}")


_SMALL = {}


@pytest.fixture
def small(dev):
    """TT-small p = 64 --layers 1 (built once, its tables read back once) with the care set of synthetic images 0..3
    installed: ``(model, tables, masks)``."""
    if "m" not in _SMALL:
        m = make_model(dev, reserve=64)
        luts = device_tables(m)
        _SMALL.update(m=m, luts=luts, masks=care_from_images(m, luts, images(0, 4).to(dev)))
    m = _SMALL["m"]
    m.set_lanes(1)
    m.set_care(_SMALL["masks"])
    return m, _SMALL["luts"], _SMALL["masks"]


def test_oracle_small_p64_covered_by_duplication(small, dev):
    m, luts, masks = small
    assert m.care_blocks == [b.name for b in m.spec.block_tts()] and len(m.care_blocks) == 12
    assert m._any_plan().query("care_blocks") == 12
    assert m._any_plan().query("care_bytes") == sum(a.nbytes for a in masks.values())
    x = mixed_batch().to(dev)
    _, rows = forward_rows(m, x)
    got = rows.cpu().numpy()
    assert_rows_equal(got, oracle_rows(m, luts, 6, masks), "small p=64")         # all 12 blocks, the float last one included
    assert not got[[1, 3, 5]].any()                                              # img0, img2, img0 again: covered
    assert (got[[0, 2]] != 0).any(axis=1).all()                                  # img5, img6: not
    assert np.array_equal(got[1], got[5])


def test_identities(small, dev):
    m, luts, masks = small
    x = images(20, 5).to(dev)
    lookups = np.array(list(m.care_lookups().values()), dtype=np.int64)
    ones = {b.name: np.full_like(masks[b.name], 0xFFFFFFFF) for b in m.spec.block_tts()}
    m.set_care(ones)
    assert not forward_rows(m, x)[1].cpu().numpy().any()
    zeros = {k: np.zeros_like(v) for k, v in masks.items()}
    m.set_care(zeros)
    got = forward_rows(m, x)[1].cpu().numpy()
    for blk in m.spec.blocks:                                                    # G * Ho * Wo of the block's own convolution
        for b in (blk.conv1, blk.conv2, blk.conv3):
            ho, wo = b.out_hw(*blk.in_hw)
            assert m.care_lookups()[b.name] == b.groups * ho * wo
        assert m.care_lookups()[blk.convf.name] == blk.convf.groups * blk.out_hw[0] * blk.out_hw[1]
    assert np.array_equal(got.astype(np.int64), np.broadcast_to(lookups, (5, 12)))
    removed = [m.care_blocks[1], m.care_blocks[6], m.care_blocks[11]]
    m.set_care({k: v for k, v in zeros.items() if k not in removed})             # a block without a bitmap gives 0
    got = forward_rows(m, x)[1].cpu().numpy()
    want = np.broadcast_to(lookups, (5, 12)).copy()
    want[:, [1, 6, 11]] = 0
    assert np.array_equal(got.astype(np.int64), want)
    # rows.sum(0)[b] == usage[b][~care].sum(), usage counted by the device on the same forward
    m.set_care(masks)
    m.count_table_usage(True)
    m.reset_table_usage()
    _, rows = forward_rows(m, x)
    m.add_table_usage(0)
    usage = m.table_usage()
    m.count_table_usage(False)
    total = rows.cpu().numpy().astype(np.int64).sum(axis=0)
    for col, b in enumerate(m.spec.block_tts()):
        keep = minimise.unpack_bits(masks[b.name], b.fan_in_bits)
        assert total[col] == usage[b.name][~keep].sum(), b.name
    assert total.sum() > 0


@pytest.mark.parametrize("variant,nfilter,tfilter,layers", [("small", 4, 8, 1), ("small", 8, 8, 0), ("small", 8, 8, 2),
                                                            ("xsmall", 8, 8, 1)])
def test_other_geometries(dev, variant, nfilter, tfilter, layers):
    """p = 32, --layers 0 and 2 (other block counts and strides), x-small (n = 4: bitmaps of one word per group)."""
    m = make_model(dev, variant, nfilter, tfilter, layers, reserve=8)
    luts = device_tables(m)
    x = torch.cat([images(0, 2), images(9), torch.zeros((1, 3, 224, 224)), images(1)]).to(dev)
    with torch.no_grad():
        m(x)
    idx = lookup_indices(m.read_stage("features.3", 5), m.spec, luts)            # one oracle pass serves both sides
    masks = minimise.care_masks(usage_of({k: v[:2] for k, v in idx.items()}, m.spec))          # what images 0 and 1 read
    m.set_care(masks)
    got = forward_rows(m, x)[1].cpu().numpy()
    assert_rows_equal(got, expected_rows(idx, m.spec, masks), f"{variant} p={nfilter * tfilter} l={layers}")
    assert not got[[0, 1, 4]].any()                                              # images 0, 1 and 1 again: covered
    if variant != "xsmall":                              # (16 entries per group: two images read nearly all of them)
        assert got[2].any()
    m.clear_care()


@pytest.mark.parametrize("n", [1, 37])
def test_batch_sizes(small, dev, n):
    """37 images: rows of 29 x 29 and 15 x 15 outputs, no multiple of the 64 lanes of a wave."""
    m, luts, masks = small
    x = images(11, n).to(dev)
    if n > 1:
        x[n // 2] = images(3)[0].to(dev)                                         # one covered image in the middle
    got = forward_rows(m, x)[1].cpu().numpy()
    assert_rows_equal(got, oracle_rows(m, luts, n, masks), f"n={n}")
    assert got[0].any() and (n == 1 or not got[n // 2].any())


def test_fused_path_batch_256_equals_four_64s(dev):
    m = make_model(dev, reserve=256)
    luts = _SMALL.get("luts") or device_tables(m)
    masks = _SMALL.get("masks") or care_from_images(m, luts, images(0, 4).to(dev))
    m.set_care(masks)
    x = images(0, 256).to(dev)
    whole = forward_rows(m, x)[1].cpu().numpy()
    parts = [forward_rows(m, x[i:i + 64])[1].cpu().numpy() for i in range(0, 256, 64)]
    assert_rows_equal(whole, np.concatenate(parts), "256 vs 4 x 64")
    assert not whole[:4].any() and whole[4:].any(axis=1).all()                   # images 0..3 made the care set
    m.clear_care()


def test_five_calls_and_graph_replay(small, dev):
    m, luts, masks = small
    x = mixed_batch().to(dev)
    first = forward_rows(m, x)[1].cpu().numpy()
    plan = m._any_plan()
    before = plan.query("graph_replays")
    for _ in range(5):
        assert_rows_equal(forward_rows(m, x)[1], first, "repeat")
    assert plan.query("graphs_enabled") == 1, _lib.load().ttnet_last_error()
    assert plan.query("graph_replays") > before
    with torch.no_grad():
        m(x)
    a, b = m.care_misses(0), m.care_misses(0)                                    # it zeroes the rows itself: no accumulation
    assert_rows_equal(a, first, "first of two calls")
    assert_rows_equal(b, first, "second of two calls")


def test_two_lanes_two_streams(small, dev):
    m, luts, masks = small
    xa, xb = mixed_batch().to(dev), torch.cat([images(2), images(40, 8)]).to(dev)
    alone = [forward_rows(m, x)[1].cpu().numpy() for x in (xa, xb)]
    torch.cuda.synchronize()
    m.set_lanes(2)
    assert m._any_plan().query("lanes") == 2
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
    got = []
    for rep in range(4):                                 # plain launches first, then replayed graphs per lane
        for lane, x in enumerate((xa, xb)):
            with torch.cuda.stream(streams[lane]):
                got.append((lane, forward_rows(m, x, lane)[1]))
    torch.cuda.synchronize()
    for lane, rows in got:
        assert_rows_equal(rows, alone[lane], f"lane {lane}")


def test_u8_and_stem_bits_entry_points(small, dev):
    m, luts, masks = small
    g = torch.Generator().manual_seed(5)
    x8 = torch.randint(0, 256, (6, 224, 224, 3), dtype=torch.uint8, generator=g).to(dev)
    with torch.no_grad():
        m.forward_u8(x8)
    rows = m.care_misses(0)
    assert_rows_equal(rows, oracle_rows(m, luts, 6, masks), "forward_u8")
    rng = np.random.default_rng(3)
    bits = (rng.random((5, m.spec.p, 56, 56)) < 0.3).astype(np.uint8)
    packed = OB.pack_rows(bits)
    with torch.no_grad():
        m.forward_from_stem_bits(torch.from_numpy(packed.view(np.int64)).to(dev))
    rows = m.care_misses(0)
    assert_rows_equal(rows, expected_rows(lookup_indices(packed, m.spec, luts), m.spec, masks), "from_stem_bits")
    assert rows.cpu().numpy().any()


def test_side_effects_logits_and_memory(dev):
    m = make_model(dev, reserve=16)
    plan = m._any_plan()
    before = {k: plan.query(k) for k in ("workspace_bytes", "care_bytes", "usage_bytes")}
    assert before["care_bytes"] == 0 and before["usage_bytes"] == 0
    x = images(70, 16).to(dev)
    with torch.no_grad():
        off = [m(x).clone() for _ in range(4)]
    luts = device_tables(m)
    masks = care_from_images(m, luts, x[:2])
    m.set_care(masks)
    assert plan.query("care_bytes") == sum(a.nbytes for a in masks.values())
    assert plan.query("usage_bytes") < 64 << 20                                  # the scratch, never the 543 MB of counters
    on = []
    for _ in range(4):
        y, rows = forward_rows(m, x)
        on.append(y.clone())
    torch.cuda.synchronize()
    for a, b in zip(off, on):
        assert torch.equal(a, b)
    assert rows.cpu().numpy()[2:].any()
    m.clear_care()
    assert {k: plan.query(k) for k in before} == before
    with torch.no_grad():
        assert torch.equal(m(x), off[0])
    # usage and care on together share the scratch: either may go first
    m.set_care(masks)
    m.count_table_usage(True)
    m.clear_care()
    m.reset_table_usage()
    with torch.no_grad():
        m(x)
    m.add_table_usage(0)
    assert all(v.sum() > 0 for v in m.table_usage().values())
    m.set_care(masks)
    m.count_table_usage(False)
    assert_rows_equal(forward_rows(m, x)[1], rows.cpu().numpy(), "after usage went")
    m.clear_care()
    assert {k: plan.query(k) for k in before} == before


def test_care_survives_a_plan_rebuild(dev):
    m = make_model(dev, reserve=4)
    luts = device_tables(m)
    masks = care_from_images(m, luts, images(0, 2).to(dev))
    m.set_care(masks)
    small_plan = m._any_plan()
    x = torch.cat([images(30, 5), images(1)]).to(dev)                            # 6 > 4: the plan is rebuilt
    _, rows = forward_rows(m, x)
    assert m._any_plan() is not small_plan
    got = rows.cpu().numpy()
    assert_rows_equal(got, oracle_rows(m, luts, 6, masks), "rebuilt plan")
    assert not got[5].any() and got[:5].any(axis=1).all()


def test_error_contract(dev):
    lib = _lib.load()
    m = make_model(dev, reserve=4)
    plan = m._any_plan()
    rows = torch.zeros((4, 12), dtype=torch.int32, device=dev)
    ptr = C.c_void_p(rows.data_ptr())
    name = b"features.4.Block_conv1"
    bits = np.zeros((64, 2048), dtype=np.uint32)                                 # 64 groups of 2^16 entries
    host = bits.ctypes.data_as(C.c_void_p)
    assert lib.ttnet_care_misses(plan.handle, 0, ptr, None) == -2                # TTNET_E_STATE: before any set_care
    assert lib.ttnet_plan_set_care(plan.handle, name, host, bits.nbytes - 4) == -1      # TTNET_E_INVALID: wrong bytes
    assert lib.ttnet_plan_set_care(plan.handle, b"features.9.Block_conv1", host, bits.nbytes) == -1
    assert lib.ttnet_care_misses(plan.handle, 0, ptr, None) == -2                # (the refused installs turned nothing on)
    assert lib.ttnet_plan_set_care(plan.handle, name, host, bits.nbytes) == 0
    assert lib.ttnet_care_misses(plan.handle, 3, ptr, None) == -1                # bad lane
    assert lib.ttnet_care_misses(plan.handle, 0, None, None) == -1
    assert lib.ttnet_care_misses(plan.handle, 0, C.c_void_p(rows.data_ptr() + 2), None) == -1
    assert lib.ttnet_care_misses(plan.handle, 0, ptr, None) == 0
    torch.cuda.synchronize()
    assert rows[0, 0].item() > 0 and not rows[:, 1:].any().item() and not rows[1:].any().item()
    m.set_lanes(2)
    assert lib.ttnet_care_misses(plan.handle, 1, ptr, None) == -2                # a lane without a forward
    assert lib.ttnet_plan_clear_care(plan.handle) == 0
    assert lib.ttnet_care_misses(plan.handle, 0, ptr, None) == -2
    with pytest.raises(KeyError):
        m.set_care({"features.9.Block_conv1": bits})
    with pytest.raises(ValueError, match="shape"):
        m.set_care({name.decode(): bits[:, :8]})
    spec, st = spec_and_state("full")
    f = ttnet.TT_vf_19lv3_imgnet(args_for("full"))
    f.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    f = f.to(dev).eval().reserve(2)
    with torch.no_grad():
        f(torch.from_numpy(synth.synth_images(1)).to(dev))
    assert lib.ttnet_plan_set_care(f._any_plan().handle, name, host, bits.nbytes) == -4          # TTNET_E_UNSUPPORTED
    assert "fan-in 30" in lib.ttnet_last_error().decode()
    spec, st = spec_and_state("valexnet")
    v = ttnet.TT_FHE_XSMALL_vAlexnet(args_for("valexnet"))
    v.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in st.items()}, strict=True)
    v = v.to(dev).eval().reserve(2)
    with torch.no_grad():
        v(torch.from_numpy(synth.synth_images(1, hw=(32, 32))).to(dev))
    b = spec.block_tts()[0]
    mask = np.zeros((b.groups, minimise.n_words(b.fan_in_bits)), dtype=np.uint32)
    with pytest.raises(_lib.TTNetError) as e:
        v.set_care({b.name: mask})
    assert e.value.status == -4 and "vAlexnet" in str(e.value)


def test_the_guarantee_any_completion_of_the_dont_cares(dev):
    """What the rows promise, on TT-small p = 32 --layers 1: every table entry outside the care set is replaced by the
    worst completion (bits complemented, the float last block + 1), and every covered image keeps its ``flatten`` row and
    its logits bit for bit, while the circuit as a whole is a different one."""
    m = make_model(dev, "small", 4, 8, 1, reserve=8)
    luts = device_tables(m)
    masks = care_from_images(m, luts, images(0, 4).to(dev))
    m.set_care(masks)
    x = mixed_batch().to(dev)
    y0, rows = forward_rows(m, x)
    y0, rows = y0.clone(), rows.cpu().numpy()
    flat0 = m.read_stage("flatten", 6)
    covered = ~rows.any(axis=1)
    assert covered[[1, 3, 5]].all() and not covered[[0, 2]].any()
    changed = 0
    for b in m.spec.block_tts():
        keep = minimise.unpack_bits(masks[b.name], b.fan_in_bits)                # bool [G, 2^n]
        worst = luts[b.name].copy()
        worst[~keep] = worst[~keep] + 1 if b.last else worst[~keep] ^ 1
        changed += int((~keep).sum())
        m.set_table(b.name, worst)
    assert changed > 0
    with torch.no_grad():
        y1 = m(x).clone()
    flat1 = m.read_stage("flatten", 6)
    assert np.array_equal(flat1[covered].view(np.uint32), flat0[covered].view(np.uint32))
    assert torch.equal(y1[torch.from_numpy(covered).to(dev)], y0[torch.from_numpy(covered).to(dev)])
    assert not np.array_equal(flat1[~covered].view(np.uint32), flat0[~covered].view(np.uint32))      # it is another circuit
    for b in m.spec.block_tts():
        m.set_table(b.name, luts[b.name])
    with torch.no_grad():
        assert torch.equal(m(x), y0)
    assert np.array_equal(m.read_stage("flatten", 6).view(np.uint32), flat0.view(np.uint32))


def test_evaluate_care_inflight_2_on_device_batches(dev):
    from scale_imagenet_amd.evaluate import care_bounds, evaluate
    m = make_model(dev, reserve=16)
    luts = device_tables(m)
    usage = usage_of(lookup_indices(care_stage(m, images(0, 4).to(dev)), m.spec, luts), m.spec)
    firsts, sizes = (0, 20, 2, 60, 80), (16, 16, 16, 16, 9)
    batches = [(images(f, n).to(dev), torch.from_numpy(synth.synth_targets(n, first=f)).to(dev)) for f, n in zip(firsts, sizes)]
    plain = evaluate(m, batches, dev, inflight=2, metrics="device")
    assert plain.care is None
    res = evaluate(m, batches, dev, inflight=2, metrics="device", care=usage, topk=5)
    assert (res.loss, res.top1, res.top5, res.images) == (plain.loss, plain.top1, plain.top5, 73)
    m.set_lanes(1)
    parts = [forward_rows(m, x)[1].cpu().numpy() for x, _ in batches]
    care = res.care
    assert care.blocks == m.care_blocks
    assert_rows_equal(care.rows, np.concatenate(parts), "evaluate")                   # dataset order
    assert care.covered[:4].all() and care.covered[32:34].all() and care.covered_images == 6      # images 0..3 and 2, 3 again
    t = np.concatenate([synth.synth_targets(n, first=f) for f, n in zip(firsts, sizes)])
    hit1 = res.predictions.classes[:, 0] == t
    hit5 = (res.predictions.classes[:, :5] == t[:, None]).any(axis=1)
    assert care.top1_bounds == care_bounds(care.covered, hit1) and care.top5_bounds == care_bounds(care.covered, hit5)
    assert care.top1_bounds[0] <= res.top1 <= care.top1_bounds[1]
    serial = evaluate(m, batches, dev, inflight=1, care=minimise.care_masks(usage))   # bitmaps instead of counts; torch metrics
    assert serial.predictions is None
    assert_rows_equal(serial.care.rows, care.rows, "evaluate again")
    assert serial.care.top1_bounds == care.top1_bounds
    m.clear_care()


def care_stage(m, x):
    with torch.no_grad():
        m(x)
    return m.read_stage("features.3", x.shape[0])
