"""GPU: progressive (SOF2) JPEG decoding of ragged batches (pack_jpeg(..., progressive=True), kind 2 of
ttnet_jpeg_decode_ragged) against what Pillow decodes (tests/golden/ref_jpeg_progressive.json and its arrays, from
tools/gen_jpeg_progressive_fixture.py): every fixture byte for byte, mixed batches, the same logits as the Pillow
fallback, containment of corrupt scans, graph replay, lanes and the reservation.  Reads only tests/golden."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

from _util import (args_for, jpeg_arrays, jpeg_bytes as _sbytes, jpeg_diff, jpeg_fixture, ragged_images as _images, sha,
                   spec_and_state)
from scale_imagenet_amd import _lib, jpeg as J, preprocess, ttnet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


PROG = jpeg_fixture(progressive=True)
SEQ = [e for e in jpeg_fixture() if e["device"]]
_pbytes, _arrays, _diff = (partial(f, progressive=True) for f in (_sbytes, jpeg_arrays, jpeg_diff))


@pytest.mark.parametrize("e", PROG, ids=lambda e: e["name"])
def test_every_progressive_fixture_is_pillow_byte_identical(e):
    rj = J.pack_jpeg([_pbytes(e["name"])], progressive=True)
    assert rj.descriptors()[0]["kind"] == J.KIND_PROGRESSIVE
    got = _images(J.decode_ragged(rj.to(DEV)))[0]
    assert got.shape == (e["h"], e["w"], 3)
    assert sha(got) == e["sha256"], _diff(e["name"], got)
    assert J.jpeg_counters(DEV) == (0, 0)          # not corrupt, and nothing counted as a sequential-fallback segment


def test_ragged_batch_mixing_progressive_sequential_raw_and_repeats():
    raw = np.arange(9 * 11 * 3, dtype=np.uint8).reshape(9, 11, 3)
    entries = [("p", e) for e in PROG] + [("s", e) for e in SEQ[::2]] + [("r", None)]
    entries += [("p", e) for e in PROG if "500" in e["name"] or "rst" in e["name"]]
    perm = np.random.default_rng(11).permutation(len(entries))
    entries = [entries[p] for p in perm]
    items = [raw if k == "r" else (_pbytes(e["name"]) if k == "p" else _sbytes(e["name"])) for k, e in entries]
    rj = J.pack_jpeg(items, progressive=True).to(DEV)
    kinds = rj.descriptors()["kind"].tolist()
    assert kinds == [{"p": 2, "s": 0, "r": 1}[k] for k, _ in entries]
    a = _images(J.decode_ragged(rj))
    b = _images(J.decode_ragged(rj))
    for (k, e), x, y in zip(entries, a, b):
        if k == "r":
            assert np.array_equal(x, raw)
        else:
            assert sha(x) == e["sha256"], (k, e["name"])
        assert np.array_equal(x, y)
    J.check_jpeg(DEV)


def test_flag_on_and_off_give_the_same_bytes_and_logits():
    """progressive=False ships Pillow's pixels (here: the fixture's arrays as raw items, what the fallback packs);
    progressive=True decodes the same files on the device."""
    arr = _arrays()
    names = [e["name"] for e in PROG if e["name"] in arr and e["h"] * e["w"] >= 40 * 20]
    assert len(names) >= 5
    off = J.pack_jpeg([arr[n] for n in names]).to(DEV)
    on = J.pack_jpeg([_pbytes(n) for n in names], progressive=True).to(DEV)
    assert set(off.descriptors()["kind"].tolist()) == {1} and set(on.descriptors()["kind"].tolist()) == {2}
    assert off.out_bytes == on.out_bytes
    assert torch.equal(J.decode_ragged(off).data[:off.out_bytes].cpu(), J.decode_ragged(on).data[:on.out_bytes].cpu())
    spec, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(DEV).eval().reserve(64)
    with torch.no_grad():
        assert torch.equal(J.jpeg_eval_forward(model, off).cpu(), J.jpeg_eval_forward(model, on).cpu())
    J.check_jpeg(DEV)


MID = "p420_rst_rows1_203x120"


def _repack_with_damage(data, fn):
    """Pack `data` for the device, then let fn(payload bytearray, scan records, header) damage the packed payload:
    the scan list stays that of the complete file, as when the damage happened after the header walk."""
    hd = J.parse_progressive(data)
    rj = J.pack_jpeg([data], progressive=True)
    d = rj.descriptors()[0]
    o, n = int(d["data_offset"]), int(d["data_bytes"])
    flat = rj.data.numpy()
    pay = bytearray(flat[o:o + n].tobytes())
    base = hd.scans[0].data_start
    fn(pay, [(s.data_start - base, s.data_end - base) for s in hd.scans], hd)
    assert len(pay) == n
    flat[o:o + n] = np.frombuffer(bytes(pay), dtype=np.uint8)
    return rj


def _batch_with(damaged: J.RaggedJpeg, canary=4096):
    """[good, damaged, good] decoded in one call with a canary region behind dst; returns (images, canary ok)."""
    good = [_pbytes("p444_q90_64x48"), _pbytes("pgrey_rst_blocks1_50x30")]
    g0, g1 = (J.pack_jpeg([g], progressive=True) for g in good)
    # concatenate the three packed batches by hand: offsets shifted
    parts, descs, size, out, blocks = [], [], 0, 0, 0
    for rj in (g0, damaged, g1):
        d = rj.descriptors().copy()
        d["data_offset"] += size
        d["table_offset"] += size
        d["out_offset"] += out
        d["block_offset"] += blocks
        parts.append(rj.data)
        descs.append(d)
        size += rj.data.numel()
        out += rj.out_bytes
        blocks += rj.n_blocks
    desc = np.concatenate(descs)
    rj = J.RaggedJpeg(torch.cat(parts), torch.from_numpy(desc.view(np.int64).reshape(len(desc), -1).copy()), blocks, out,
                      int(desc["h"].max()), int(desc["w"].max())).to(DEV)
    ctx = J._context(DEV, 3)
    ctx.reserve(len(rj), rj.n_blocks, rj.data.numel())
    dst = torch.full((J._align16(out) + canary,), 0xA5, dtype=torch.uint8, device=DEV)
    od = torch.empty((len(rj), 2), dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().ttnet_jpeg_decode_ragged(
        ctx.h, C.c_void_p(rj.data.data_ptr()), rj.data.numel(), C.c_void_p(rj.desc.data_ptr()), len(rj), rj.n_blocks,
        C.c_void_p(dst.data_ptr()), out, C.c_void_p(od.data_ptr()), C.c_void_p(ctx.stats.data_ptr()), None))
    torch.cuda.synchronize(DEV)
    h = dst.cpu().numpy()
    ims = [h[int(d["out_offset"]):int(d["out_offset"]) + int(d["h"]) * int(d["w"]) * 3].reshape(int(d["h"]), int(d["w"]), 3)
           for d in desc]
    return ims, bool((h[out:] == 0xA5).all())


def _good_refs():
    by = {e["name"]: e for e in PROG}
    return by["p444_q90_64x48"]["sha256"], by["pgrey_rst_blocks1_50x30"]["sha256"]


def _check_contained(damaged, must_be_corrupt):
    J.jpeg_counters(DEV)
    ims, canary_ok = _batch_with(damaged)
    bad, _ = J.jpeg_counters(DEV)
    r0, r2 = _good_refs()
    assert canary_ok
    assert sha(ims[0]) == r0 and sha(ims[2]) == r2          # the neighbours are untouched
    assert bad in (0, 1)
    if bad:
        assert not ims[1].any()
    if must_be_corrupt:
        assert bad == 1
    return bad


@pytest.mark.parametrize("k", range(10))
def test_scan_cut_short_is_contained_and_counted(k):
    """Scan k loses the second half of its data (overwritten by what a reader meets at the end of a scan: a marker)."""
    def cut(pay, spans, hd):
        lo, hi = spans[k]
        mid = lo + max(1, (hi - lo) // 2)
        pay[mid:hi] = b"\xff\xd9" * ((hi - mid) // 2) + b"\xff" * ((hi - mid) % 2)
    data = _pbytes(MID)
    assert len(J.parse_progressive(data).scans) == 10
    # a DC refinement of few blocks may still find its bits in the first half: every other scan must run out of data
    bad = _check_contained(_repack_with_damage(data, cut), must_be_corrupt=False)
    hd = J.parse_progressive(data)
    if not (hd.scans[k].ss == 0 and hd.scans[k].ah):
        assert bad == 1


def test_flipped_entropy_bytes_are_contained():
    rng = np.random.default_rng(23)
    total = 0
    for trial in range(6):
        def flip(pay, spans, hd):
            lo, hi = spans[int(rng.integers(0, len(spans)))]
            for p in rng.integers(lo, hi, size=3):
                v = pay[p] ^ int(rng.integers(1, 255))
                if v in (0xFF, 0x00) or pay[p] in (0xFF, 0x00) or (p > 0 and pay[p - 1] == 0xFF) or (0xD0 <= v <= 0xD7):
                    continue                          # would make or break a marker
                pay[p] = v
        total += _check_contained(_repack_with_damage(_pbytes(MID), flip), must_be_corrupt=False)
    J.jpeg_counters(DEV)


def test_renumbered_restart_marker_is_corrupt():
    def renumber(pay, spans, hd):
        lo, hi = spans[1]
        k = bytes(pay).find(b"\xff\xd1", lo, hi)
        assert k >= 0
        pay[k + 1] = 0xD5
    assert _check_contained(_repack_with_damage(_pbytes(MID), renumber), must_be_corrupt=True) == 1
    with pytest.raises(RuntimeError, match="corrupt"):
        J.decode_ragged(_repack_with_damage(_pbytes(MID), renumber).to(DEV))
        J.check_jpeg(DEV)


def _mixed(order):
    names_p = ["p420_q90_64x48", "p444_rst_rows1_90x70", "pgrey_q90_61x47", "p422_q90_33x31", "p420_q5_96x72"]
    names_s = ["s420_q90_64x48", "grey_q90_61x47", "s444_rst_rows1_90x70"]
    ents = [("p", n) for n in names_p] + [("s", n) for n in names_s]
    ents = [ents[i] for i in order]
    sh = {e["name"]: e for e in PROG + SEQ}
    return [(_pbytes(n) if k == "p" else _sbytes(n)) for k, n in ents], [sh[n] for _, n in ents]


def test_graph_capture_replays_with_another_mixed_batch():
    i1, e1 = _mixed(range(8))
    i2, e2 = _mixed([7, 0, 6, 1, 5, 2, 4, 3])
    b1, b2 = J.pack_jpeg(i1, progressive=True), J.pack_jpeg(i2, progressive=True)
    lane = 9                                         # (a captured lane keeps its workspace for good)
    size = max(b1.data.numel(), b2.data.numel())
    J.reserve_jpeg(DEV, 16, 2 * max(b1.n_blocks, b2.n_blocks), 2 * size, lane=lane)
    data = torch.zeros(size, dtype=torch.uint8, device=DEV)
    desc = torch.zeros_like(b1.desc, device=DEV)

    def load(b):
        data.zero_()
        data[: b.data.numel()].copy_(b.data.to(DEV))
        desc.copy_(b.desc.to(DEV))
    static = J.RaggedJpeg(data, desc, max(b1.n_blocks, b2.n_blocks), max(b1.out_bytes, b2.out_bytes), 8192, 8192)
    load(b1)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        J.decode_ragged(static, lane=lane)           # warm-up outside capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = J.decode_ragged(static, lane=lane)
    for b, ents in ((b1, e1), (b2, e2), (b1, e1)):
        load(b)
        g.replay()
        torch.cuda.synchronize(DEV)
        data_h = out.data.cpu().numpy()
        for e, d in zip(ents, b.descriptors()):
            o = int(d["out_offset"])
            assert sha(data_h[o:o + e["h"] * e["w"] * 3]) == e["sha256"], e["name"]
    J.check_jpeg(DEV)
    big = J.pack_jpeg([_pbytes("p420_q90_600x560")] * 3, progressive=True).to(DEV)
    with pytest.raises(RuntimeError, match="captured graph"):
        J.decode_ragged(big, lane=lane)              # a captured lane is never regrown


def test_two_lanes_on_two_streams():
    i1, _ = _mixed(range(8))
    i2, _ = _mixed([7, 0, 6, 1, 5, 2, 4, 3])
    b1 = J.pack_jpeg(i1 + [_pbytes("p420_q90_500x375_a")], progressive=True).to(DEV)
    b2 = J.pack_jpeg([_pbytes("p420_q90_375x500_c")] + i2, progressive=True).to(DEV)
    n1, n2 = b1.out_bytes, b2.out_bytes             # (the output buffer is padded to 16 bytes: compare the images)
    ref1, ref2 = J.decode_ragged(b1).data[:n1].cpu(), J.decode_ragged(b2).data[:n2].cpu()
    torch.cuda.synchronize(DEV)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    s1.wait_stream(torch.cuda.current_stream(DEV))
    s2.wait_stream(torch.cuda.current_stream(DEV))
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            o1 = J.decode_ragged(b1, lane=0)
        with torch.cuda.stream(s2):
            o2 = J.decode_ragged(b2, lane=1)
        outs.append((o1, o2))
    torch.cuda.synchronize(DEV)
    for o1, o2 in outs:
        assert torch.equal(o1.data[:n1].cpu(), ref1) and torch.equal(o2.data[:n2].cpu(), ref2)
    J.check_jpeg(DEV)


def test_decode_past_the_reservation_is_invalid():
    rj = J.pack_jpeg(_mixed(range(8))[0], progressive=True).to(DEV)
    J.decode_ragged(rj)
    ctx = J._context(DEV)
    out = torch.empty(rj.out_bytes + 16, dtype=torch.uint8, device=DEV)
    od = torch.empty((len(rj), 2), dtype=torch.int64, device=DEV)
    lib = _lib.load()
    st = lib.ttnet_jpeg_decode_ragged(ctx.h, C.c_void_p(rj.data.data_ptr()), rj.data.numel(), C.c_void_p(rj.desc.data_ptr()),
                                      len(rj), ctx.res[1] + 1, C.c_void_p(out.data_ptr()), out.numel(),
                                      C.c_void_p(od.data_ptr()), C.c_void_p(ctx.stats.data_ptr()), None)
    assert st == -1 and "reservation" in lib.ttnet_last_error().decode()   # TTNET_E_INVALID
    J.check_jpeg(DEV)
