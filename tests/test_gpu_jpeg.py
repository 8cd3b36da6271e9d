"""GPU: JPEG decoding of ragged batches (ttnet_jpeg_decode_ragged, scale_imagenet_amd/jpeg.py) against what Pillow
decodes (tests/golden/ref_jpeg.json, ref_jpeg_arrays.npz, from tools/gen_jpeg_fixture.py); batches, corrupt data,
graph replay, lanes, the reservation, and the eval forward from file bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from _util import (args_for, decode_images, jpeg_arrays as _arrays, jpeg_bytes as _bytes, jpeg_diff as _diff,
                   jpeg_fixture as _fixture, ragged_images as _images, sha, spec_and_state)
from scale_imagenet_amd import _lib, jpeg as J, preprocess, ttnet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


DEVICE_FIX = [e for e in _fixture() if e["device"]]
FALLBACK_FIX = [e for e in _fixture() if not e["device"]]


def _items(entries):
    """Packable items: the file bytes of device-decoded fixtures, Pillow's arrays for the fallback ones (no Pillow on
    the GPU machine is needed)."""
    arr = _arrays()
    return [(_bytes(e["name"]) if e["device"] else arr[e["name"]]) for e in entries]


@pytest.mark.parametrize("e", DEVICE_FIX, ids=lambda e: e["name"])
def test_every_device_fixture_is_pillow_byte_identical(e):
    rj = J.pack_jpeg([_bytes(e["name"])])
    assert rj.descriptors()[0]["kind"] == J.KIND_JPEG
    got = _images(J.decode_ragged(rj.to(DEV)))[0]
    assert got.shape == (e["h"], e["w"], 3)
    assert sha(got) == e["sha256"], _diff(e["name"], got)
    assert J.jpeg_counters(DEV)[0] == 0


def test_ragged_batch_shuffled_with_fallback_entries_and_repeats():
    entries = list(_fixture()) + [e for e in DEVICE_FIX if "500" in e["name"] or "rst" in e["name"]] * 2
    perm = np.random.default_rng(5).permutation(len(entries))
    entries = [entries[p] for p in perm]
    rj = J.pack_jpeg(_items(entries)).to(DEV)
    a = _images(J.decode_ragged(rj))
    b = _images(J.decode_ragged(rj))
    for e, x, y in zip(entries, a, b):
        assert sha(x) == e["sha256"], _diff(e["name"], x)
        assert np.array_equal(x, y)
    J.check_jpeg(DEV)


def test_sequential_switch_gives_the_same_bytes(monkeypatch):
    rj = J.pack_jpeg(_items(DEVICE_FIX)).to(DEV)
    par = J.decode_ragged(rj).data.cpu()
    bad, nseq_par = J.jpeg_counters(DEV)
    nseg = sum(J.parse_header(_bytes(e["name"])).segments() for e in DEVICE_FIX)
    assert bad == 0 and nseq_par < nseg // 4, (nseq_par, nseg)     # the subsequences settle almost everywhere
    monkeypatch.setenv("TTNET_JPEG_SEQUENTIAL", "1")
    seq = J.decode_ragged(rj).data.cpu()
    bad, nseq = J.jpeg_counters(DEV)
    assert bad == 0 and nseq == nseg
    assert torch.equal(par, seq)


def _scan_span(data):
    hd = J.parse_header(data)
    return hd.scan_offset, len(data)


def test_corrupt_images_are_contained_and_counted():
    good = [_bytes(e["name"]) for e in DEVICE_FIX if e["name"] in ("s420_q90_500x375_a", "s444_q90_64x48",
                                                                   "s420_rst_blocks3_100x75", "grey_q90_61x47")]
    trunc = bytearray(_bytes("s420_q90_500x375_b"))
    s0, n = _scan_span(trunc)
    trunc = bytes(trunc[: s0 + (n - s0) // 2])                                       # truncated scan
    flip = bytearray(_bytes("s420_q100_96x72"))
    s0, n = _scan_span(flip)
    for p in range(s0 + 40, n - 2, 97):                                               # garbage in the scan
        flip[p] = (flip[p] ^ 0x5A) if flip[p] not in (0xFF, 0x00) and flip[p - 1] != 0xFF else flip[p]
    rst = bytearray(_bytes("s420_rst_blocks3_100x75"))
    k = rst.find(b"\xff\xd1")
    rst[k + 1] = 0xD5                                                                # misnumbered restart marker
    items = [good[0], bytes(trunc), good[1], bytes(flip), good[2], bytes(rst), good[3]]
    got = _images(J.decode_ragged(J.pack_jpeg(items).to(DEV)))
    bad, _ = J.jpeg_counters(DEV)
    assert bad == 3
    for i in (1, 3, 5):
        assert not got[i].any(), i
    ref = _images(J.decode_ragged(J.pack_jpeg(good).to(DEV)))
    for g, r in zip([got[0], got[2], got[4], got[6]], ref):
        assert np.array_equal(g, r)
    J.check_jpeg(DEV)
    with pytest.raises(RuntimeError, match="corrupt"):
        J.decode_ragged(J.pack_jpeg([bytes(trunc)]).to(DEV))
        J.check_jpeg(DEV)


def test_graph_capture_replays_with_a_new_batch():
    b1 = J.pack_jpeg(_items(DEVICE_FIX[:10]))
    b2 = J.pack_jpeg(_items(list(reversed(DEVICE_FIX[:10]))))
    lane = 5                                         # (a captured lane keeps its workspace for good)
    J.reserve_jpeg(DEV, 64, 4 * max(b1.n_blocks, b2.n_blocks), 4 * max(b1.data.numel(), b2.data.numel()), lane=lane)
    size = max(b1.data.numel(), b2.data.numel())
    data = torch.zeros(size, dtype=torch.uint8, device=DEV)
    desc = torch.zeros_like(b1.desc, device=DEV)

    def load(b):
        data.zero_()
        data[: b.data.numel()].copy_(b.data.to(DEV))
        desc.copy_(b.desc.to(DEV))
    out_bytes = max(b1.out_bytes, b2.out_bytes)
    static = J.RaggedJpeg(data, desc, max(b1.n_blocks, b2.n_blocks), out_bytes, 8192, 8192)
    load(b1)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        J.decode_ragged(static, lane=lane)           # warm-up outside capture
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = J.decode_ragged(static, lane=lane)
    for b, entries in ((b1, DEVICE_FIX[:10]), (b2, list(reversed(DEVICE_FIX[:10])))):
        load(b)
        g.replay()
        torch.cuda.synchronize(DEV)
        data_h, dd = out.data.cpu().numpy(), b.descriptors()
        for e, d in zip(entries, dd):
            o = int(d["out_offset"])
            x = data_h[o:o + e["h"] * e["w"] * 3].reshape(e["h"], e["w"], 3)
            assert sha(x) == e["sha256"], e["name"]
    J.check_jpeg(DEV)


def test_two_lanes_on_two_streams():
    b1 = J.pack_jpeg(_items(DEVICE_FIX)).to(DEV)
    b2 = J.pack_jpeg(_items(list(reversed(DEVICE_FIX)))).to(DEV)
    ref1, ref2 = J.decode_ragged(b1).data.cpu(), J.decode_ragged(b2).data.cpu()
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
        assert torch.equal(o1.data.cpu(), ref1) and torch.equal(o2.data.cpu(), ref2)
    J.check_jpeg(DEV)


def test_decode_past_the_reservation_is_invalid():
    rj = J.pack_jpeg(_items(DEVICE_FIX[:4])).to(DEV)
    J.decode_ragged(rj)
    ctx = J._context(DEV)
    out = torch.empty(rj.out_bytes + 16, dtype=torch.uint8, device=DEV)
    od = torch.empty((len(rj), 2), dtype=torch.int64, device=DEV)
    lib = _lib.load()
    st = lib.ttnet_jpeg_decode_ragged(ctx.h, C.c_void_p(rj.data.data_ptr()), rj.data.numel(), C.c_void_p(rj.desc.data_ptr()),
                                      len(rj), ctx.res[1] + 1, C.c_void_p(out.data_ptr()), out.numel(),
                                      C.c_void_p(od.data_ptr()), C.c_void_p(ctx.stats.data_ptr()), None)
    assert st == -1 and "reservation" in lib.ttnet_last_error().decode()
    st = lib.ttnet_jpeg_decode_ragged(ctx.h, C.c_void_p(rj.data.data_ptr()), ctx.res[2] + 16, C.c_void_p(rj.desc.data_ptr()),
                                      len(rj), rj.n_blocks, C.c_void_p(out.data_ptr()), out.numel(),
                                      C.c_void_p(od.data_ptr()), C.c_void_p(ctx.stats.data_ptr()), None)
    assert st == -1


def test_eval_forward_from_file_bytes_matches_pillow_decoded_path():
    spec, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(DEV).eval().reserve(64)
    big = [e for e in DEVICE_FIX if "500" in e["name"]]
    entries = big + [e for e in _fixture() if e["h"] * e["w"] >= 64 * 48][:8] + big
    arr = _arrays()
    pil = []
    for e in entries:
        if e["name"] in arr:
            pil.append(arr[e["name"]])
        else:
            x = _images(J.decode_ragged(J.pack_jpeg([_bytes(e["name"])]).to(DEV)))[0]
            assert sha(x) == e["sha256"]
            pil.append(x)
    with torch.no_grad():
        want = preprocess.imgnet_eval_forward(model, preprocess.pack_u8(pil).to(DEV)).cpu()
        got = J.jpeg_eval_forward(model, J.pack_jpeg(_items(entries)).to(DEV)).cpu()
    assert torch.equal(got, want)
    J.check_jpeg(DEV)


def _fill_before_eoi(data, last_ff):
    """The file with 0xFF fill bytes before its EOI so that the marker's FF is byte `last_ff` of the entropy-coded
    data (fill bytes before a marker are legal; Pillow decodes the same image)."""
    assert data[-2:] == b"\xff\xd9"
    s0 = J.parse_header(data).scan_offset
    n = last_ff + 2 - (len(data) - s0)
    assert n >= 0
    return data[:-2] + b"\xff" * n + b"\xff\xd9"


def test_marker_at_the_end_of_a_destuff_chunk():
    """The de-stuff kernel works in chunks of 1024 bytes; an end marker whose FF is a chunk's last byte is found by the
    next chunk's first thread, so the scan's end changes while other waves are still in the loop."""
    e = next(e for e in DEVICE_FIX if e["name"] == "s444_q90_64x48")
    base = _bytes(e["name"])
    items = [_fill_before_eoi(base, last) for last in (6143, 6144, 7167)] + [base]
    for x in decode_images(items * 8, DEV):
        assert sha(x) == e["sha256"]
    J.check_jpeg(DEV)


def test_a_captured_lane_is_not_regrown():
    small = J.pack_jpeg(_items(DEVICE_FIX[:3])).to(DEV)
    big = J.pack_jpeg(_items(DEVICE_FIX)).to(DEV)
    lane = 7
    J.reserve_jpeg(DEV, 8, small.n_blocks, small.data.numel(), lane=lane)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        J.decode_ragged(small, lane=lane)
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        J.decode_ragged(small, lane=lane)
    with pytest.raises(RuntimeError, match="captured graph"):
        J.decode_ragged(big, lane=lane)
    g.replay()
    torch.cuda.synchronize(DEV)
    J.decode_ragged(big, lane=lane + 1)
    J.check_jpeg(DEV)
