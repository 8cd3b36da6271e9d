"""CPU: the walk over every scan of a progressive file (scale_imagenet_amd/jpeg.py parse_progressive) against the
committed fixtures, the unchanged defaults, pack_jpeg's kind-2 layout, the refusals and malformed input."""
import io
from functools import partial

import numpy as np
import pytest

from _util import jpeg_bytes as _seq_bytes, jpeg_fixture
from scale_imagenet_amd import jpeg as J

_bytes = partial(_seq_bytes, progressive=True)


# libjpeg's default progressive script (jcparam.c jpeg_simple_progression), as (components, Ss, Se, Ah, Al)
COLOUR_SCRIPT = [([0, 1, 2], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([2], 1, 63, 0, 1), ([1], 1, 63, 0, 1), ([0], 6, 63, 0, 2),
                 ([0], 1, 63, 2, 1), ([0, 1, 2], 0, 0, 1, 0), ([2], 1, 63, 1, 0), ([1], 1, 63, 1, 0), ([0], 1, 63, 1, 0)]
GREY_SCRIPT = [([0], 0, 0, 0, 1), ([0], 1, 5, 0, 2), ([0], 6, 63, 0, 2), ([0], 1, 63, 2, 1), ([0], 0, 0, 1, 0),
               ([0], 1, 63, 1, 0)]


@pytest.mark.parametrize("e", jpeg_fixture(progressive=True), ids=lambda e: e["name"])
def test_parser_reproduces_fixture_scan_list(e):
    data = _bytes(e["name"])
    hd = J.parse_progressive(data)
    assert isinstance(hd, J.ProgressiveHeader), getattr(hd, "reason", None)
    assert (hd.h, hd.w) == (e["h"], e["w"]) and [list(s) for s in hd.sampling] == e["sampling"]
    got = [(s.comps, s.ss, s.se, s.ah, s.al) for s in hd.scans]
    assert got == (GREY_SCRIPT if hd.ncomp == 1 else COLOUR_SCRIPT) and len(got) == e["n_scans"]
    assert got == [(s["comps"], s["ss"], s["se"], s["ah"], s["al"]) for s in e["scans"]]
    # (with restart_marker_rows libjpeg writes a new DRI in front of a scan whose row has another block count)
    assert [s.restart_interval for s in hd.scans] == [s["restart_interval"] for s in e["scans"]]
    assert hd.restart_interval == hd.scans[0].restart_interval == e["restart_interval"]
    assert ("rst" in e["name"]) == (e["restart_interval"] > 0)
    # the data ranges tile the file: each starts right behind its SOS header and runs to the next marker, which is a
    # DHT or SOS of the next scan (or EOI); nothing but marker segments lies between two scans
    for k, s in enumerate(hd.scans):
        ns = len(s.comps)
        sos = s.data_start - (2 + 6 + 2 * ns)
        assert data[sos:sos + 2] == b"\xff\xda" and int.from_bytes(data[sos + 2:sos + 4], "big") == 6 + 2 * ns
        assert 0 < s.data_start < s.data_end <= len(data)
        assert data[s.data_end] == 0xFF and data[s.data_end + 1] in ((0xC4, 0xDA, 0xDD) if k + 1 < len(hd.scans) else (0xD9,))
        body = data[s.data_start:s.data_end]
        i = body.find(b"\xff")
        while i >= 0:
            assert i + 1 < len(body) and (body[i + 1] == 0 or 0xD0 <= body[i + 1] <= 0xD7), (k, i)
            i = body.find(b"\xff", i + 2)
        if k + 1 < len(hd.scans):
            p = s.data_end
            while data[p + 1] != 0xDA:
                p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
            assert p + 2 + int.from_bytes(data[p + 2:p + 4], "big") == hd.scans[k + 1].data_start
    assert hd.scans[-1].data_end == len(data) - 2
    # the schedule: a scan runs in a later round than the scans it refines, at most four per round, slots distinct
    slots = [s.slot for s in hd.scans]
    assert len(set(slots)) == len(slots) and max(slots) // 4 + 1 == hd.rounds <= len(slots)
    for j, s in enumerate(hd.scans):
        for t in hd.scans[:j]:
            if set(s.comps) & set(t.comps) and s.ss <= t.se and t.ss <= s.se:
                assert t.slot // 4 < s.slot // 4


def _sequential_twin(data):
    """The same frame encoded sequentially (Pillow, when it is there): the block count must agree."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    b = io.BytesIO()
    im.save(b, "JPEG", quality="keep", subsampling="keep")
    return b.getvalue()


def test_defaults_are_unchanged_and_the_flag_packs_kind_2():
    names = ["p420_q90_64x48", "pgrey_q90_61x47", "p444_rst_rows1_90x70", "p422_q90_15x17", "p420_q90_600x560"]
    files = [_bytes(n) for n in names]
    for f in files:
        hd = J.parse_header(f)
        assert isinstance(hd, J.Unsupported) and "progressive" in hd.reason
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    if have_pil:
        off = J.pack_jpeg(files[:2])
        assert off.descriptors()["kind"].tolist() == [J.KIND_RAW] * 2 and all("progressive" in r for r in off.reasons)
        assert off.n_blocks == 0
        rj, _ = J.collate_jpeg([(files[0], 3)])
        assert rj.descriptors()[0]["kind"] == J.KIND_RAW
    raw = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    seq = _seq_bytes("s420_q90_64x48")
    rj = J.pack_jpeg(files + [raw, seq], progressive=True)
    d = rj.descriptors()
    flat = rj.data.numpy()
    assert J.KIND_PROGRESSIVE == 2 and d.dtype.itemsize == 80 and rj.desc.shape == (7, 10)
    assert d["kind"].tolist() == [2] * 5 + [J.KIND_RAW, J.KIND_JPEG]
    assert rj.reasons == [None] * 5 + ["already decoded", None]
    assert rj.data.numel() % 16 == 0
    out = blocks = 0
    for i, f in enumerate(files):
        hd = J.parse_progressive(f)
        assert d[i]["table_offset"] % 16 == 0 and d[i]["data_offset"] % 16 == 0
        ns, nr, nt = d[i]["reserved"][0] & 255, (d[i]["reserved"][0] >> 8) & 255, (d[i]["reserved"][0] >> 16) & 255
        assert (ns, nr) == (len(hd.scans), hd.rounds) and ns <= J.MAX_SCANS and d[i]["reserved"][1] == J.SCAN_OFF
        assert d[i]["data_offset"] == d[i]["table_offset"] + J.TABLE_BYTES + 272 * nt
        t, o = int(d[i]["table_offset"]), int(d[i]["data_offset"])
        q = flat[t:t + 384].view("<u2").reshape(3, 64)
        for k, c in enumerate(hd.comps):
            assert list(q[k]) == hd.qt[c[3]]
        base = hd.scans[0].data_start
        assert flat[o:o + d[i]["data_bytes"]].tobytes() == f[base:hd.scans[-1].data_end]
        recs = flat[t + J.SCAN_OFF:t + J.SCAN_OFF + 32 * ns].view(J.JSCAN_DTYPE)
        for r, s in zip(recs, hd.scans):
            assert (r["ss"], r["se"], r["ah"], r["al"], r["ncomp"], r["slot"], r["restart_interval"]) == \
                (s.ss, s.se, s.ah, s.al, len(s.comps), s.slot, s.restart_interval)
            assert list(r["comp"][:len(s.comps)]) == s.comps
            lo = o + int(r["data_offset"])
            assert flat[lo:lo + int(r["data_bytes"])].tobytes() == f[s.data_start:s.data_end]
            for k, tab in enumerate(s.tables):
                if tab is not None:
                    assert r["table"][k] < nt
                    p = t + J.TABLE_BYTES + 272 * int(r["table"][k])
                    assert list(flat[p:p + 16]) == tab[0] and list(flat[p + 16:p + 16 + len(tab[1])]) == tab[1]
        assert (d[i]["h"], d[i]["w"], d[i]["ncomp"]) == (hd.h, hd.w, hd.ncomp)
        assert d[i]["block_offset"] == blocks and d[i]["out_offset"] == out
        mx, my, b = hd.mcus()
        assert hd.blocks() == mx * my * b
        if have_pil:
            twin = J.parse_header(_sequential_twin(f))
            assert isinstance(twin, J.JpegHeader) and twin.blocks() == hd.blocks() and twin.sampling == hd.sampling
        blocks += hd.blocks()
        out += hd.h * hd.w * 3
    assert d[5]["out_offset"] == out and d[6]["block_offset"] == blocks
    assert rj.n_blocks == blocks + J.parse_header(seq).blocks() and rj.out_bytes == out + raw.size + 64 * 48 * 3
    assert (rj.max_h, rj.max_w) == (560, 600)
    rj2, targets = J.collate_jpeg_progressive([(files[0], 3), (seq, 4)])
    assert rj2.descriptors()["kind"].tolist() == [2, 0] and targets.tolist() == [3, 4]
    # a batch without progressive files packs exactly as without the flag
    a, b = J.pack_jpeg([seq, raw]), J.pack_jpeg([seq, raw], progressive=True)
    assert np.array_equal(a.data.numpy(), b.data.numpy()) and np.array_equal(a.desc.numpy(), b.desc.numpy())


def _sos_positions(data):
    hd = J.parse_progressive(data)
    return [s.data_start - (8 + 2 * len(s.comps)) for s in hd.scans], hd


def _patch(data, pos, val):
    b = bytearray(data)
    b[pos] = val
    return bytes(b)


def test_refusals_have_reasons():
    data = _bytes("p420_q90_64x48")
    sos, hd = _sos_positions(data)
    sof = data.find(b"\xff\xc2")
    ahal = lambda k: sos[k] + 4 + 2 * len(hd.scans[k].comps) + 3          # noqa: E731  (the Ah/Al byte of scan k)
    without = lambda k: data[:sos[k]] + data[hd.scans[k].data_end:]         # noqa: E731  (scan k and its data removed)
    cases = {
        "sof10": (data.replace(b"\xff\xc2", b"\xff\xca", 1), "arithmetic-coded progressive"),
        "12-bit": (_patch(data, sof + 4, 12), "12-bit"),
        "4 components": (data[:sof + 9] + b"\x04" + data[sof + 10:], "malformed SOF"),
        "dnl": (data[:sof + 5] + b"\x00\x00" + data[sof + 7:], "DNL"),
        "out-of-order refinement": (_patch(data, ahal(5), 0x32), "out-of-order refinement"),
        "refinement skipping a bit": (_patch(data, ahal(5), 0x20), "Al 0 other than Ah - 1"),
        "ac before dc": (data[:sos[0]] + data[sos[1]:], "before its DC scan"),
        "first pass twice": (data[:sos[2]] + data[sos[2]:sos[3]] + data[sos[2]:], "out-of-order refinement"),
        "ac scan of two components": (_patch(_patch(data, sos[0] + 11, 1), sos[0] + 12, 5), "AC scan with more than one component"),
        "no scans": (data[:sos[0]] + b"\xff\xd9", "no scan"),
        "sequential": (_seq_bytes("s420_q90_64x48"), "not progressive"),
        "not jpeg": (b"\x89PNG\r\n\x1a\n" + bytes(64), "no SOI"),
    }
    for k in range(1, 10):                      # truncated after k < all scans: the progression is incomplete
        cases[f"first {k} scans"] = (data[:hd.scans[k - 1].data_end] + b"\xff\xd9", "incomplete progression")
        cases[f"first {k} scans, no EOI"] = (data[:hd.scans[k - 1].data_end], "incomplete progression")
    for k in (6, 9):
        cases[f"without scan {k}"] = (without(k), "incomplete progression")
    cases["scan without data"] = (data[:hd.scans[9].data_start] + b"\xff\xd9", "has no entropy-coded data")
    for name, (blob, want) in cases.items():
        r = J.parse_progressive(blob)
        assert isinstance(r, J.Unsupported), name
        assert want in r.reason, (name, r.reason)
    # a real 4-component progressive frame (CMYK), when Pillow is there to write one
    try:
        from PIL import Image
        b = io.BytesIO()
        Image.new("CMYK", (16, 16), (10, 20, 30, 40)).save(b, "JPEG", progressive=True)
        r = J.parse_progressive(b.getvalue())
        assert isinstance(r, J.Unsupported) and "4 components" in r.reason
    except ImportError:
        pass
    # an SOS naming a Huffman table that was never defined
    r = J.parse_progressive(_patch(data, sos[1] + 4 + 2, 0x03))
    assert isinstance(r, J.Unsupported) and "is not defined" in r.reason


def test_truncations_and_garbage_never_raise_or_leave_the_buffer():
    data = _bytes("p420_rst_blocks3_100x75")
    hd = J.parse_progressive(data)
    head = hd.scans[1].data_start + 8

    def check(blob):
        r = J.parse_progressive(blob)
        assert isinstance(r, (J.Unsupported, J.ProgressiveHeader))
        if isinstance(r, J.ProgressiveHeader):
            for s in r.scans:
                assert 0 <= s.data_start < s.data_end <= len(blob)
            J.pack_jpeg([blob], progressive=True)
        return r
    for cut in range(0, head):
        assert isinstance(check(memoryview(data)[:cut]), J.Unsupported), cut
    for cut in range(head, len(data), 7):
        check(data[:cut])
    rng = np.random.default_rng(0)
    for _ in range(300):
        b = bytearray(data)
        for p in rng.integers(2, len(data), size=4):
            b[p] = int(rng.integers(0, 256))
        for p in rng.integers(2, hd.scans[0].data_start, size=2):
            b[p] = int(rng.integers(0, 256))
        try:
            check(bytes(b))
        except RuntimeError as e:            # pack_jpeg's Pillow fallback may refuse the damaged file: by name, not a crash
            assert "pack_jpeg" in str(e)
    assert isinstance(J.parse_progressive(b""), J.Unsupported)
    assert isinstance(J.parse_progressive(b"\xff\xd8" + bytes(rng.integers(0, 256, 100, dtype=np.uint8))), J.Unsupported)


def test_scan_bound():
    """More than MAX_SCANS scans is refused whatever they hold (here: one AC coefficient per scan, 63 scans)."""
    data = _bytes("pgrey_q90_7x9")
    sos, hd = _sos_positions(data)
    one = data[sos[1]:hd.scans[1].data_end]                 # SOS + data of the Y 1..5 first pass
    dht_and_all = data[hd.scans[0].data_end:sos[1]]         # the DHT in front of it
    body = b""
    for k in range(1, 64):
        s = bytearray(one)
        s[4 + 2 + 1] = s[4 + 2 + 2] = k                     # Ss = Se = k
        s[4 + 2 + 3] = 0x00
        body += bytes(s)
    blob = data[:hd.scans[0].data_end] + dht_and_all + body + b"\xff\xd9"
    r = J.parse_progressive(blob)
    assert isinstance(r, J.Unsupported) and f"more than {J.MAX_SCANS} scans" in r.reason
