"""CPU: the JPEG header walk (scale_imagenet_amd/jpeg.py parse_header) against the committed fixtures and Pillow, the
classification of what the device does not decode, malformed headers, and pack_jpeg's layout."""
import io
import os

import numpy as np
import pytest

from _util import GOLD, jpeg_bytes as _bytes, jpeg_fixture as _fixture
from scale_imagenet_amd import jpeg as J


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
          61, 54, 47, 55, 62, 63]


def _natural(zz):
    """A DQT table (zig-zag order) in natural order, as Pillow's Image.quantization reports it."""
    out = [0] * 64
    for k, v in enumerate(zz):
        out[ZIGZAG[k]] = v
    return out


@pytest.mark.parametrize("e", _fixture(), ids=lambda e: e["name"])
def test_parser_reproduces_fixture(e):
    hd = J.parse_header(_bytes(e["name"]))
    assert isinstance(hd, J.JpegHeader) == e["device"], getattr(hd, "reason", None)
    if not e["device"]:
        assert hd.reason == e["reason"]
        return
    assert (hd.h, hd.w) == (e["h"], e["w"])
    assert [list(s) for s in hd.sampling] == e["sampling"]
    assert hd.restart_interval == e["restart_interval"]
    assert ("rst" in e["name"]) == (hd.restart_interval > 0)
    # the quantisation tables as Pillow reports them (Image.quantization: natural order)
    assert {str(k): _natural(v) for k, v in hd.qt.items()} == e["quantization"]
    try:
        from PIL import Image
    except ImportError:
        return
    im = Image.open(io.BytesIO(_bytes(e["name"])))
    assert {k: list(v) for k, v in im.quantization.items()} == {k: _natural(v) for k, v in hd.qt.items()}
    assert im.size == (hd.w, hd.h)


def _with_marker(data, marker, payload):
    """Insert a marker segment right after SOI."""
    return data[:2] + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload + data[2:]


def _patch_sof(data, fn):
    i = data.find(b"\xff\xc0")
    b = bytearray(data)
    fn(b, i + 4)           # i + 4: first byte of the SOF payload (precision)
    return bytes(b)


def test_unsupported_kinds_have_reasons():
    base = _bytes("s420_q90_64x48")
    cases = {
        "progressive": (_bytes("prog_q90_64x48"), "progressive"),
        "cmyk": (_bytes("cmyk_q90_40x30"), "4 components"),
        "12-bit": (_patch_sof(base, lambda b, p: b.__setitem__(p, 12)), "12-bit"),
        "lossless": (base.replace(b"\xff\xc0", b"\xff\xc3", 1), "lossless"),
        "arithmetic": (base.replace(b"\xff\xc0", b"\xff\xc9", 1), "arithmetic"),
        "adobe rgb": (_with_marker(base, 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00"), "Adobe colour transform 0"),
        "440": (_patch_sof(base, lambda b, p: b.__setitem__(p + 7, 0x12)), "sampling"),
        "dnl height": (_patch_sof(base, lambda b, p: b.__setitem__(slice(p + 1, p + 3), b"\x00\x00")), "DNL"),
        "too wide": (_patch_sof(base, lambda b, p: b.__setitem__(slice(p + 3, p + 5), (9000).to_bytes(2, "big"))),
                     "beyond 8192"),
        "not jpeg": (b"\x89PNG\r\n\x1a\n" + bytes(64), "no SOI"),
    }
    for name, (data, want) in cases.items():
        hd = J.parse_header(data)
        assert isinstance(hd, J.Unsupported), name
        assert want in hd.reason, (name, hd.reason)


def test_truncated_and_garbage_headers_never_read_out_of_range():
    data = _bytes("s420_opt_120x90")
    hd = J.parse_header(data)
    for cut in range(0, hd.scan_offset):
        r = J.parse_header(memoryview(data)[:cut])
        assert isinstance(r, J.Unsupported), cut
    rng = np.random.default_rng(0)
    for _ in range(300):
        b = bytearray(data[:hd.scan_offset + 16])
        for p in rng.integers(2, hd.scan_offset, size=4):
            b[p] = int(rng.integers(0, 256))
        r = J.parse_header(bytes(b))
        assert isinstance(r, (J.Unsupported, J.JpegHeader))
    assert isinstance(J.parse_header(b""), J.Unsupported)
    assert isinstance(J.parse_header(b"\xff\xd8" + bytes(rng.integers(0, 256, 100, dtype=np.uint8))), J.Unsupported)


def test_pack_jpeg_layout():
    names = ["s420_q90_64x48", "grey_q90_61x47", "s444_rst_rows1_90x70", "s422_q90_15x17"]
    files = [_bytes(n) for n in names]
    raw = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    rj = J.pack_jpeg(files + [raw])
    d = rj.descriptors()
    flat = rj.data.numpy()
    assert len(rj) == 5 and rj.data.numel() % 16 == 0
    out, blocks = 0, 0
    for i, f in enumerate(files):
        hd = J.parse_header(f)
        assert d[i]["kind"] == J.KIND_JPEG
        assert d[i]["table_offset"] % 16 == 0 and d[i]["data_offset"] == d[i]["table_offset"] + J.TABLE_BYTES
        o = int(d[i]["data_offset"])
        assert flat[o:o + d[i]["data_bytes"]].tobytes() == f[hd.scan_offset:]
        t = int(d[i]["table_offset"])
        q = flat[t:t + 384].view("<u2").reshape(3, 64)
        for k, c in enumerate(hd.comps):
            assert list(q[k]) == hd.qt[c[3]]
        for k, (td, ta) in enumerate(hd.scan_tables):
            for a, key in enumerate(((0, td), (1, ta))):
                counts, syms = hd.dht[key]
                p = t + 384 + (2 * k + a) * 272
                assert list(flat[p:p + 16]) == counts and list(flat[p + 16:p + 16 + len(syms)]) == syms
        assert (d[i]["h"], d[i]["w"], d[i]["ncomp"], d[i]["restart_interval"]) == (hd.h, hd.w, hd.ncomp,
                                                                                    hd.restart_interval)
        assert d[i]["block_offset"] == blocks and d[i]["out_offset"] == out
        blocks += hd.blocks()
        out += hd.h * hd.w * 3
    assert d[4]["kind"] == J.KIND_RAW and d[4]["out_offset"] == out and d[4]["data_offset"] % 16 == 0
    o = int(d[4]["data_offset"])
    assert np.array_equal(flat[o:o + raw.size], raw.reshape(-1))
    assert rj.n_blocks == blocks and rj.out_bytes == out + raw.size
    assert (rj.max_h, rj.max_w) == (70, 90)
    assert rj.reasons == [None] * 4 + ["already decoded"]


def test_pack_jpeg_fallback_and_errors():
    prog = _bytes("prog_q90_64x48")
    try:
        import PIL  # noqa: F401
        rj = J.pack_jpeg([prog])
        assert rj.descriptors()[0]["kind"] == J.KIND_RAW and "progressive" in rj.reasons[0]
        arr = np.load(os.path.join(GOLD, "ref_jpeg_arrays.npz"))["prog_q90_64x48"]
        o = int(rj.descriptors()[0]["data_offset"])
        assert np.array_equal(rj.data.numpy()[o:o + arr.size], arr.reshape(-1))
    except ImportError:
        with pytest.raises(RuntimeError, match="Pillow"):
            J.pack_jpeg([prog], names=["prog.jpg"])
    with pytest.raises(RuntimeError, match="uint8 HWC"):
        J.pack_jpeg([np.zeros((4, 4), np.uint8)])
    with pytest.raises(RuntimeError, match="not file bytes"):
        J.pack_jpeg([12])


def test_file_bytes_folder_and_collate(tmp_path):
    for c, files in (("b_cls", ["z.jpg", "a.JPEG"]), ("a_cls", ["m.jpg"])):
        (tmp_path / c).mkdir()
        for f in files:
            (tmp_path / c / f).write_bytes(_bytes("s420_q90_8x8"))
    (tmp_path / "a_cls" / "notes.txt").write_text("x")
    ds = J.FileBytesFolder(str(tmp_path))
    assert ds.classes == ["a_cls", "b_cls"]
    assert [os.path.basename(p) for p, _ in ds.samples] == ["m.jpg", "a.JPEG", "z.jpg"]
    assert ds.targets == [0, 1, 1]
    rj, targets = J.collate_jpeg([ds[i] for i in range(len(ds))])
    assert len(rj) == 3 and targets.tolist() == [0, 1, 1]
