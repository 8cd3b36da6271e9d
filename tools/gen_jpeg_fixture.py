"""Writes the JPEG decoder's fixtures: tests/golden/jpeg/*.jpg (Pillow-encoded, seeded synthetic images),
tests/golden/ref_jpeg.json (per file: h, w, sampling, restart interval, whether the device decodes it, and the SHA-256
of what PILLOW ITSELF decodes, ``Image.open(f).convert("RGB")``) and tests/golden/ref_jpeg_arrays.npz (the full
decoded arrays of the smallest files, so that a failing test can say which pixels differ, and of the fallback files
(progressive, CMYK), which the GPU tests pack as already-decoded items).

    python tools/gen_jpeg_fixture.py        (needs Pillow; the tests only read what it writes)
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")
SUB = {"420": 2, "422": 1, "444": 0}
SMALL = 64 * 64          # files with at most this many pixels keep their full decoded array


def content(h, w, seed, natural=False):
    """Smooth regions plus texture plus a few hard edges: bright saturated areas make the coder emit 0xFF bytes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / (7 + 30 * natural) + c) * np.cos(y / (9 + 20 * natural) - c)
                     for c in (0.0, 1.3, 2.6)], axis=-1)
    tex = rng.normal(0, 25 if natural else 45, (h, w, 3))
    if natural:      # texture only in a band, smooth sky above, a bright object
        tex[: h // 3] *= 0.1
        cy, cx, r = h * 0.6, w * 0.55, min(h, w) * 0.2
        base[(y - cy) ** 2 + (x - cx) ** 2 < r * r] = (250, 240, 20)
    return np.clip(base + tex, 0, 255).astype(np.uint8)


def encode(a, mode="RGB", **kw):
    from PIL import Image
    im = Image.fromarray(a if mode != "L" else a[..., 0])
    if mode == "CMYK":
        im = im.convert("CMYK")
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def scan_has_stuffing(data):
    """True if the entropy-coded data after the (first) SOS holds an FF 00 pair."""
    i = data.find(b"\xff\xda")
    n = int.from_bytes(data[i + 2:i + 4], "big")
    return b"\xff\x00" in data[i + 2 + n:]


def cases():
    c = []
    for s in ("420", "422", "444"):
        c.append((f"s{s}_q90_64x48", 48, 64, "RGB", dict(quality=90, subsampling=SUB[s])))
        c.append((f"s{s}_q90_15x17", 17, 15, "RGB", dict(quality=90, subsampling=SUB[s])))
        c.append((f"s{s}_q90_33x31", 31, 33, "RGB", dict(quality=90, subsampling=SUB[s])))
    for (w, h) in ((1, 1), (7, 9), (8, 8), (16, 33), (2, 3), (17, 1), (1, 18)):
        c.append((f"s420_q90_{w}x{h}", h, w, "RGB", dict(quality=90, subsampling=2)))
    c.append(("s422_q90_7x9", 9, 7, "RGB", dict(quality=90, subsampling=1)))
    c.append(("s444_q90_1x1", 1, 1, "RGB", dict(quality=90, subsampling=0)))
    c.append(("grey_q90_61x47", 47, 61, "L", dict(quality=90)))
    c.append(("grey_q90_1x1", 1, 1, "L", dict(quality=90)))
    c.append(("grey_q90_7x9", 9, 7, "L", dict(quality=90)))
    c.append(("s420_rst_blocks3_100x75", 75, 100, "RGB", dict(quality=90, subsampling=2, restart_marker_blocks=3)))
    c.append(("s444_rst_rows1_90x70", 70, 90, "RGB", dict(quality=90, subsampling=0, restart_marker_rows=1)))
    c.append(("s422_rst_blocks1_41x23", 23, 41, "RGB", dict(quality=90, subsampling=1, restart_marker_blocks=1)))
    c.append(("grey_rst_blocks1_50x30", 30, 50, "L", dict(quality=90, restart_marker_blocks=1)))
    c.append(("s420_opt_120x90", 90, 120, "RGB", dict(quality=90, subsampling=2, optimize=True)))
    c.append(("grey_opt_70x50", 50, 70, "L", dict(quality=90, optimize=True)))
    c.append(("s420_q100_96x72", 72, 96, "RGB", dict(quality=100, subsampling=2)))
    c.append(("s444_q100_57x43", 43, 57, "RGB", dict(quality=100, subsampling=0)))
    c.append(("s420_q5_96x72", 72, 96, "RGB", dict(quality=5, subsampling=2)))
    c.append(("s420_q90_500x375_a", 375, 500, "RGB", dict(quality=90, subsampling=2)))
    c.append(("s420_q90_500x375_b", 375, 500, "RGB", dict(quality=90, subsampling=2)))
    c.append(("s420_q90_375x500_c", 500, 375, "RGB", dict(quality=90, subsampling=2)))
    c.append(("prog_q90_64x48", 48, 64, "RGB", dict(quality=90, progressive=True)))
    c.append(("cmyk_q90_40x30", 30, 40, "CMYK", dict(quality=90)))
    # wider than one IDCT tile (32 MCU columns) and taller than one pass of its grid (32 MCU rows)
    c.append(("s420_q90_600x560", 560, 600, "RGB", dict(quality=90, subsampling=2)))
    c.append(("s444_q90_300x60", 60, 300, "RGB", dict(quality=90, subsampling=0)))
    c.append(("s422_q90_530x40", 40, 530, "RGB", dict(quality=90, subsampling=1)))
    c.append(("grey_q90_530x270", 270, 530, "L", dict(quality=90)))
    return c


def main():
    import PIL
    from PIL import Image
    from scale_imagenet_amd import jpeg as J
    os.makedirs(OUT, exist_ok=True)
    entries, arrays, stuffed = [], {}, 0
    for seed, (name, h, w, mode, kw) in enumerate(cases()):
        data = encode(content(h, w, 1000 + seed, natural="500" in name or "560" in name), mode, **kw)
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        im = Image.open(io.BytesIO(data))
        rgb = np.asarray(im.convert("RGB"))
        assert rgb.shape == (h, w, 3)
        hd = J.parse_header(data)
        device = isinstance(hd, J.JpegHeader)
        e = {"name": name, "h": h, "w": w, "mode": im.mode, "device": device,
             "sha256": hashlib.sha256(rgb.tobytes()).hexdigest(), "bytes": len(data),
             "quantization": {str(k): list(v) for k, v in im.quantization.items()}}
        if device:
            e.update(sampling=[list(s) for s in hd.sampling], restart_interval=hd.restart_interval)
            stuffed += scan_has_stuffing(data)
            if "500" in name or "q100" in name:
                assert scan_has_stuffing(data), (name, "no FF 00 in the scan")
        else:
            e["reason"] = hd.reason
        if h * w <= SMALL or not device:
            arrays[name] = rgb
        entries.append(e)
        print(f"{name}: {len(data)} bytes, {'device' if device else 'fallback: ' + hd.reason}", flush=True)
    assert stuffed >= 8, stuffed
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_jpeg_arrays.npz"), **arrays)
    with open(os.path.join(ROOT, "tests", "golden", "ref_jpeg.json"), "w") as f:
        json.dump({"pillow_version": PIL.__version__, "images": entries}, f, indent=1)
        f.write("\n")
    print(f"Pillow {PIL.__version__}: {len(entries)} files, {stuffed} device files with stuffing")


if __name__ == "__main__":
    main()
