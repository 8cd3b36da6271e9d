"""Writes the progressive JPEG decoder's fixtures: tests/golden/jpeg_progressive/*.jpg (Pillow-encoded with
progressive=True: libjpeg's default scan script, which has all four scan kinds), tests/golden/ref_jpeg_progressive.json
(per file: h, w, sampling, restart interval, the scan list, and the SHA-256 of what PILLOW ITSELF decodes,
``Image.open(f).convert("RGB")``) and tests/golden/ref_jpeg_progressive_arrays.npz (the full decoded arrays of the
files of at most 64 x 64 pixels, so that a failing test can say which pixels differ).

    python tools/gen_jpeg_progressive_fixture.py        (needs Pillow; the tests only read what it writes)
"""
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_jpeg_fixture import SMALL, SUB, content, encode  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_progressive")
MAX_FILE = 145 * 1024      # no fixture larger than the largest sequential one


def cases():
    P = dict(progressive=True, optimize=True)
    c = []
    for s in ("420", "422", "444"):
        for (w, h) in ((64, 48), (15, 17), (33, 31)):
            c.append((f"p{s}_q90_{w}x{h}", h, w, "RGB", dict(quality=90, subsampling=SUB[s], **P)))
    for (w, h) in ((1, 1), (7, 9), (8, 8), (16, 33), (17, 1), (1, 18)):
        c.append((f"p420_q90_{w}x{h}", h, w, "RGB", dict(quality=90, subsampling=2, **P)))
    c.append(("p422_q90_7x9", 9, 7, "RGB", dict(quality=90, subsampling=1, **P)))
    c.append(("p444_q90_1x1", 1, 1, "RGB", dict(quality=90, subsampling=0, **P)))
    for (w, h) in ((61, 47), (1, 1), (7, 9), (530, 270)):
        c.append((f"pgrey_q90_{w}x{h}", h, w, "L", dict(quality=90, **P)))
    c.append(("p420_q5_96x72", 72, 96, "RGB", dict(quality=5, subsampling=2, **P)))
    c.append(("p420_q100_96x72", 72, 96, "RGB", dict(quality=100, subsampling=2, **P)))
    c.append(("p444_q100_57x43", 43, 57, "RGB", dict(quality=100, subsampling=0, **P)))
    c.append(("p422_q5_75x41", 41, 75, "RGB", dict(quality=5, subsampling=1, **P)))
    c.append(("p420_rst_blocks3_100x75", 75, 100, "RGB", dict(quality=90, subsampling=2, restart_marker_blocks=3, **P)))
    c.append(("p444_rst_rows1_90x70", 70, 90, "RGB", dict(quality=90, subsampling=0, restart_marker_rows=1, **P)))
    c.append(("p422_rst_blocks1_41x23", 23, 41, "RGB", dict(quality=90, subsampling=1, restart_marker_blocks=1, **P)))
    c.append(("p420_rst_rows1_203x120", 120, 203, "RGB", dict(quality=90, subsampling=2, restart_marker_rows=1, **P)))
    c.append(("pgrey_rst_blocks1_50x30", 30, 50, "L", dict(quality=90, restart_marker_blocks=1, **P)))
    c.append(("pgrey_rst_rows1_70x50", 50, 70, "L", dict(quality=90, restart_marker_rows=1, **P)))
    # custom tables with entries beyond 255 (16-bit DQT); Pillow takes natural-order lists
    q16 = [[min(1 + 9 * k, 600) for k in range(64)], [min(2 + 12 * k, 900) for k in range(64)]]
    c.append(("p420_qt16_88x56", 56, 88, "RGB", dict(qtables=q16, subsampling=2, **P)))
    c.append(("p420_q90_500x375_a", 375, 500, "RGB", dict(quality=90, subsampling=2, **P)))
    c.append(("p420_q90_500x375_b", 375, 500, "RGB", dict(quality=90, subsampling=2, **P)))
    c.append(("p420_q90_375x500_c", 500, 375, "RGB", dict(quality=90, subsampling=2, **P)))
    c.append(("p420_q90_600x560", 560, 600, "RGB", dict(quality=90, subsampling=2, **P)))
    c.append(("p444_q90_300x60", 60, 300, "RGB", dict(quality=90, subsampling=0, **P)))
    c.append(("p422_q90_530x40", 40, 530, "RGB", dict(quality=90, subsampling=1, **P)))
    return c


def main():
    import PIL
    from PIL import Image
    from scale_imagenet_amd import jpeg as J
    os.makedirs(OUT, exist_ok=True)
    entries, arrays = [], {}
    kinds = set()
    for seed, (name, h, w, mode, kw) in enumerate(cases()):
        data = encode(content(h, w, 2000 + seed, natural="500" in name or "560" in name), mode, **kw)
        assert len(data) <= MAX_FILE, (name, len(data))
        im = Image.open(io.BytesIO(data))
        rgb = np.asarray(im.convert("RGB"))
        assert rgb.shape == (h, w, 3)
        hd = J.parse_progressive(data)
        assert isinstance(hd, J.ProgressiveHeader), (name, hd)
        assert "progressive" in J.parse_header(data).reason
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        scans = [{"comps": s.comps, "ss": s.ss, "se": s.se, "ah": s.ah, "al": s.al, "restart_interval": s.restart_interval}
                 for s in hd.scans]
        kinds |= {(s.ss == 0, s.ah == 0) for s in hd.scans}
        assert ("rst" in name) == (hd.restart_interval > 0)
        entries.append({"name": name, "h": h, "w": w, "mode": im.mode, "sha256": hashlib.sha256(rgb.tobytes()).hexdigest(),
                        "bytes": len(data), "sampling": [list(s) for s in hd.sampling],
                        "restart_interval": hd.restart_interval, "n_scans": len(scans), "scans": scans,
                        "max_quant": max(max(v) for v in hd.qt.values())})
        if h * w <= SMALL:
            arrays[name] = rgb
        print(f"{name}: {len(data)} bytes, {len(scans)} scans, DRI {hd.restart_interval}", flush=True)
    assert len(kinds) == 4, kinds                     # DC / AC, first pass / refinement
    assert any(e["max_quant"] > 255 for e in entries), "no 16-bit quantisation table"
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_jpeg_progressive_arrays.npz"), **arrays)
    with open(os.path.join(ROOT, "tests", "golden", "ref_jpeg_progressive.json"), "w") as f:
        json.dump({"pillow_version": PIL.__version__, "images": entries}, f, indent=1)
        f.write("\n")
    print(f"Pillow {PIL.__version__}: {len(entries)} files")


if __name__ == "__main__":
    main()
