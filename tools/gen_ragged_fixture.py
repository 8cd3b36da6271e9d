"""Writes tests/golden/ref_resize_ragged.json: what PILLOW ITSELF computes for Resize(256) + CenterCrop(224) on the
geometries the ragged resize (ttnet_resize_center_crop_u8_ragged) is tested on beyond tests/golden/ref_resize.npz:
camera-sized images (the single-size kernel refuses 2848 x 4288 and above), unequal and large tap counts, extreme
aspects, no resampling, upscaling.  Per geometry: SHA-256 of Pillow's crop of one seeded test image
(tests/_util.py:resize_test_images, seed h * 1000 + w).  torchvision's size and crop-offset rules are restated
(oracle/pil_resize.py); the numpy oracle is asserted byte-identical to Pillow on every geometry.

    python tools/gen_ragged_fixture.py        (needs Pillow; the tests only read the JSON)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (h, w): taps (horizontal / vertical) at 256 / 224 in the comments
GEOMETRIES = [(3000, 4000),     # 25 / 25
              (2848, 4288),     # 25 / 25
              (512, 769),       # 7 / 5
              (600, 800),       # 7 / 7
              (1400, 1100),     # 11 / 11
              (4000, 257),      # 3 / 33
              (257, 4000),      # 33 / 3
              (256, 256),       # no resampling
              (256, 300),       # no resampling, crop only
              (100, 120)]       # upscale


def main():
    import PIL
    from PIL import Image
    from _util import resize_test_images, sha
    from oracle import pil_resize as PR
    entries = []
    for (h, w) in GEOMETRIES:
        seed = h * 1000 + w
        x = resize_test_images(1, h, w, seed=seed)[0]
        nh, nw = PR.resized_size(h, w, 256)
        im = Image.fromarray(x)
        if (nh, nw) != (h, w):
            im = im.resize((nw, nh), Image.BILINEAR)
        a = np.asarray(im)
        top, left = int(round((nh - 224) / 2.0)), int(round((nw - 224) / 2.0))
        crop = a[top:top + 224, left:left + 224]
        assert crop.shape == (224, 224, 3)
        assert np.array_equal(crop, PR.resize_center_crop(x)), (h, w, "oracle/pil_resize.py != Pillow")
        entries.append({"h": h, "w": w, "seed": seed, "sha256": sha(crop)})
        print(f"{h}x{w}: {entries[-1]['sha256'][:16]}", flush=True)
    out = {"pillow_version": PIL.__version__, "resize": 256, "crop": 224, "images": entries}
    path = os.path.join(ROOT, "tests", "golden", "ref_resize_ragged.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"Pillow {PIL.__version__}: {len(entries)} geometries, oracle/pil_resize.py byte-identical on all -> {path}")


if __name__ == "__main__":
    main()
