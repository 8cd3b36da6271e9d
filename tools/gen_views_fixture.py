"""Writes tests/golden/ref_views.json: what PILLOW ITSELF computes for the views of ttnet_resize_views_u8_ragged
(include/ttnet.h), as SHA-256 per view next to the view's descriptor.

  families   per geometry (h, w, resize, crop) the CENTER / FLIP / FIVE / TEN views of one seeded test image
             (tests/_util.py:resize_test_images, seed h * 1000 + w), made the way torchvision makes them, restated on
             Image objects: Image.resize(BILINEAR) for Resize, Image.crop for the five crops, Image.transpose(
             FLIP_LEFT_RIGHT) and the five crops again for the other five -- NOT through the window formulas.  The
             descriptors beside them are the formulas' (preprocess.eval_views_host), so a wrong formula shows as a hash
             that the kernel cannot meet.
  boxes      explicit views of three small images packed into one buffer: Image.crop(box).resize((nw, nh), BILINEAR),
             then Image.crop of the window and the transpose.

The numpy oracle (oracle/pil_resize.resample_axis: horizontal pass, then vertical pass, each skipped when that size is
unchanged) is asserted byte-identical to Pillow on every view.

    python tools/gen_views_fixture.py        (needs Pillow; the tests only read the JSON)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (h, w, resize, crop)
FAMILY_CASES = [(375, 500, 256, 224),      # odd x margin
                (500, 333, 256, 224),
                (257, 300, 256, 224),
                (100, 120, 256, 224),      # upscale
                (256, 256, 256, 224),      # no resampling
                (224, 300, 224, 224),      # zero y margin: the five windows collapse to two distinct ones
                (61, 47, 40, 32),
                (47, 61, 41, 32),          # odd margin
                (2848, 4288, 256, 224)]    # 25 taps
# three small images in one buffer of 20340 bytes (not a multiple of 16): (h, w)
BOX_IMAGES = [(61, 47), (40, 80), (23, 31)]
# crop -> (image, flip, bx, by, bw, bh, nw, nh, x0, y0)
BOX_CASES = {
    8: [(0, 0, 5, 7, 1, 1, 8, 8, 0, 0),              # a 1 x 1 box upscaled
        (2, 1, 22, 13, 9, 10, 12, 8, 2, 0),          # ends on the buffer's last byte
        (0, 0, 3, 4, 16, 30, 16, 11, 4, 2),          # bw == nw, bh != nh
        (1, 1, 2, 1, 40, 12, 9, 12, 0, 3),           # bh == nh, bw != nw
        (1, 1, 5, 3, 73, 4, 10, 10, 1, 2),           # scale 7.3 horizontally, 0.4 vertically
        (0, 0, 0, 0, 20, 20, 12, 12, 2, 2),          # the four corners of image 0
        (0, 1, 27, 0, 20, 20, 12, 12, 2, 2),
        (0, 0, 0, 41, 20, 20, 12, 12, 2, 2),
        (0, 1, 27, 41, 20, 20, 12, 12, 2, 2)],
    32: [(1, 0, 0, 0, 80, 40, 40, 36, 4, 2),
         (0, 1, 10, 10, 30, 40, 32, 32, 0, 0),
         (2, 0, 0, 0, 31, 23, 64, 50, 30, 18)],
    224: [(2, 1, 3, 2, 20, 18, 224, 300, 0, 70),
          (1, 0, 0, 0, 80, 40, 448, 224, 100, 0)],
}


def five_crop(im, crop):
    """torchvision.transforms.functional.five_crop on an Image: tl, tr, bl, br, center_crop."""
    w, h = im.size
    top, left = int(round((h - crop) / 2.0)), int(round((w - crop) / 2.0))
    return [im.crop((0, 0, crop, crop)), im.crop((w - crop, 0, w, crop)), im.crop((0, h - crop, crop, h)),
            im.crop((w - crop, h - crop, w, h)), im.crop((left, top, left + crop, top + crop))]


def family_images(x, resize, crop):
    """{family: [Image]} of one uint8 image, by Pillow's own operations."""
    from PIL import Image
    from oracle import pil_resize as PR
    h, w, _ = x.shape
    nh, nw = PR.resized_size(h, w, resize)
    im = Image.fromarray(x)
    if (nh, nw) != (h, w):
        im = im.resize((nw, nh), Image.BILINEAR)
    mirrored = im.transpose(Image.FLIP_LEFT_RIGHT)
    five, five_m = five_crop(im, crop), five_crop(mirrored, crop)
    return {"center": [five[4]], "flip": [five[4], five_m[4]], "five": five, "ten": five + five_m}


def oracle_view(img, d, crop):
    """The view `d` = (image, flags, bx, by, bw, bh, nw, nh, x0, y0) of `img` by the numpy oracle."""
    from oracle import pil_resize as PR
    _, flags, bx, by, bw, bh, nw, nh, x0, y0 = d
    out = img[by:by + bh, bx:bx + bw]
    if nw != bw:
        out = PR.resample_axis(out, nw, 1)
    if nh != bh:
        out = PR.resample_axis(out, nh, 0)
    out = out[y0:y0 + crop, x0:x0 + crop]
    return np.ascontiguousarray(out[:, ::-1] if flags & 1 else out)


def main():
    import PIL
    from PIL import Image
    from _util import resize_test_images, sha
    from scale_imagenet_amd import preprocess
    families, n_views = [], 0
    for (h, w, resize, crop) in FAMILY_CASES:
        seed = h * 1000 + w
        x = resize_test_images(1, h, w, seed=seed)[0]
        ims = family_images(x, resize, crop)
        entry = {"h": h, "w": w, "resize": resize, "crop": crop, "seed": seed, "views": {}}
        cache = {}
        for family, crops in ims.items():
            desc = preprocess.eval_views_host([(h, w)], family, resize, crop).records()[:, :10].tolist()
            assert len(desc) == len(crops)
            hashes = []
            for d, c in zip(desc, crops):
                a = np.asarray(c)
                assert a.shape == (crop, crop, 3)
                if tuple(d) not in cache:
                    cache[tuple(d)] = oracle_view(x, d, crop)
                assert np.array_equal(a, cache[tuple(d)]), (h, w, family, d, "oracle/pil_resize.py != Pillow")
                hashes.append(sha(a))
            entry["views"][family] = {"desc": desc, "sha256": hashes}
            n_views += len(desc)
        families.append(entry)
        print(f"{h}x{w} resize {resize} crop {crop}: ten[0] {entry['views']['ten']['sha256'][0][:16]}", flush=True)
    box_images = [resize_test_images(1, h, w, seed=h * 1000 + w)[0] for h, w in BOX_IMAGES]
    assert sum(a.size for a in box_images) % 16 != 0
    last = BOX_CASES[8][1]
    assert last[0] == len(BOX_IMAGES) - 1 and last[2] + last[4] == BOX_IMAGES[-1][1] and last[3] + last[5] == BOX_IMAGES[-1][0]
    boxes = []
    for crop, cases in BOX_CASES.items():
        hashes = []
        for d in cases:
            image, flags, bx, by, bw, bh, nw, nh, x0, y0 = d
            im = Image.fromarray(box_images[image]).crop((bx, by, bx + bw, by + bh)).resize((nw, nh), Image.BILINEAR)
            im = im.crop((x0, y0, x0 + crop, y0 + crop))
            if flags & 1:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            a = np.asarray(im)
            assert np.array_equal(a, oracle_view(box_images[image], d, crop)), (d, "oracle/pil_resize.py != Pillow")
            hashes.append(sha(a))
        boxes.append({"crop": crop, "desc": [list(d) for d in cases], "sha256": hashes})
        n_views += len(cases)
    out = {"pillow_version": PIL.__version__, "fields": list(preprocess.VIEW_FIELDS), "families": families,
           "box_images": [{"h": h, "w": w, "seed": h * 1000 + w} for h, w in BOX_IMAGES], "boxes": boxes}
    path = os.path.join(ROOT, "tests", "golden", "ref_views.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"Pillow {PIL.__version__}: {n_views} views, oracle/pil_resize.py byte-identical on all -> {path}")


if __name__ == "__main__":
    main()
