"""Writes tests/golden/ref_resize_paths.json: what PILLOW ITSELF computes on the geometries that reach every path of
csrc/preproc.hip (tests/_resize_paths.py holds the case lists and says which path each one reaches):

  uniform   per case (h, w, resize, crop, n, seed): SHA-256 of Pillow's Image.resize(BILINEAR) + centre crop of each of
            the n seeded test images (tests/_util.py:resize_test_images) -- every tap-count instantiation of the
            single-size kernel, the buffer's last partial piece, short last tiles, the largest accepted geometry, and
            the two refused ones (which the ragged entry point serves);
  ragged    per (resize, crop) one mixed batch of five images (_resize_paths.ragged_sizes): crops 20 to 684, the crops
            around the WIDE threshold (340 / 344) and three dword columns per thread (684);
  views     for the WIDE crops 344 and 684: the ten-crop sequence of every image of that batch, made the way torchvision
            makes it on Image objects (tools/gen_views_fixture.py:family_images), and explicit boxes
            (_resize_paths.view_boxes) by Image.crop -> resize -> crop -> transpose.

The numpy oracle (oracle/pil_resize.py) is asserted byte-identical to Pillow on every image and view.  Hashes and
integers only.

    python tools/gen_resize_paths_fixture.py        (needs Pillow; the tests only read the JSON)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def pillow_center_crop(x, resize, crop):
    from PIL import Image
    from oracle import pil_resize as PR
    h, w, _ = x.shape
    nh, nw = PR.resized_size(h, w, resize)
    im = Image.fromarray(x)
    if (nh, nw) != (h, w):
        im = im.resize((nw, nh), Image.BILINEAR)
    a = np.asarray(im)
    top, left = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    out = a[top:top + crop, left:left + crop]
    assert out.shape == (crop, crop, 3)
    return out


def main():
    import PIL
    from PIL import Image
    import _resize_paths as RP
    from _util import oracle_views, sha
    from gen_views_fixture import family_images
    from scale_imagenet_amd import preprocess
    uniform = []
    for c in RP.UNIFORM_CASES + RP.UNIFORM_REFUSED:
        hashes = []
        for x, want in zip(c.images(), RP.uniform_oracle(c)):
            a = pillow_center_crop(x, c.resize, c.crop)
            assert np.array_equal(a, want), (c.key, "oracle/pil_resize.py != Pillow")
            hashes.append(sha(a))
        uniform.append({"case": c.case, "h": c.h, "w": c.w, "resize": c.resize, "crop": c.crop, "n": c.n, "seed": c.seed,
                        "sha256": hashes})
        print(f"{c.key}: {hashes[0][:16]}", flush=True)
    ragged = []
    for resize, crop in RP.RAGGED_PAIRS:
        images = []
        for i, (x, want) in enumerate(zip(RP.ragged_images(resize), RP.ragged_oracle(resize, crop))):
            a = pillow_center_crop(x, resize, crop)
            assert np.array_equal(a, want), (resize, crop, x.shape, "oracle/pil_resize.py != Pillow")
            images.append({"h": x.shape[0], "w": x.shape[1], "seed": RP.ragged_seed(resize, i), "sha256": sha(a)})
        ragged.append({"resize": resize, "crop": crop, "images": images})
        print(f"ragged {resize} / {crop}: {images[0]['sha256'][:16]}", flush=True)
    views, n_views = [], 0
    for resize, crop in RP.VIEW_PAIRS:
        ims = RP.ragged_images(resize)
        ten = []
        for x in ims:
            desc = preprocess.eval_views_host([x.shape[:2]], "ten", resize, crop).records()
            crops = family_images(np.asarray(x), resize, crop)["ten"]
            for c, want in zip(crops, oracle_views(x, desc, crop)):
                a = np.asarray(c)
                assert np.array_equal(a, want), (resize, crop, x.shape, "oracle/pil_resize.py != Pillow")
                ten.append(sha(a))
        boxes = RP.view_boxes(resize, crop)
        hashes = []
        for d in boxes:
            image, flags, bx, by, bw, bh, nw, nh, x0, y0 = d
            im = Image.fromarray(np.asarray(ims[image])).crop((bx, by, bx + bw, by + bh)).resize((nw, nh), Image.BILINEAR)
            im = im.crop((x0, y0, x0 + crop, y0 + crop))
            if flags & 1:
                im = im.transpose(Image.FLIP_LEFT_RIGHT)
            a = np.asarray(im)
            assert np.array_equal(a, oracle_views(ims[image], [d], crop)[0]), (d, "oracle/pil_resize.py != Pillow")
            hashes.append(sha(a))
        views.append({"resize": resize, "crop": crop, "ten": ten, "boxes": {"desc": [list(d) for d in boxes], "sha256": hashes}})
        n_views += len(ten) + len(boxes)
        print(f"views {resize} / {crop}: {ten[0][:16]}", flush=True)
    out = {"pillow_version": PIL.__version__, "uniform": uniform, "ragged": ragged, "views": views}
    path = os.path.join(ROOT, "tests", "golden", "ref_resize_paths.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"Pillow {PIL.__version__}: {sum(len(u['sha256']) for u in uniform)} uniform crops, "
          f"{sum(len(r['images']) for r in ragged)} ragged crops, {n_views} views, oracle/pil_resize.py byte-identical on all "
          f"-> {path}")


if __name__ == "__main__":
    main()
