"""Shared helpers for the tests (test infrastructure; may import oracle/)."""
import hashlib
import json
import os
from argparse import Namespace
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

LOGIT_TOL = 1e-5          # the north star's bound; the only absolute logit tolerance of the GPU tests


def scaled_tol(ref):
    """1e-5 is stated for logits of the reference's scale (|logit| <= ~3 on the golden images).  Inputs
    far from the calibration set (random stem bits, uncalibrated heads) give logits k times larger,
    where float32 itself no longer resolves 1e-5 (an ulp at 64 is 7.6e-6): the bound scales with k."""
    return LOGIT_TOL * max(1.0, float(np.abs(ref).max()) / 4.0)

VARIANT_ARGS = {
    "small": dict(nfilter=8, tfilter=8, layers=1),
    "xsmall": dict(nfilter=8, tfilter=8, layers=1),
    "full": dict(nfilter=6, tfilter=10, layers=1),
}


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def args_for(variant: str) -> Namespace:
    return Namespace(groups=[1, None, 4, None], **VARIANT_ARGS.get(variant, VARIANT_ARGS["small"]))


@lru_cache(maxsize=None)
def golden_npz(variant: str):
    with np.load(os.path.join(GOLD, f"ref_{variant}.npz")) as z:
        return {k: z[k] for k in z.files}


@lru_cache(maxsize=None)
def golden_json(variant: str):
    with open(os.path.join(GOLD, f"ref_luts_{variant}.json")) as f:
        return json.load(f)


@lru_cache(maxsize=None)
def golden_layout(variant: str):
    with open(os.path.join(GOLD, f"state_layout_{variant}.json")) as f:
        return json.load(f)


@lru_cache(maxsize=None)
def spec_and_state(variant: str):
    from scale_imagenet_amd.spec import VAlexSpec, make_spec
    from scale_imagenet_amd.synth import synth_state_dict
    spec = VAlexSpec() if variant == "valexnet" else make_spec(variant, **VARIANT_ARGS[variant])
    return spec, synth_state_dict(spec)


RESIZE_GEOMETRIES = [(375, 500), (500, 333), (256, 256), (300, 256), (256, 341), (224, 224), (1200, 900), (333, 500),
                     (480, 640)]


def resize_test_images(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """uint8 [n,h,w,3] test images for the Resize / CenterCrop checks: 8-pixel blocks plus noise (edges and
    flats).  numpy's PCG64 stream is stable across versions, so oracle/gen_golden.py (which feeds these to
    Pillow) and the tests regenerate identical inputs."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(n, h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 8, axis=1), 8, axis=2)[:, :h, :w].astype(np.int16)
    img += rng.integers(-20, 21, size=img.shape, dtype=np.int16)
    return np.clip(img, 0, 255).astype(np.uint8)


def oracle_views(img, descs, crop):
    """The views `descs` ([image, flags, bx, by, bw, bh, nw, nh, x0, y0], all of `img`) by the numpy oracle; a box is
    resized once however many windows are cut from it."""
    from oracle import pil_resize as PR
    resized, out = {}, []
    for d in descs:
        _, flags, bx, by, bw, bh, nw, nh, x0, y0 = (int(v) for v in d[:10])
        key = (bx, by, bw, bh, nw, nh)
        if key not in resized:
            r = img[by:by + bh, bx:bx + bw]
            if nw != bw:
                r = PR.resample_axis(r, nw, 1)             # horizontal pass first
            if nh != bh:
                r = PR.resample_axis(r, nh, 0)
            resized[key] = r
        v = resized[key][y0:y0 + crop, x0:x0 + crop]
        out.append(np.ascontiguousarray(v[:, ::-1] if flags & 1 else v))
    return out


@lru_cache(maxsize=None)
def golden_resize():
    with np.load(os.path.join(GOLD, "ref_resize.npz")) as z:
        return {k: z[k] for k in z.files}


def _jpeg_set(progressive: bool) -> str:
    return "jpeg_progressive" if progressive else "jpeg"


@lru_cache(maxsize=None)
def jpeg_fixture(progressive: bool = False):
    """The entries of ref_jpeg.json / ref_jpeg_progressive.json (what Pillow decodes of tests/golden/jpeg*/)."""
    with open(os.path.join(GOLD, f"ref_{_jpeg_set(progressive)}.json")) as f:
        return json.load(f)["images"]


def jpeg_bytes(name: str, progressive: bool = False) -> bytes:
    with open(os.path.join(GOLD, _jpeg_set(progressive), name + ".jpg"), "rb") as f:
        return f.read()


@lru_cache(maxsize=None)
def jpeg_arrays(progressive: bool = False):
    """Pillow's pixels of the fixtures that are small enough to be committed."""
    with np.load(os.path.join(GOLD, f"ref_{_jpeg_set(progressive)}_arrays.npz")) as z:
        return {k: z[k] for k in z.files}


def ragged_images(r):
    """The images of a RaggedU8 as host arrays [h, w, 3]."""
    data = r.data.cpu().numpy()
    out = []
    for d in r.descriptors():
        o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
        out.append(data[o:o + h * w * 3].reshape(h, w, 3))
    return out


def jpeg_diff(name: str, got: np.ndarray, progressive: bool = False) -> str:
    """For an assertion message: where a decoded image differs from Pillow's."""
    arr = jpeg_arrays(progressive).get(name)
    if arr is None:
        return f"{name}: sha differs ({int((got != 0).sum())} non-zero bytes)"
    d = np.argwhere(got != arr)
    return (f"{name}: {len(d)} bytes differ, first (y, x, c) {d[:8].tolist()}, "
            f"max |diff| {int(np.abs(got.astype(int) - arr.astype(int)).max())}")


def decode_images(items, device, progressive: bool = False):
    """pack_jpeg -> device -> decode_ragged -> host images."""
    from scale_imagenet_amd import jpeg as J
    return ragged_images(J.decode_ragged(J.pack_jpeg(items, progressive=progressive).to(device)))
