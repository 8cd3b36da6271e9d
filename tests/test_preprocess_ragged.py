"""CPU: the host side of the ragged Resize + CenterCrop (scale_imagenet_amd.preprocess.pack_u8 / collate_u8 /
RaggedU8), its C descriptor, and the numpy oracle against Pillow's outputs on the ragged geometries (the fixture
tests/golden/ref_resize_ragged.json, written by tools/gen_ragged_fixture.py)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from _util import GOLD, ROOT, resize_test_images, sha
from oracle import pil_resize as PR
from scale_imagenet_amd import _lib, preprocess, synth


def _fixture():
    with open(os.path.join(GOLD, "ref_resize_ragged.json")) as f:
        return json.load(f)


def test_descriptor_struct_matches_header():
    assert C.sizeof(_lib.ImageDesc) == 16
    assert [(n, C.sizeof(t), getattr(_lib.ImageDesc, n).offset) for n, t in _lib.ImageDesc._fields_] == \
        [("offset", 8, 0), ("h", 4, 8), ("w", 4, 12)]
    text = open(os.path.join(ROOT, "include", "ttnet.h")).read()
    m = re.search(r"typedef struct ttnet_image_desc \{(.*?)\} ttnet_image_desc;", text, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "int64_t offset; int32_t h, w;"
    assert preprocess.DESC_DTYPE.itemsize == 16


def test_pack_layout():
    sizes = [(375, 500), (1, 1), (100, 120), (7, 3), (500, 333)]
    ims = [resize_test_images(1, h, w, seed=i)[0] for i, (h, w) in enumerate(sizes)]
    ims[2] = torch.from_numpy(ims[2])                         # tensors are accepted too
    ims[3] = np.asfortranarray(ims[3])                        # and non-contiguous arrays
    r = preprocess.pack_u8(ims)
    assert len(r) == 5 and r.data.dtype == torch.uint8 and r.desc.dtype == torch.int64 and r.desc.shape == (5, 2)
    assert (r.max_h, r.max_w) == (500, 500)
    d = r.descriptors()
    off = 0
    for i, (h, w) in enumerate(sizes):
        assert (int(d["offset"][i]), int(d["h"][i]), int(d["w"][i])) == (off, h, w)
        want = np.asarray(ims[i])
        assert np.array_equal(r.data.numpy()[off:off + h * w * 3].reshape(h, w, 3), want)
        off += h * w * 3
    assert r.data.numel() == off
    # the int64 view is the packed record: offset, then h in the low and w in the high half
    assert int(r.desc[1, 0]) == 375 * 500 * 3 and int(r.desc[1, 1]) == 1 | (1 << 32)


def test_collate_and_pin():
    batch = [(resize_test_images(1, h, w, seed=h)[0], t) for (h, w), t in [((300, 400), 3), ((640, 480), 7), ((256, 256), 1)]]
    r, y = preprocess.collate_u8(batch)
    assert isinstance(r, preprocess.RaggedU8) and y.tolist() == [3, 7, 1]
    assert (r.max_h, r.max_w) == (640, 480)
    d = r.descriptors()
    assert d["offset"].tolist() == [0, 300 * 400 * 3, 300 * 400 * 3 + 640 * 480 * 3]
    loader = torch.utils.data.DataLoader(batch, batch_size=2, collate_fn=preprocess.collate_u8)
    got = [len(rb) for rb, _ in loader]
    assert got == [2, 1]
    r2 = r.to("cpu")
    assert r2.data.data_ptr() == r.data.data_ptr() and (r2.max_h, r2.max_w) == (640, 480)


@pytest.mark.parametrize("bad,msg", [
    (np.zeros((10, 10, 3), np.float32), "image 1 must be uint8"),
    (np.zeros((10, 10), np.uint8), "image 1 must be uint8"),
    (np.zeros((10, 10, 4), np.uint8), "image 1 must be uint8"),
    (np.zeros((0, 10, 3), np.uint8), "image 1 is 10x0"),
    (np.zeros((8193, 2, 3), np.uint8), "image 1 is 2x8193"),
    ([[1, 2, 3]], "image 1 must be uint8"),
])
def test_pack_rejects(bad, msg):
    with pytest.raises(RuntimeError, match=msg):
        preprocess.pack_u8([np.zeros((4, 4, 3), np.uint8), bad])
    with pytest.raises(RuntimeError):
        preprocess.pack_u8([])


def test_ragged_wrapper_rejects_host_batches():
    r = preprocess.pack_u8([np.zeros((300, 300, 3), np.uint8)])
    with pytest.raises(RuntimeError, match="move it"):
        preprocess.resize_center_crop_u8_ragged(r)
    with pytest.raises(RuntimeError, match="RaggedU8"):
        preprocess.resize_center_crop_u8_ragged(torch.zeros((1, 300, 300, 3), dtype=torch.uint8))


def test_imagenet_like_sizes_seeded():
    a, b = synth.imagenet_like_sizes(256, seed=0), synth.imagenet_like_sizes(256, seed=0)
    assert a == b and len(a) == 256 and len(set(a)) > 20
    assert max(max(s) for s in a) <= 4288 and min(min(s) for s in a) >= 60


def test_oracle_matches_pillow_fixture_on_ragged_geometries():
    """oracle/pil_resize.py against Pillow 12.x's own crops (SHA-256) on every ragged geometry: the GPU tests rely
    on both."""
    fx = _fixture()
    assert fx["pillow_version"].startswith("12.") and (fx["resize"], fx["crop"]) == (256, 224)
    assert len(fx["images"]) >= 10
    for e in fx["images"]:
        x = resize_test_images(1, e["h"], e["w"], seed=e["seed"])[0]
        assert sha(PR.resize_center_crop(x)) == e["sha256"], (e["h"], e["w"])
