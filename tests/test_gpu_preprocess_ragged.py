"""GPU: Resize(256) + CenterCrop(224) of RAGGED batches in one launch (ttnet_resize_center_crop_u8_ragged) against
Pillow's own crops (tests/golden/ref_resize.npz, tests/golden/ref_resize_ragged.json), oracle/pil_resize.py, and the
single-size entry point; bad descriptors, graph capture with new geometries, and the eval forward."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _util import GOLD, RESIZE_GEOMETRIES, args_for, golden_resize, resize_test_images, sha, spec_and_state
from oracle import pil_resize as PR
from scale_imagenet_amd import _lib, preprocess, synth, ttnet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _fixture():
    with open(os.path.join(GOLD, "ref_resize_ragged.json")) as f:
        return json.load(f)["images"]


def _mixed():
    """(image, sha of Pillow's crop) for every geometry with a committed Pillow output; the last image is 100 x 120
    (upscaling) so that the buffer's length is not a multiple of 16."""
    g = golden_resize()
    out = [(resize_test_images(2, h, w, seed=h * 1000 + w)[0], str(g[f"sha_{h}x{w}"][0])) for h, w in RESIZE_GEOMETRIES]
    fx = sorted(_fixture(), key=lambda e: (e["h"], e["w"]) == (100, 120))
    out += [(resize_test_images(1, e["h"], e["w"], seed=e["seed"])[0], e["sha256"]) for e in fx]
    assert (out[-1][0].shape[:2]) == (100, 120)
    return out


def test_mixed_batch_matches_pillow_and_oracle():
    items = _mixed()
    r = preprocess.pack_u8([x for x, _ in items])
    assert r.data.numel() % 16 != 0
    got = preprocess.resize_center_crop_u8_ragged(r.to(DEV)).cpu().numpy()
    assert got.shape == (len(items), 224, 224, 3)
    for i, (x, want_sha) in enumerate(items):
        assert sha(got[i]) == want_sha, (i, x.shape, "differs from Pillow's output")
        want = PR.resize_center_crop(x)
        assert np.array_equal(got[i], want), (i, x.shape, int(np.abs(got[i].astype(int) - want.astype(int)).max()))
    preprocess.check_ragged(DEV)


@pytest.mark.parametrize("h,w", RESIZE_GEOMETRIES)
def test_same_bytes_as_single_size_entry_point(h, w):
    x = resize_test_images(5, h, w, seed=h + 7 * w)
    single = preprocess.resize_center_crop_u8(torch.from_numpy(x).to(DEV))
    ragged = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8(list(x)).to(DEV))
    assert torch.equal(single, ragged)


def test_order_and_batch_composition():
    sizes = synth.imagenet_like_sizes(256, seed=3)
    ims = [resize_test_images(1, h, w, seed=1000 + i)[0] for i, (h, w) in enumerate(sizes)]
    got = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8(ims).to(DEV)).cpu().numpy()
    for i, x in enumerate(ims):
        assert np.array_equal(got[i], PR.resize_center_crop(x)), (i, x.shape)
    perm = np.random.default_rng(0).permutation(len(ims))
    shuffled = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8([ims[p] for p in perm]).to(DEV)).cpu().numpy()
    assert np.array_equal(shuffled, got[perm])
    big = int(np.argmax([h * w for h, w in sizes]))
    alone = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8([ims[big]]).to(DEV)).cpu().numpy()
    assert np.array_equal(alone[0], got[big])
    preprocess.check_ragged(DEV)


def _raw_call(src, src_bytes, desc, max_h, max_w, out, bad):
    return _lib.load().ttnet_resize_center_crop_u8_ragged(
        C.c_void_p(src.data_ptr()), int(src_bytes), C.c_void_p(desc.data_ptr()), desc.shape[0], max_h, max_w, 256, 224,
        C.c_void_p(out.data_ptr()), C.c_void_p(bad.data_ptr()), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def test_bad_descriptors_give_zero_crops_and_are_counted():
    """The source allocation is 64 MiB, the declared src_bytes far smaller: a descriptor past src_bytes or beyond
    max_h / max_w stays inside the allocation even if the guard were wrong."""
    ims = [resize_test_images(1, h, w, seed=i)[0] for i, (h, w) in enumerate([(375, 500), (300, 400), (500, 333), (256, 300)])]
    r = preprocess.pack_u8(ims)
    src = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    src[:r.data.numel()] = r.data.to(DEV)
    d = r.descriptors().copy()
    d[1]["offset"] = r.data.numel() - 100          # ends past src_bytes
    d[2]["h"] = 600                                # beyond max_h
    d = np.concatenate([d, np.array([(-48, 10, 10), (0, 0, 5)], dtype=preprocess.DESC_DTYPE)])   # negative offset, h = 0
    desc = torch.from_numpy(d.view(np.int64).reshape(-1, 2)).to(DEV)
    out = torch.full((len(d), 224, 224, 3), 7, dtype=torch.uint8, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_raw_call(src, r.data.numel(), desc, 500, 500, out, bad))
    got = out.cpu().numpy()
    assert int(bad.item()) == 4
    for i in (1, 2, 4, 5):
        assert not got[i].any(), i
    for i in (0, 3):                                                        # the good neighbours are untouched
        assert np.array_equal(got[i], PR.resize_center_crop(ims[i])), i
    # the Python wrapper: a batch with a bad descriptor raises on a later call (check_ragged at once)
    rb = r.to(DEV)
    rb.desc[1, 0] = r.data.numel()                  # image 1 starts at the end of the buffer
    crops = preprocess.resize_center_crop_u8_ragged(rb)
    assert not crops[1].any() and torch.equal(crops[3].cpu(), torch.from_numpy(PR.resize_center_crop(ims[3])))
    with pytest.raises(RuntimeError, match="out of bounds"):
        preprocess.check_ragged(DEV)
    preprocess.check_ragged(DEV)                     # cleared
    preprocess.resize_center_crop_u8_ragged(rb)
    torch.cuda.synchronize(DEV)
    with pytest.raises(RuntimeError, match="out of bounds"):
        preprocess.resize_center_crop_u8_ragged(r.to(DEV))
    preprocess.check_ragged(DEV)
    # refused on the host, loudly: resize < crop, bounds beyond the kernel
    with pytest.raises(_lib.TTNetError):
        _lib.check(_lib.load().ttnet_resize_center_crop_u8_ragged(
            C.c_void_p(src.data_ptr()), 100, C.c_void_p(desc.data_ptr()), 1, 500, 500, 200, 224,
            C.c_void_p(out.data_ptr()), None, None))
    with pytest.raises(_lib.TTNetError):
        _lib.check(_raw_call(src, src.numel(), desc, 30000, 30000, out, bad))


def test_graph_capture_replays_new_geometries():
    n = 6
    sizes_a = [(375, 500), (500, 333), (3000, 4000), (256, 300), (600, 800), (100, 120)]
    sizes_b = [(480, 640), (1400, 1100), (257, 4000), (300, 256), (512, 769), (2848, 4288)]
    ims_a = [resize_test_images(1, h, w, seed=i)[0] for i, (h, w) in enumerate(sizes_a)]
    ims_b = [resize_test_images(1, h, w, seed=50 + i)[0] for i, (h, w) in enumerate(sizes_b)]
    ra, rb = preprocess.pack_u8(ims_a), preprocess.pack_u8(ims_b)
    cap = max(ra.data.numel(), rb.data.numel())
    src = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    desc = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    src[:ra.data.numel()] = ra.data.to(DEV)
    desc.copy_(ra.desc)
    r = preprocess.RaggedU8(src, desc, 4000, 4288)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        preprocess.resize_center_crop_u8_ragged(r)      # warm-up
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = preprocess.resize_center_crop_u8_ragged(r)
    g.replay()
    torch.cuda.synchronize(DEV)
    for i, x in enumerate(ims_a):
        assert np.array_equal(out[i].cpu().numpy(), PR.resize_center_crop(x)), ("a", i)
    src[:rb.data.numel()] = rb.data.to(DEV)              # new geometries, same buffers, same n and bounds
    desc.copy_(rb.desc)
    g.replay()
    torch.cuda.synchronize(DEV)
    for i, x in enumerate(ims_b):
        assert np.array_equal(out[i].cpu().numpy(), PR.resize_center_crop(x)), ("b", i)
    preprocess.check_ragged(DEV)


def test_eval_forward_on_ragged_batch():
    spec, st = spec_and_state("small")
    m = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()})
    m = m.to(DEV).eval().reserve(8)
    sizes = [(375, 500), (500, 333), (1200, 900), (256, 300), (100, 120), (2848, 4288)]
    ims = [resize_test_images(1, h, w, seed=20 + i)[0] for i, (h, w) in enumerate(sizes)]
    r = preprocess.collate_u8([(x, i) for i, x in enumerate(ims)])[0].pin_memory().to(DEV, non_blocking=True)
    with torch.no_grad():
        y = preprocess.imgnet_eval_forward(m, r).cpu().numpy()
        crop = np.stack([PR.resize_center_crop(x) for x in ims])
        xf = synth.normalize_u8(np.ascontiguousarray(crop.transpose(0, 3, 1, 2)))
        want = m(torch.from_numpy(xf).to(DEV)).cpu().numpy()
    assert y.shape == (len(ims), 1000)
    assert (np.abs(y - want).max(axis=1) <= 1e-5).sum() >= len(ims) - 1      # (an image may cross a stem near tie)
