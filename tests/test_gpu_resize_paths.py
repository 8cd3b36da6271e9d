"""GPU: every tap-count path of the single-size resize kernel and crops beyond 224 of the ragged / views kernel
(csrc/preproc.hip) against Pillow's own hashes (tests/golden/ref_resize_paths.json) and oracle/pil_resize.py, byte for byte.

Which template instantiation ran on an accepted geometry is INFERRED from the twins of tests/_resize_paths.py, not
observed; tests/test_resize_paths_cpu.py asserts that the case lists reach every path.  Only the refusal text of the
single-size entry point ties the twin's arithmetic to the launcher's own (test_uniform_refusal...)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _resize_paths as RP
from _util import oracle_views, sha
from scale_imagenet_amd import _lib, preprocess

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
UNSUPPORTED = -4                                           # TTNET_E_UNSUPPORTED


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, RP.first_difference(got, want))


def _fixture_uniform(c):
    return [e for e in RP.fixture()["uniform"] if (e["case"], e["h"], e["w"], e["resize"], e["crop"], e["n"]) == tuple(c)][0]


def _ragged_entry(resize, crop):
    return [e for e in RP.fixture()["ragged"] if (e["resize"], e["crop"]) == (resize, crop)][0]


@pytest.mark.parametrize("c", RP.UNIFORM_CASES, ids=lambda c: c.key)
def test_uniform_case_matches_pillow_oracle_and_ragged_entry(c):
    p = c.plan()
    assert p.accepted
    x = torch.from_numpy(np.array(c.images())).to(DEV)
    out = preprocess.resize_center_crop_u8(x, c.resize, c.crop)
    got = out.cpu().numpy()
    assert got.shape == (c.n, c.crop, c.crop, 3)
    want_sha = _fixture_uniform(c)["sha256"]
    for i, want in enumerate(RP.uniform_oracle(c)):
        _same(got[i], want, (c.key, p.name, "image", i))
        assert sha(got[i]) == want_sha[i], (c.key, p.name, i, "differs from Pillow's output")
    ragged = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8(list(c.images())).to(DEV), c.resize, c.crop)
    assert torch.equal(out, ragged), (c.key, RP.first_difference(ragged.cpu().numpy(), got))
    preprocess.check_ragged(DEV)


@pytest.mark.parametrize("c", RP.UNIFORM_REFUSED, ids=lambda c: c.key)
def test_uniform_refusal_names_the_twins_lds_bytes_and_launches_nothing(c):
    p = c.plan()
    assert not p.accepted
    x = torch.from_numpy(np.array(c.images())).to(DEV)
    out = torch.full((c.n, c.crop, c.crop, 3), 0xA5, dtype=torch.uint8, device=DEV)
    status = _lib.load().ttnet_resize_center_crop_u8(C.c_void_p(x.data_ptr()), c.n, c.h, c.w, c.resize, c.crop,
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    with pytest.raises(_lib.TTNetError) as e:
        _lib.check(status)
    torch.cuda.synchronize(DEV)
    assert e.value.status == UNSUPPORTED
    m = re.search(r"needs (\d+) bytes of LDS", str(e.value))
    assert m, str(e.value)
    assert int(m.group(1)) == p.lds, ("the launcher's LDS bytes against the twin's", str(e.value), p)
    assert bool((out == 0xA5).all()), "a refused call wrote to its output"
    with pytest.raises(_lib.TTNetError):
        preprocess.resize_center_crop_u8(x, c.resize, c.crop)
    # the ragged entry point serves the same image
    got = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8(list(c.images())).to(DEV), c.resize, c.crop).cpu().numpy()
    want_sha = _fixture_uniform(c)["sha256"]
    for i, want in enumerate(RP.uniform_oracle(c)):
        _same(got[i], want, (c.key, "ragged", i))
        assert sha(got[i]) == want_sha[i]
    preprocess.check_ragged(DEV)


@pytest.mark.parametrize("resize,crop", RP.RAGGED_PAIRS)
def test_ragged_batch_matches_pillow_and_oracle_in_any_order(resize, crop):
    ims = list(RP.ragged_images(resize))
    r = preprocess.pack_u8(ims)
    assert r.data.numel() % 16 != 0
    plan = RP.ragged_center_plan(r.max_h, r.max_w, resize, crop)
    got = preprocess.resize_center_crop_u8_ragged(r.to(DEV), resize, crop).cpu().numpy()
    assert got.shape == (len(ims), crop, crop, 3)
    want = RP.ragged_oracle(resize, crop)
    for i, e in enumerate(_ragged_entry(resize, crop)["images"]):
        _same(got[i], want[i], (resize, crop, ims[i].shape, plan))
        assert sha(got[i]) == e["sha256"], (resize, crop, i, "differs from Pillow's output")
    perm = np.random.default_rng(crop).permutation(len(ims))
    assert (perm != np.arange(len(ims))).any()
    shuffled = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8([ims[k] for k in perm]).to(DEV), resize, crop).cpu().numpy()
    for j, k in enumerate(perm):
        _same(shuffled[j], got[k], (resize, crop, "shuffled", j, int(k)))
    preprocess.check_ragged(DEV)


@pytest.mark.parametrize("resize,crop", RP.VIEW_PAIRS)
def test_views_under_wide_match_pillow_and_oracle(resize, crop):
    ims = list(RP.ragged_images(resize))
    sizes = [x.shape[:2] for x in ims]
    fx = [e for e in RP.fixture()["views"] if (e["resize"], e["crop"]) == (resize, crop)][0]
    r = preprocess.pack_u8(ims)
    assert r.data.numel() % 16 != 0
    r = r.to(DEV)
    # the ten-crop family from the device generator
    ten = preprocess.eval_views(r, "ten", resize, crop)
    host = preprocess.eval_views_host(sizes, "ten", resize, crop)
    assert np.array_equal(ten.records(), host.records()) and ten.max_scale == host.max_scale
    assert RP.ragged_plan(crop, ten.max_scale).wide
    got = preprocess.resize_views_u8_ragged(r, ten, crop).cpu().numpy()
    rec = host.records()
    assert got.shape == (10 * len(ims), crop, crop, 3)
    for i, x in enumerate(ims):
        for v, want in enumerate(oracle_views(x, rec[10 * i:10 * i + 10], crop)):
            _same(got[10 * i + v], want, (resize, crop, "ten", i, v))
            assert sha(got[10 * i + v]) == fx["ten"][10 * i + v], (resize, crop, i, v, "differs from Pillow's output")
    # CENTER views are the centre-crop call
    center = preprocess.resize_views_u8_ragged(r, preprocess.eval_views(r, "center", resize, crop), crop)
    assert torch.equal(center, preprocess.resize_center_crop_u8_ragged(r, resize, crop))
    _same(center.cpu().numpy(), np.stack(RP.ragged_oracle(resize, crop)), (resize, crop, "center"))
    _same(got[4::10], center.cpu().numpy(), (resize, crop, "view 4 of ten is the centre crop"))
    # explicit boxes with flips; the first ends on the last byte of the unaligned buffer
    boxes = RP.view_boxes(resize, crop)
    assert [tuple(d) for d in fx["boxes"]["desc"]] == boxes
    b0 = boxes[0]
    assert b0[0] == len(ims) - 1 and (b0[3] + b0[5], b0[2] + b0[4]) == sizes[-1]
    views = preprocess.make_views(boxes, sizes, crop)
    got = preprocess.resize_views_u8_ragged(r, views.to(DEV), crop).cpu().numpy()
    for k, d in enumerate(boxes):
        _same(got[k], oracle_views(ims[d[0]], [d], crop)[0], (resize, crop, "box", d))
        assert sha(got[k]) == fx["boxes"]["sha256"][k], (resize, crop, d, "differs from Pillow's output")
    preprocess.check_ragged(DEV)


def test_invalid_view_and_invalid_descriptor_under_wide():
    """Crop 344 (two dword columns per thread).  The source allocation is larger than the declared src_bytes and the output
    has a guard crop on either side: whatever a guard let through would still land in memory the test owns."""
    resize, crop = 360, 344
    ims = list(RP.ragged_images(resize))
    sizes = [x.shape[:2] for x in ims]
    r = preprocess.pack_u8(ims)
    src = torch.zeros(16 << 20, dtype=torch.uint8, device=DEV)
    assert r.data.numel() < src.numel() // 2
    src[:r.data.numel()] = r.data.to(DEV)
    idesc = r.desc.to(DEV)
    boxes = RP.view_boxes(resize, crop)
    good = preprocess.make_views(boxes[:3], sizes, crop)
    rec = good.records().copy()
    bad_view = rec[1].copy()
    bad_view[8] = bad_view[6] - crop + 1                   # the window ends one column past nw
    rows = np.stack([rec[0], bad_view, rec[1], rec[2]])
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(idesc, rows):
        vdesc = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
        out = torch.full((len(rows) + 2, crop, crop, 3), 7, dtype=torch.uint8, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.check(_lib.load().ttnet_resize_views_u8_ragged(
            C.c_void_p(src.data_ptr()), r.data.numel(), C.c_void_p(idesc.data_ptr()), len(ims), C.c_void_p(vdesc.data_ptr()),
            len(rows), float(good.max_scale), crop, C.c_void_p(out.data_ptr() + crop * crop * 3), C.c_void_p(count.data_ptr()), stream))
        got = out.cpu().numpy()
        assert (got[0] == 7).all() and (got[-1] == 7).all(), "guard crops around dst were written"
        return got[1:-1], int(count.item())

    want = [oracle_views(ims[d[0]], [d], crop)[0] for d in rec]
    got, count = call(idesc, rows)
    assert count == 1 and not got[1].any(), "an invalid view: a zero crop, counted once"
    for k, w in ((0, want[0]), (2, want[1]), (3, want[2])):
        _same(got[k], w, ("beside an invalid view", k))
    # an invalid image descriptor (its bytes end past src_bytes): its view is refused, once, the others are right
    idesc2 = idesc.clone()
    idesc2[int(rec[1, 0]), 0] = r.data.numel() - 100
    got, count = call(idesc2, rec)
    assert count == 1 and not got[1].any(), "a view of an invalid image: a zero crop, counted once"
    _same(got[0], want[0], "beside an invalid image, 0")
    _same(got[2], want[2], "beside an invalid image, 2")


def _raw_ragged(src, src_bytes, desc, max_h, max_w, resize, crop, out, bad):
    return _lib.load().ttnet_resize_center_crop_u8_ragged(
        C.c_void_p(src.data_ptr()), int(src_bytes), C.c_void_p(desc.data_ptr()), desc.shape[0], max_h, max_w, resize, crop,
        C.c_void_p(out.data_ptr()), C.c_void_p(bad.data_ptr()), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def test_ragged_bound_9274_runs_and_9275_is_refused():
    m = RP.largest_accepted_side(256, 224)                 # 9274: derived in tests/test_resize_paths_cpu.py
    assert RP.ragged_center_plan(m, m, 256, 224).accepted and not RP.ragged_center_plan(m + 1, m + 1, 256, 224).accepted
    c = [c for c in RP.UNIFORM_CASES if (c.h, c.w, c.resize, c.crop) == (512, 769, 256, 224)][0]
    x = c.images()[:1]
    r = preprocess.pack_u8(list(x)).to(DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((1, 224, 224, 3), 0xA5, dtype=torch.uint8, device=DEV)
    status = _raw_ragged(r.data, r.data.numel(), r.desc, m + 1, m + 1, 256, 224, out, bad)
    with pytest.raises(_lib.TTNetError) as e:
        _lib.check(status)
    torch.cuda.synchronize(DEV)
    assert e.value.status == UNSUPPORTED
    assert bool((out == 0xA5).all()) and int(bad.item()) == 0, "a refused call wrote to its output"
    _lib.check(_raw_ragged(r.data, r.data.numel(), r.desc, m, m, 256, 224, out, bad))
    _same(out[0].cpu().numpy(), RP.uniform_oracle(c)[0], ("declared max", m))
    assert int(bad.item()) == 0


def test_graph_capture_at_crop_384_replays_new_geometries():
    resize, crop = 438, 384
    assert RP.ragged_center_plan(1200, 1200, resize, crop).wide
    ims_a = list(RP.ragged_images(resize))
    uw = [c for c in RP.UNIFORM_CASES if c.case == "uwide"]
    ims_b = [ims_a[3], uw[0].images()[0], ims_a[0], uw[1].images()[1], ims_a[2]]
    want_b = [RP.ragged_oracle(resize, crop)[3], RP.uniform_oracle(uw[0])[0], RP.ragged_oracle(resize, crop)[0],
              RP.uniform_oracle(uw[1])[1], RP.ragged_oracle(resize, crop)[2]]
    ra, rb = preprocess.pack_u8(ims_a), preprocess.pack_u8(ims_b)
    src = torch.zeros(max(ra.data.numel(), rb.data.numel()), dtype=torch.uint8, device=DEV)
    desc = torch.zeros((len(ims_a), 2), dtype=torch.int64, device=DEV)
    src[:ra.data.numel()] = ra.data.to(DEV)
    desc.copy_(ra.desc)
    r = preprocess.RaggedU8(src, desc, 1200, 1200)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        preprocess.resize_center_crop_u8_ragged(r, resize, crop)      # warm-up
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = preprocess.resize_center_crop_u8_ragged(r, resize, crop)
    g.replay()
    torch.cuda.synchronize(DEV)
    for i, want in enumerate(RP.ragged_oracle(resize, crop)):
        _same(out[i].cpu().numpy(), want, ("a", i))
    src[:rb.data.numel()] = rb.data.to(DEV)                # new geometries, same buffers, same n and bounds
    desc.copy_(rb.desc)
    g.replay()
    torch.cuda.synchronize(DEV)
    for i, want in enumerate(want_b):
        _same(out[i].cpu().numpy(), want, ("b", i))
    preprocess.check_ragged(DEV)
