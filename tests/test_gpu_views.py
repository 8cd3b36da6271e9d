"""GPU: views of ragged batches (ttnet_resize_views_u8_ragged, ttnet_make_eval_views, ttnet_mean_views) against Pillow's
own crops (tests/golden/ref_views.json: SHA-256 of Image.crop / resize / transpose and of the five / ten-crop sequence),
oracle/pil_resize.py, the centre-crop entry point, and the multi-crop forwards up to evaluate(views=)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from _util import GOLD, args_for, jpeg_bytes, oracle_views, ragged_images, resize_test_images, sha, spec_and_state
from oracle import pil_resize as PR
from scale_imagenet_amd import _lib, jpeg, preprocess, ttnet
from scale_imagenet_amd.evaluate import evaluate, topk_rows_host

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FAMILIES = (("center", 1), ("flip", 2), ("five", 5), ("ten", 10))


def _fixture():
    with open(os.path.join(GOLD, "ref_views.json")) as f:
        return json.load(f)


def sizes_of(ims):
    return [x.shape[:2] for x in ims]


@pytest.fixture(scope="module")
def xsmall():
    _, st = spec_and_state("xsmall")
    m = ttnet.TT_vf_19lv3_imgnet_xsmall(args_for("xsmall"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return m.to(DEV).eval().reserve(64)


@pytest.mark.parametrize("crop", [8, 32, 224])
def test_fixture_views_match_pillow_and_oracle(crop):
    """Every fixture view of this crop size -- the four families of every geometry and the explicit boxes -- in ONE launch."""
    fx = _fixture()
    ims, records, want_sha = [], [], []
    for e in fx["families"]:
        if e["crop"] != crop:
            continue
        ims.append(resize_test_images(1, e["h"], e["w"], seed=e["seed"])[0])
        for family, _ in FAMILIES:
            for d, s in zip(e["views"][family]["desc"], e["views"][family]["sha256"]):
                records.append([len(ims) - 1] + d[1:])
                want_sha.append(s)
    first_box = len(ims)
    ims += [resize_test_images(1, b["h"], b["w"], seed=b["seed"])[0] for b in fx["box_images"]]       # last in the buffer
    cases = [b for b in fx["boxes"] if b["crop"] == crop]
    assert len(cases) == 1
    for d, s in zip(cases[0]["desc"], cases[0]["sha256"]):
        records.append([first_box + d[0]] + d[1:])
        want_sha.append(s)
    r = preprocess.pack_u8(ims)
    if crop == 8:                                          # one of its boxes ends on the last byte of an unaligned buffer
        assert r.data.numel() % 16 != 0
        last = records[1]
        assert last[0] == len(ims) - 1 and (last[2] + last[4], last[3] + last[5]) == ims[-1].shape[1::-1]
    views = preprocess.make_views([tuple(d) for d in records], sizes_of(ims), crop)
    got = preprocess.resize_views_u8_ragged(r.to(DEV), views.to(DEV), crop).cpu().numpy()
    preprocess.check_ragged(DEV)
    assert got.shape == (len(records), crop, crop, 3)
    for i in range(len(ims)):
        mine = [k for k, d in enumerate(records) if d[0] == i]
        for k, want in zip(mine, oracle_views(ims[i], [records[k] for k in mine], crop)):
            assert sha(got[k]) == want_sha[k], (k, records[k], "differs from Pillow's output")
            assert np.array_equal(got[k], want), (k, records[k], int(np.abs(got[k].astype(int) - want.astype(int)).max()))


def _desc_only(sizes):
    """A RaggedU8 whose descriptors name `sizes` (the generator reads nothing else)."""
    d = np.zeros(len(sizes), dtype=preprocess.DESC_DTYPE)
    d["h"], d["w"] = [s[0] for s in sizes], [s[1] for s in sizes]
    d["offset"][1:] = np.cumsum([s[0] * s[1] * 3 for s in sizes])[:-1]
    return preprocess.RaggedU8(torch.zeros(16, dtype=torch.uint8), torch.from_numpy(d.view(np.int64).reshape(-1, 2)),
                               max(1, max(s[0] for s in sizes)), max(1, max(s[1] for s in sizes))).to(DEV)


@pytest.mark.parametrize("resize,crop", [(256, 224), (224, 224), (40, 32), (41, 32)])
def test_device_generator_equals_host_twin(resize, crop):
    sizes = [(375, 500), (500, 333), (257, 300), (100, 120), (256, 256), (224, 300), (61, 47), (47, 61), (2848, 4288),
             (0, 0), (1, 8192), (8192, 1), (resize, resize), (crop, 700), (3000, 4000)]
    sizes += [(int(h), int(w)) for h, w in np.random.default_rng(resize).integers(1, 900, size=(300, 2))]     # two blocks
    r = _desc_only(sizes)
    for family, V in FAMILIES:
        dev_views = preprocess.eval_views(r, family, resize, crop)
        host = preprocess.eval_views_host(sizes, family, resize, crop)
        got = dev_views.records()
        assert got.dtype == np.int32 and got.shape == (len(sizes) * V, 12)
        assert np.array_equal(got, host.records()), (family, np.argwhere(got != host.records())[:4].tolist())
        assert dev_views.max_scale == host.max_scale and dev_views.per_image == V


def test_center_views_give_the_bytes_of_the_center_crop_call():
    sizes = [(375, 500), (500, 333), (256, 256), (100, 120), (1200, 900), (257, 4000), (600, 800), (224, 224)]
    ims = [resize_test_images(1, h, w, seed=300 + i)[0] for i, (h, w) in enumerate(sizes)]
    r = preprocess.pack_u8(ims).to(DEV)
    old = preprocess.resize_center_crop_u8_ragged(r)
    new = preprocess.resize_views_u8_ragged(r, preprocess.eval_views(r, "center"))
    assert torch.equal(old, new)
    assert np.array_equal(new[5].cpu().numpy(), PR.resize_center_crop(ims[5]))          # 33 taps horizontally, 3 vertically
    # FLIP: the centre crop, then the centre crop of the resized image mirrored (375 x 500: an odd margin, another window)
    flip = preprocess.resize_views_u8_ragged(r, preprocess.eval_views(r, "flip")).cpu().numpy()
    assert np.array_equal(flip[0::2], old.cpu().numpy())
    want = oracle_views(ims[0], preprocess.eval_views_host(sizes[:1], "flip").records(), 224)
    assert np.array_equal(flip[1], want[1]) and not np.array_equal(flip[1], flip[0][:, ::-1])
    preprocess.check_ragged(DEV)


def test_order_and_composition():
    ims = [resize_test_images(1, h, w, seed=400 + i)[0] for i, (h, w) in enumerate([(61, 47), (47, 61), (100, 120), (33, 90)])]
    r = preprocess.pack_u8(ims).to(DEV)
    host = preprocess.eval_views_host(sizes_of(ims), "ten", 40, 32)
    rec = host.records()
    base = preprocess.resize_views_u8_ragged(r, host.to(DEV), 32).cpu().numpy()
    for i, x in enumerate(ims):
        for v, want in enumerate(oracle_views(x, rec[i * 10:(i + 1) * 10], 32)):
            assert np.array_equal(base[i * 10 + v], want), (i, v)
    perm = np.random.default_rng(1).permutation(len(rec))                  # views of the four images interleaved
    shuffled = preprocess.resize_views_u8_ragged(r, preprocess.Views(torch.from_numpy(rec[perm].copy()), host.max_scale).to(DEV), 32)
    assert np.array_equal(shuffled.cpu().numpy(), base[perm])
    for k in range(len(rec)):                                              # each view alone
        one = preprocess.resize_views_u8_ragged(r, preprocess.Views(torch.from_numpy(rec[k:k + 1].copy()), host.max_scale).to(DEV), 32)
        assert np.array_equal(one[0].cpu().numpy(), base[k]), k
    repeated = preprocess.Views(torch.from_numpy(np.repeat(rec[7:8], 5, axis=0)), host.max_scale).to(DEV)     # one view five times
    assert np.array_equal(preprocess.resize_views_u8_ragged(r, repeated, 32).cpu().numpy(), np.repeat(base[7:8], 5, axis=0))
    preprocess.check_ragged(DEV)


def _raw_views(src, src_bytes, idesc, vdesc, max_scale, crop, out, bad):
    return _lib.load().ttnet_resize_views_u8_ragged(
        C.c_void_p(src.data_ptr()), int(src_bytes), C.c_void_p(idesc.data_ptr()), idesc.shape[0], C.c_void_p(vdesc.data_ptr()),
        vdesc.shape[0], float(max_scale), crop, C.c_void_p(out.data_ptr()), C.c_void_p(bad.data_ptr()) if bad is not None else None,
        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))


def test_bad_views_give_zero_crops_and_are_counted():
    """Valid calls with refused descriptors.  The source allocation is 16 MiB and the declared src_bytes far smaller, and
    the output has a guard crop on either side: whatever a guard let through would still land in memory the test owns."""
    crop = 32
    ims = [resize_test_images(1, h, w, seed=500 + i)[0] for i, (h, w) in enumerate([(100, 120), (61, 47), (90, 200)])]
    r = preprocess.pack_u8(ims)
    src = torch.zeros(16 << 20, dtype=torch.uint8, device=DEV)
    src[:r.data.numel()] = r.data.to(DEV)
    idesc = r.desc.to(DEV)
    good = [(0, 0, 10, 5, 100, 90, 50, 40, 9, 4), (1, 1, 0, 0, 47, 61, 32, 45, 0, 13), (2, 0, 100, 45, 100, 45, 64, 32, 32, 0),
            (2, 1, 0, 0, 200, 90, 100, 45, 34, 6)]
    bad = {"image index out of range": (3, 0, 0, 0, 10, 10, 32, 32, 0, 0),
           "negative image index": (-1, 0, 0, 0, 10, 10, 32, 32, 0, 0),
           "box past the image's right edge": (1, 0, 8, 0, 40, 61, 32, 45, 0, 0),
           "box past the image's last row": (1, 0, 0, 30, 47, 32, 32, 45, 0, 0),
           "empty box": (0, 0, 10, 5, 0, 90, 50, 40, 0, 0),
           "window past nw": (0, 0, 10, 5, 100, 90, 50, 40, 19, 4),
           "window past nh": (0, 0, 10, 5, 100, 90, 50, 40, 9, 9),
           "negative window": (0, 0, 10, 5, 100, 90, 50, 40, -1, 4),
           "nw = 0": (0, 0, 10, 5, 100, 90, 0, 40, 0, 4),
           "nh beyond 65536": (0, 0, 10, 5, 100, 90, 50, 65537, 9, 4),
           "scale above max_scale": (2, 0, 0, 0, 200, 90, 32, 45, 0, 6),
           "another flag bit": (0, 2, 10, 5, 100, 90, 50, 40, 9, 4)}
    rows = [list(good[0]) + [0, 0]]
    kinds = [None]
    for k, (kind, d) in enumerate(bad.items()):
        rows.append(list(d) + [0, 0])
        kinds.append(kind)
        if k % 4 == 3:
            rows.append(list(good[1 + k // 4]) + [0, 0])
            kinds.append(None)
    rows += [list(good[0]) + [1, 0], list(good[0]) + [0, -7]]
    kinds += ["reserved word 10 set", "reserved word 11 set"]
    rec = np.array(rows, dtype=np.int32)
    max_scale = 2.5                                        # the good views need 2.25 and 200 / 32 = 6.25 is refused
    vdesc = torch.from_numpy(rec).to(DEV)
    out = torch.full((len(rec) + 2, crop, crop, 3), 7, dtype=torch.uint8, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_raw_views(src, r.data.numel(), idesc, vdesc, max_scale, crop, out[1:], count))
    got = out.cpu().numpy()
    n_bad = sum(k is not None for k in kinds)
    assert n_bad == 14 and int(count.item()) == n_bad
    assert (got[0] == 7).all() and (got[-1] == 7).all(), "guard crops around dst were written"
    for k, kind in enumerate(kinds):
        if kind is not None:
            assert not got[1 + k].any(), kind
        else:
            want = oracle_views(ims[rec[k, 0]], [rec[k]], crop)[0]
            assert np.array_equal(got[1 + k], want), (k, "a good view beside bad ones")
    # an image descriptor that is itself bad (bytes past src_bytes) refuses every view of that image, once per view
    idesc2 = idesc.clone()
    idesc2[1, 0] = r.data.numel() - 100
    count.zero_()
    _lib.check(_raw_views(src, r.data.numel(), idesc2, torch.from_numpy(np.array([list(g) + [0, 0] for g in good], dtype=np.int32)).to(DEV),
                          max_scale, crop, out[1:], count))
    assert int(count.item()) == 1 and not out[2].any() and out[1].any() and out[3].any()
    # bad_dev may be NULL
    _lib.check(_raw_views(src, r.data.numel(), idesc, vdesc, max_scale, crop, out[1:], None))
    torch.cuda.synchronize(DEV)
    # the Python wrapper shares the sticky count of the centre-crop call
    rd = r.to(DEV)
    crops = preprocess.resize_views_u8_ragged(rd, preprocess.Views(vdesc, max_scale), crop)
    assert not crops[1].any() and crops[0].any()
    with pytest.raises(RuntimeError, match="out of bounds"):
        preprocess.check_ragged(DEV)
    preprocess.check_ragged(DEV)                           # cleared
    preprocess.resize_views_u8_ragged(rd, preprocess.Views(vdesc, max_scale), crop)
    torch.cuda.synchronize(DEV)
    with pytest.raises(RuntimeError, match="out of bounds"):
        preprocess.resize_center_crop_u8_ragged(rd)
    preprocess.check_ragged(DEV)
    # refused on the host, loudly, nothing launched: bounds beyond the kernel, counts, alignment
    ok = vdesc[:1]
    for kwargs in (dict(max_scale=1e5), dict(max_scale=0.5), dict(max_scale=float("nan")), dict(crop=30), dict(vdesc=vdesc[:0]),
                   dict(vdesc=torch.zeros((1, 13), dtype=torch.int32, device=DEV)[:, 1:])):
        a = dict(vdesc=ok, max_scale=max_scale, crop=crop)
        a.update(kwargs)
        with pytest.raises(_lib.TTNetError):
            _lib.check(_raw_views(src, r.data.numel(), idesc, a["vdesc"], a["max_scale"], a["crop"], out[1:], count))
    with pytest.raises(_lib.TTNetError) as e:
        _lib.check(_raw_views(src, r.data.numel(), idesc, ok, 700.0, 224, out[1:], count))       # 224 * 700 bytes per staged row
    assert e.value.status == -4                            # TTNET_E_UNSUPPORTED


def test_graph_of_generator_and_resize_replays_new_images():
    n = 4
    sizes_a = [(375, 500), (500, 333), (1200, 900), (100, 120)]
    sizes_b = [(480, 640), (256, 300), (300, 256), (1400, 1100)]
    ims_a = [resize_test_images(1, h, w, seed=600 + i)[0] for i, (h, w) in enumerate(sizes_a)]
    ims_b = [resize_test_images(1, h, w, seed=650 + i)[0] for i, (h, w) in enumerate(sizes_b)]
    ra, rb = preprocess.pack_u8(ims_a), preprocess.pack_u8(ims_b)
    src = torch.zeros(max(ra.data.numel(), rb.data.numel()), dtype=torch.uint8, device=DEV)
    desc = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    src[:ra.data.numel()] = ra.data.to(DEV)
    desc.copy_(ra.desc)
    r = preprocess.RaggedU8(src, desc, 1400, 1100)

    def both():
        return preprocess.resize_views_u8_ragged(r, preprocess.eval_views(r, "ten"))

    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        both()                                             # warm-up
    torch.cuda.current_stream(DEV).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = both()
    for ims, rr in ((ims_a, None), (ims_b, rb)):
        if rr is not None:                                 # new images of new sizes, same buffers
            src[:rr.data.numel()] = rr.data.to(DEV)
            desc.copy_(rr.desc)
        g.replay()
        torch.cuda.synchronize(DEV)
        got = out.cpu().numpy()
        rec = preprocess.eval_views_host(sizes_of(ims), "ten").records()
        for i, x in enumerate(ims):
            for v, want in enumerate(oracle_views(x, rec[i * 10:(i + 1) * 10], 224)):
                assert np.array_equal(got[i * 10 + v], want), (i, v)
    preprocess.check_ragged(DEV)


@pytest.mark.parametrize("V", [1, 2, 5, 10])
@pytest.mark.parametrize("n_classes", [10, 1000])
def test_mean_views_bit_equal_to_host(V, n_classes):
    rng = np.random.default_rng(V * 1000 + n_classes)
    x = (rng.standard_normal((7 * V, n_classes)) * 10.0 ** rng.integers(-3, 6, size=(7 * V, 1))).astype(np.float32)
    want = preprocess.mean_views_host(x, V)
    got = preprocess.mean_views(torch.from_numpy(x).to(DEV), V).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (7, n_classes)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if V == 1:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))      # a copy
    x[V - 1, 3] = np.nan
    x[2 * V, 0] = np.inf
    got = preprocess.mean_views(torch.from_numpy(x).to(DEV), V).cpu().numpy()
    assert np.isnan(got[0, 3]) and got[2, 0] == np.inf
    assert np.array_equal(got, preprocess.mean_views_host(x, V), equal_nan=True)
    for bad_v in (0, 33, 3):                               # 7 rows are no multiple of 3
        with pytest.raises(ValueError):
            preprocess.mean_views(torch.from_numpy(x[:7]).to(DEV), bad_v)


SIZES6 = [(375, 500), (500, 333), (256, 300), (100, 120), (1200, 900), (61, 47)]


def _images6(seed):
    return [resize_test_images(1, h, w, seed=seed + i)[0] for i, (h, w) in enumerate(SIZES6)]


def test_ten_crop_forward_is_the_mean_of_the_crops_forwards(xsmall):
    m = xsmall
    ims = _images6(700)
    r = preprocess.pack_u8(ims).to(DEV)
    with torch.no_grad():
        got = preprocess.imgnet_views_forward(m, r, "ten").cpu().numpy()
        crops = preprocess.resize_views_u8_ragged(r, preprocess.eval_views(r, "ten"))
        rows = m.forward_u8(crops)
        assert got.shape == (6, m.spec.n_classes) and rows.shape[0] == 60
        want = preprocess.mean_views_host(rows, 10)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        alone = torch.cat([m.forward_u8(crops[k:k + 1]) for k in range(60)])
        assert torch.equal(rows, alone), "a crop's logits depend on its batch"
        center = preprocess.imgnet_views_forward(m, r, "center")
        assert torch.equal(center, preprocess.imgnet_eval_forward(m, r))
        flip = preprocess.imgnet_views_forward(m, r, "flip").cpu().numpy()
        assert np.array_equal(flip, preprocess.mean_views_host(rows.view(6, 10, -1)[:, [4, 9]].reshape(12, -1), 2))
    assert not np.array_equal(got, center.cpu().numpy())
    rec = preprocess.eval_views_host(SIZES6, "ten").records()
    assert np.array_equal(crops[50:].cpu().numpy(), np.stack(oracle_views(ims[5], rec[50:], 224)))
    preprocess.check_ragged(DEV)
    m.check_range()


JPEG_FILES = ["s420_q90_375x500_c", "s420_q90_500x375_a", "s444_q100_57x43", "grey_q90_530x270"]


def test_jpeg_views_forward_decodes_once_and_means(xsmall):
    m = xsmall
    rj = jpeg.pack_jpeg([jpeg_bytes(name) for name in JPEG_FILES]).to(DEV)
    with torch.no_grad():
        got = jpeg.jpeg_views_forward(m, rj, "ten").cpu().numpy()
        decoded = jpeg.decode_ragged(rj)
        crops = preprocess.resize_views_u8_ragged(decoded, preprocess.eval_views(decoded, "ten"))
        want = preprocess.mean_views_host(m.forward_u8(crops), 10)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert torch.equal(jpeg.jpeg_views_forward(m, rj, "center"), jpeg.jpeg_eval_forward(m, rj))
    ims = ragged_images(decoded)
    rec = preprocess.eval_views_host(sizes_of(ims), "ten").records()
    assert np.array_equal(crops[20:30].cpu().numpy(), np.stack(oracle_views(ims[2], rec[20:30], 224)))      # 57 x 43, upscaled
    jpeg.check_jpeg(DEV)
    preprocess.check_ragged(DEV)


def test_evaluate_with_views_matches_a_hand_rolled_loop(xsmall):
    m = xsmall
    batches = []
    for b, cut in enumerate((slice(0, 4), slice(2, 6))):
        ims = _images6(800 + 10 * b)[cut]
        batches.append((preprocess.pack_u8(ims), torch.tensor([(37 * (b * 4 + i)) % 1000 for i in range(len(ims))], dtype=torch.int64)))
    n, V = 8, 10
    res = evaluate(m, batches, DEV, views="ten", topk=5, table_usage=True)
    # by hand: the same forwards with the usage added after each, torch metrics as the reference accumulates them
    m.set_lanes(1)
    m.reset_table_usage()
    logits, loss_sum = [], 0.0
    with torch.no_grad():
        for r, t in batches:
            y = preprocess.imgnet_views_forward(m, r.to(DEV), "ten")
            m.add_table_usage(0)
            logits.append(y.cpu())
            loss_sum += torch.nn.functional.cross_entropy(y, t.to(DEV)).item() * len(t)
    usage = m.table_usage()
    m.count_table_usage(False)
    y, t = torch.cat(logits), torch.cat([t for _, t in batches])
    pred = topk_rows_host(y, 5)
    assert res.images == n
    assert np.array_equal(res.predictions.classes, pred.classes) and np.array_equal(res.predictions.logit, pred.logit)
    assert res.top1 == pytest.approx(100.0 * float((pred.classes[:, 0] == t.numpy()).mean()), abs=1e-9)
    assert res.top5 == pytest.approx(100.0 * float((pred.classes == t.numpy()[:, None]).any(axis=1).mean()), abs=1e-9)
    assert res.loss == pytest.approx(loss_sum / n, rel=1e-12)
    assert sorted(res.table_usage) == sorted(usage)
    for name in usage:
        assert np.array_equal(res.table_usage[name], usage[name]), name
    for blk in m.spec.blocks:                              # every one of the n * V crops is counted
        h, w = blk.in_hw
        for b in (blk.conv1, blk.conv2, blk.conv3):
            ho, wo = b.out_hw(h, w)
            assert (res.table_usage[b.name].sum(axis=1) == n * V * ho * wo).all(), b.name
        ho, wo = blk.out_hw
        assert (res.table_usage[blk.convf.name].sum(axis=1) == n * V * ho * wo).all(), blk.convf.name
    # device metrics, two batches in flight, and no views: the existing path is what it was
    res2 = evaluate(m, batches, DEV, views="ten", topk=5, inflight=2, metrics="device")
    assert np.array_equal(res2.predictions.classes, pred.classes) and (res2.top1, res2.top5) == (res.top1, res.top5)
    plain = evaluate(m, batches, DEV, topk=5)
    with torch.no_grad():
        center = torch.cat([preprocess.imgnet_eval_forward(m, r.to(DEV)).cpu() for r, _ in batches])
    assert np.array_equal(plain.predictions.logit, topk_rows_host(center, 5).logit)
    with pytest.raises(RuntimeError, match="RaggedU8 or RaggedJpeg"):
        evaluate(m, [(torch.zeros((2, 224, 224, 3), dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))], DEV, views="five")
