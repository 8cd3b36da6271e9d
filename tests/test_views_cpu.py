"""CPU: the host side of the views (include/ttnet.h: ttnet_view_desc) -- the numpy twin of the device generator against
the descriptors of tests/golden/ref_views.json (whose hashes are Pillow's own five / ten-crop sequence), make_views'
validation, the mean's arithmetic, evaluate's argument errors and the --views flag."""
import json
import os

import numpy as np
import pytest
import torch

from _util import GOLD
from scale_imagenet_amd import _lib, preprocess


def _fixture():
    with open(os.path.join(GOLD, "ref_views.json")) as f:
        return json.load(f)


def test_eval_views_host_reproduces_the_fixture_descriptors():
    fx = _fixture()
    assert fx["fields"] == list(preprocess.VIEW_FIELDS)
    assert len(fx["families"]) == 9
    for e in fx["families"]:
        for family, V in (("center", 1), ("flip", 2), ("five", 5), ("ten", 10)):
            v = preprocess.eval_views_host([(e["h"], e["w"])], family, e["resize"], e["crop"])
            rec = v.records()
            assert rec.dtype == np.int32 and rec.shape == (V, 12) and v.per_image == V
            assert rec[:, :10].tolist() == e["views"][family]["desc"], (e["h"], e["w"], family)
            assert not rec[:, 10:].any()
            assert len(e["views"][family]["sha256"]) == V
    # 375 x 500 -> 341 x 256: the margin 117 is odd, so the mirrored image's centre crop is not the mirror of the centre crop
    ten = np.array(fx["families"][0]["views"]["ten"]["desc"])
    assert ten[4, 8] == 58 and ten[9, 8] == 59 and ten[9, 1] == 1
    # 224 x 300 at resize 224: zero y margin, the five windows collapse to two distinct columns
    five = np.array(fx["families"][5]["views"]["five"]["desc"])
    assert set(five[:, 9].tolist()) == {0} and len({tuple(r) for r in five[:, 8:10].tolist()}) == 3


def test_eval_views_host_batch_order_scale_and_undecoded_images():
    sizes = [(375, 500), (0, 0), (500, 333)]
    v = preprocess.eval_views_host(sizes, "ten")
    rec = v.records()
    assert rec.shape == (30, 12)
    assert rec[:, 0].tolist() == [i for i in range(3) for _ in range(10)]        # image-major
    assert not rec[10:20, 1:].any()                                              # h = w = 0: invalid views (bw = 0)
    assert rec[20:, 1:10].tolist() == preprocess.eval_views_host([(500, 333)], "ten").records()[:, 1:10].tolist()
    # the bound the ragged centre crop sizes itself by: min(max_h, max_w) / (resize - 1)
    assert v.max_scale == 500 / 255.0                      # (max_h = max_w = 500)
    assert preprocess.eval_views_host([(100, 120)], "five").max_scale == 1.0
    assert _lib.load().ttnet_eval_views_max_scale(8192, 8192, 256) == 8192 / 255.0
    with pytest.raises(ValueError, match="views must be one of"):
        preprocess.eval_views_host(sizes, "nine")
    with pytest.raises(ValueError, match="at least crop"):
        preprocess.eval_views_host(sizes, "ten", resize=200, crop=224)


GOOD = dict(image=1, bx=2, by=3, bw=10, bh=12, nw=16, nh=9, x0=4, y0=1, flip=True)
SIZES = [(30, 40), (20, 25)]


def test_make_views_builds_descriptors_and_max_scale():
    v = preprocess.make_views([GOOD, (0, 0, 0, 0, 40, 30, 8, 8, 0, 0), dict(image=0, bx=39, by=29, bw=1, bh=1)], SIZES, crop=8)
    assert v.records().tolist() == [[1, 1, 2, 3, 10, 12, 16, 9, 4, 1, 0, 0], [0, 0, 0, 0, 40, 30, 8, 8, 0, 0, 0, 0],
                                    [0, 0, 39, 29, 1, 1, 8, 8, 0, 0, 0, 0]]
    assert v.max_scale == 40 / 8 and v.per_image is None and len(v) == 3
    assert preprocess.make_views([dict(image=0, bx=0, by=0, bw=2, bh=2)], SIZES, crop=8).max_scale == 1.0     # upscaling only
    p = v.pin_memory() if torch.cuda.is_available() else v.to("cpu")
    assert torch.equal(p.desc, v.desc) and p.max_scale == v.max_scale


@pytest.mark.parametrize("change,match", [
    (dict(image=2), "image 2 outside"), (dict(image=-1), "image -1 outside"),
    (dict(bx=-1), "box columns"), (dict(bw=0), "box columns"), (dict(bx=16), "box columns"),
    (dict(by=-1), "box rows"), (dict(bh=0), "box rows"), (dict(bh=18), "box rows"),
    (dict(nw=0), "resized size"), (dict(nh=65537), "resized size"),
    (dict(x0=-1), "window columns"), (dict(x0=9), "window columns"),
    (dict(y0=-1), "window rows"), (dict(y0=2), "window rows"),
    (dict(bw=2.5), "bw must be an int32"), (dict(nh=2 ** 31), "nh must be an int32"), (dict(zoom=2), "unknown keys"),
])
def test_make_views_rejects_every_invalid_field(change, match):
    with pytest.raises(ValueError, match=match):
        preprocess.make_views([dict(image=0, bx=0, by=0, bw=4, bh=4), {**GOOD, **change}], SIZES, crop=8)


def test_make_views_rejects_flags_records_and_counts():
    with pytest.raises(ValueError, match="flags 2"):
        preprocess.make_views([(1, 2, 2, 3, 10, 12, 16, 9, 4, 1)], SIZES, crop=8)
    with pytest.raises(ValueError, match="ten numbers"):
        preprocess.make_views([(1, 0, 2, 3)], SIZES, crop=8)
    with pytest.raises(ValueError, match="lacks"):
        preprocess.make_views([dict(image=0, bx=0, by=0, bw=4)], SIZES, crop=8)
    with pytest.raises(ValueError, match="1 to 65535"):
        preprocess.make_views([], SIZES, crop=8)
    with pytest.raises(RuntimeError, match=r"int32 \[nv, 12\]"):
        preprocess.Views(torch.zeros((3, 10), dtype=torch.int32), 1.0)
    with pytest.raises(RuntimeError, match="max_scale"):
        preprocess.Views(torch.zeros((3, 12), dtype=torch.int32), 0.5)


def test_mean_views_host_hand_case():
    # 2 images x 3 views x 2 classes; float64 sums in view order, one division, one rounding to float32
    x = np.array([[1.0, 1e8], [2.0, 1.0], [4.0, -1e8],
                  [0.1, np.nan], [0.2, 1.0], [0.3, 2.0]], dtype=np.float32)
    got = preprocess.mean_views_host(x, 3)
    assert got.dtype == np.float32 and got.shape == (2, 2)
    assert got[0, 0] == np.float32(7.0 / 3.0)
    assert got[0, 1] == np.float32(1.0 / 3.0)              # float32 sums would lose the 1.0 beside 1e8
    want = (np.float64(np.float32(0.1)) + np.float64(np.float32(0.2)) + np.float64(np.float32(0.3))) / 3.0
    assert got[1, 0] == np.float32(want)
    assert np.isnan(got[1, 1])                             # NaN propagates
    assert np.array_equal(preprocess.mean_views_host(torch.from_numpy(x), 1), x, equal_nan=True)      # V = 1 copies
    for V in (0, 4, 33):
        with pytest.raises(ValueError):
            preprocess.mean_views_host(x, V)
    with pytest.raises(RuntimeError, match="no CPU path"):
        preprocess.mean_views(torch.from_numpy(x), 3)


class _Stub(torch.nn.Module):
    def forward(self, x):
        return torch.zeros((x.shape[0], 10))

    def forward_u8(self, x, lane=0):
        return torch.zeros((x.shape[0], 10))


def test_evaluate_views_argument_errors():
    from scale_imagenet_amd.evaluate import evaluate
    cpu = torch.device("cpu")
    targets = torch.zeros(2, dtype=torch.int64)
    floats = [(torch.zeros((2, 3, 4, 4)), targets)]
    crops = [(torch.zeros((2, 224, 224, 3), dtype=torch.uint8), targets)]
    with pytest.raises(ValueError, match="views must be None"):
        evaluate(_Stub(), floats, cpu, views="center")
    with pytest.raises(ValueError, match="views must be None"):
        evaluate(_Stub(), floats, cpu, views="nine")
    with pytest.raises(ValueError, match="care"):
        evaluate(_Stub(), floats, cpu, views="ten", care={})
    with pytest.raises(RuntimeError, match="RaggedU8 or RaggedJpeg"):
        evaluate(_Stub(), floats, cpu, views="ten")
    with pytest.raises(RuntimeError, match="RaggedU8 or RaggedJpeg"):
        evaluate(_Stub(), crops, cpu, views="flip")
    assert evaluate(_Stub(), floats, cpu).images == 2       # views=None: what it was
    assert evaluate(_Stub(), crops, cpu, views=None).images == 2


def test_views_flag():
    from scale_imagenet_amd import main as M
    from scale_imagenet_amd import predict as P
    none = M.build_parser().parse_args([])
    assert none.views is None and M.views_per_image(none) == 1 and M.views_args(none) == {}
    for parser in (M.build_parser(), P.build_parser()):
        for name, V in (("flip", 2), ("five", 5), ("ten", 10)):
            a = parser.parse_args(["--views", name, "--eval_batch_size", "7"])
            assert a.views == name and M.views_per_image(a) == V and M.views_args(a) == {"views": name}
        with pytest.raises(SystemExit):
            parser.parse_args(["--views", "center"])
    with pytest.raises(SystemExit, match="--views does not go with --care_from"):
        M.views_args(M.build_parser().parse_args(["--views", "ten", "--care_from", "u.npz"]))
    assert P.build_parser().parse_args([]).views is None


def test_load_model_reserves_batch_times_views(monkeypatch):
    """main / predict size the plan for eval_batch_size * V: a plan that grew mid-run would restart the usage counters."""
    from scale_imagenet_amd import main as M
    from scale_imagenet_amd import ttnet
    seen = {}

    class Fake:
        spec = None

        def __init__(self, args):
            pass

        def load_state_dict(self, state, strict=True):
            pass

        def to(self, device):
            return self

        def eval(self):
            return self

        def reserve(self, n):
            seen["reserve"] = n
            return self

    monkeypatch.setattr(ttnet, "TT_vf_19lv3_imgnet_small", Fake)
    monkeypatch.setattr(M, "_state_dict", lambda args, spec, rank: {})
    M.load_model(M.build_parser().parse_args(["--views", "ten", "--eval_batch_size", "7"]), torch.device("cpu"), 0)
    assert seen["reserve"] == 70
    M.load_model(M.build_parser().parse_args(["--eval_batch_size", "7"]), torch.device("cpu"), 0)
    assert seen["reserve"] == 7
