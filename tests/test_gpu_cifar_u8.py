"""GPU: the CIFAR path of TT_FHE_XSMALL_vAlexnet -- uint8 HWC input with ToTensor + Normalize folded into the stem
kernel (va_stem_u8_kernel), its plan / graph plumbing, and ``python -m scale_imagenet_amd.cifar`` end to end.

Synthetic weights and synthetic images (``synth.synth_images_u8(n, hw=(32, 32))``, borders NOT painted: saturated borders
hide a forgotten border class, see test_a_forgotten_border_would_be_seen).  The float64 oracle is ``OF.forward_valexnet`` on
double tensors, fed the float32 tensor that ToTensor + Normalize produce; its tap ``stem.pre`` is the pre-activation and a
bit may differ from ``pre >= 0`` only where ``|pre| < OB.NEAR_TIE``."""
import csv
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import ROOT, args_for, spec_and_state
from oracle import ttnet_bits as OB
from oracle import ttnet_float as OF
from scale_imagenet_amd import _lib, cifar, synth, ttnet
from scale_imagenet_amd.evaluate import evaluate

pytestmark = pytest.mark.gpu

N = 64
NORMS = {"cifar": (cifar.CIFAR_MEAN, cifar.CIFAR_STD),
         "half": ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25)),
         "totensor": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def new_model(dev, max_batch=256):
    _, st = spec_and_state("valexnet")
    m = ttnet.TT_FHE_XSMALL_vAlexnet(args_for("valexnet"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return m.to(dev).eval().reserve(max_batch)


@pytest.fixture(scope="module")
def model(dev):
    return new_model(dev).set_lanes(2)


@lru_cache(maxsize=None)
def images_u8(n, first=0):
    """Planar synthetic bytes [n, 3, 32, 32] (what the oracle normalises); ``hwc`` gives the kernel's layout."""
    a = synth.synth_images_u8(n, first=first, hw=(32, 32))
    a.setflags(write=False)
    return a


def hwc(u8, dev):
    return torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev)


def normalise(u8, norm="cifar"):
    """ToTensor + Normalize in float32, as torchvision computes them."""
    mean, std = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in NORMS[norm])
    return ((u8.astype(np.float32) / np.float32(255.0) - mean) / std).astype(np.float32)


@lru_cache(maxsize=None)
def oracle_pre(n, norm="cifar", first=0):
    """float64 ``stem.pre`` [n, 64, 10, 10] of the oracle on the normalised float32 tensor."""
    spec, st = spec_and_state("valexnet")
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in OF.to_torch_state(st).items()}
    taps = {}
    OF.forward_valexnet(torch.from_numpy(normalise(images_u8(n, first), norm)).double(), sd, spec, taps)
    pre = taps["stem.pre"].numpy()
    assert pre.dtype == np.float64 and pre.shape == (n, 64, 10, 10)
    pre.setflags(write=False)
    return pre


def near_tie_images(pre):
    return (np.abs(pre) < OB.NEAR_TIE).reshape(pre.shape[0], -1).any(axis=1)


def stem_bits(model, n):
    return OB.unpack_rows(model.read_stage("features.4", n), 10)


def check_bits(bits, pre, what):
    bad = np.argwhere(bits != (pre >= 0).astype(np.uint8))
    worst = max((abs(pre[tuple(d)]) for d in bad), default=0.0)
    print(f"{what}: {len(bad)} of {bits.size} stem bits differ from float64, largest |pre| there {worst:.2e}; "
          f"{int((np.abs(pre) < OB.NEAR_TIE).sum())} near ties in the oracle")
    assert worst < OB.NEAR_TIE, what


# ---- 1. stem bits against float64 -------------------------------------------------------------------------------------

def test_default_constants_are_cifar(dev):
    """A model that never heard of set_input_norm normalises with the reference's CIFAR constants."""
    m = new_model(dev, N)
    with torch.no_grad():
        m.forward_u8(hwc(images_u8(N), dev))
    check_bits(stem_bits(m, N), oracle_pre(N, "cifar"), "default constants")


@pytest.mark.parametrize("norm", ["half", "totensor", "cifar"])
def test_stem_bits_under_set_input_norm(model, dev, norm):
    x8 = hwc(images_u8(N), dev)
    model.set_input_norm(*NORMS[norm])
    try:
        with torch.no_grad():
            model.forward_u8(x8)
        check_bits(stem_bits(model, N), oracle_pre(N, norm), norm)
    finally:
        model.set_input_norm(*NORMS["cifar"])
    with torch.no_grad():
        model.forward_u8(x8)
    check_bits(stem_bits(model, N), oracle_pre(N, "cifar"), f"cifar again after {norm}")


def test_input_norm_drops_the_graphs_and_is_refolded(model, dev):
    """Constants set while a graph is cached: the graph goes, the next forwards use the new constants (plain and replayed)."""
    x8 = hwc(images_u8(N), dev)
    with torch.no_grad():
        for _ in range(4):
            model.forward_u8(x8)
    plan = model._any_plan()
    assert plan.query("graphs_enabled") == 1 and plan.query("graphs_cached") >= 1
    drops = plan.query("graph_drops")
    model.set_input_norm(*NORMS["half"])
    try:
        assert plan.query("graphs_cached") == 0 and plan.query("graph_drops") > drops
        with torch.no_grad():
            for _ in range(4):
                model.forward_u8(x8)
        assert plan.query("graphs_cached") == 1
        check_bits(stem_bits(model, N), oracle_pre(N, "half"), "half, replayed")
    finally:
        model.set_input_norm(*NORMS["cifar"])


# ---- 2. the test has teeth ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", ["cifar", "half"])
def test_a_forgotten_border_would_be_seen(norm):
    """The same stem in float64 with the INTERIOR constant applied everywhere (the padding taken for the byte round(255 mean)
    instead of zero in normalised space) differs from the oracle on bits outside the near-tie band, in pooled row 0 or
    column 0: the plain synthetic images do tell a kernel with border classes from one without."""
    _, st = spec_and_state("valexnet")
    T = torch.from_numpy
    w, b = st["features.0.weight"].astype(np.float64), st["features.0.bias"].astype(np.float64)
    sc, sh = OB.fold_bn(st, "features.2")
    mean, std = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in NORMS[norm])
    centre = np.round(255.0 * mean)
    cb = images_u8(N).astype(np.float64) - centre[None, :, None, None]
    wp = w / (255.0 * std)[None, :, None, None]
    k_int = b + (w * ((centre / 255.0 - mean) / std)[None, :, None, None]).sum(axis=(1, 2, 3))
    conv = F.conv2d(T(cb), T(wp), None, 1, 1) + T(k_int)[None, :, None, None]
    forgot = F.max_pool2d(F.relu(conv) * T(np.asarray(sc, np.float64))[None, :, None, None]
                          + T(np.asarray(sh, np.float64))[None, :, None, None], 3).numpy()
    pre = oracle_pre(N, norm)
    far = ((forgot >= 0) != (pre >= 0)) & (np.abs(pre) >= OB.NEAR_TIE)
    on_border = far[:, :, 0, :].sum() + far[:, :, 1:, 0].sum()
    print(f"{norm}: a stem without border classes flips {int(far.sum())} bits outside the near-tie band, {int(on_border)} of them "
          "in pooled row 0 / column 0")
    assert on_border >= 1
    assert far.sum() == on_border                         # (and nowhere else: the interior constant is right there)


# ---- 3. same logits where the bits agree; graph replay ---------------------------------------------------------------------

def test_same_logits_as_float_input_and_graph_replay(model, dev):
    pre = oracle_pre(N)
    ties = near_tie_images(pre)
    assert ties.sum() <= 2, f"{int(ties.sum())} of the {N} images hold a near tie of the oracle"
    xa, xf = hwc(images_u8(N), dev), torch.from_numpy(normalise(images_u8(N))).to(dev)
    with torch.no_grad():
        y_f = model(xf).clone()
        rows_f = model.read_stage("features.4", N).copy()
        model.set_profiling(True)                          # plain launches whatever is cached
        y_plain = model.forward_u8(xa).clone()
        rows_u = model.read_stage("features.4", N).copy()
        model.set_profiling(False)
        replays = model._any_plan().query("graph_replays")
        ys = [model.forward_u8(xa).clone() for _ in range(5)]
    plan = model._any_plan()
    assert plan.query("graphs_enabled") == 1 and plan.query("graph_replays") >= replays + 3
    for i, y in enumerate(ys):
        assert torch.equal(y, y_plain), f"call {i} of forward_u8 differs from the plain launches"
    assert np.array_equal(model.read_stage("features.4", N), rows_u)
    same = (rows_u == rows_f).reshape(N, -1).all(axis=1)
    print(f"{int((~same).sum())} images differ in features.4 between the uint8 and the float32 stem; {int(ties.sum())} hold a near tie")
    assert not (~same & ~ties).any(), "stem rows differ on an image without a near tie"
    keep = torch.from_numpy(same).to(dev)
    assert torch.equal(y_plain[keep], y_f[keep])
    check_bits(OB.unpack_rows(rows_u, 10), pre, "uint8 stem")
    # two input tensors alternating through one lane: the replayed graph reads the pointer it was given
    xb = hwc(images_u8(N, first=N), dev)
    assert xb.data_ptr() != xa.data_ptr()
    with torch.no_grad():
        model.set_profiling(True)
        yb_plain = model.forward_u8(xb).clone()
        model.set_profiling(False)
        assert not torch.equal(yb_plain, y_plain)
        replays = plan.query("graph_replays")
        for x, want in ((xb, yb_plain), (xa, y_plain), (xb, yb_plain), (xa, y_plain), (xa, y_plain)):
            assert torch.equal(model.forward_u8(x), want)
    assert plan.query("graph_replays") == replays + 5


# ---- 4. batch edges and lanes ------------------------------------------------------------------------------------------------

_ALONE = {}


def alone(model, dev):
    """Rows and logits of each of 67 images in a batch of its own (once)."""
    if not _ALONE:
        x8 = hwc(images_u8(67), dev)
        rows, logits = [], []
        with torch.no_grad():
            for i in range(67):
                logits.append(model.forward_u8(x8[i:i + 1]).cpu().numpy()[0])
                rows.append(model.read_stage("features.4", 1)[0].copy())
        _ALONE["rows"], _ALONE["logits"] = np.stack(rows), np.stack(logits)
    return _ALONE["rows"], _ALONE["logits"]


@pytest.mark.parametrize("n", [1, 7, 67])
def test_batch_edges_and_two_lanes(model, dev, n):
    rows1, logits1 = alone(model, dev)
    x8 = hwc(images_u8(67), dev)
    parts = {0: slice(0, n), 1: slice(67 - n, 67)}                          # lane -> its images
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(dev))
    for last in (0, 1):                                                      # read_stage answers for the lane used last
        out = {}
        with torch.no_grad():
            for lane in (1 - last, last):
                with torch.cuda.stream(streams[lane]):
                    out[lane] = model.forward_u8(x8[parts[lane]], lane=lane)
        torch.cuda.synchronize(dev)
        for lane in (0, 1):
            assert np.array_equal(out[lane].cpu().numpy(), logits1[parts[lane]]), (n, lane)
        assert np.array_equal(model.read_stage("features.4", n), rows1[parts[last]]), (n, last)


# ---- 5. contract ---------------------------------------------------------------------------------------------------------------

def test_input_contract(model, dev):
    u8 = images_u8(5)
    good = hwc(u8, dev)
    with torch.no_grad():
        model.forward_u8(good[:4])
        for bad in (torch.from_numpy(u8.copy()).to(dev),                                  # CHW
                    torch.zeros((4, 32, 32, 4), dtype=torch.uint8, device=dev),
                    torch.zeros((2, 224, 224, 3), dtype=torch.uint8, device=dev),
                    good.float(), good.cpu()):
            with pytest.raises(RuntimeError):
                model.forward_u8(bad)
        # the C ABI itself refuses a pointer that is not 4-byte aligned (the wrapper would have copied it)
        import ctypes as C
        plan = model._any_plan()
        out = torch.empty((4, 10), device=dev, dtype=torch.float32)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for off in (1, 2):
            with pytest.raises(_lib.TTNetError, match="aligned"):
                _lib.check(plan.lib.ttnet_forward_u8(plan.handle, 0, C.c_void_p(good.data_ptr() + off), 4, C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(stream)))
        with pytest.raises(_lib.TTNetError):
            _lib.check(plan.lib.ttnet_plan_set_input_norm(plan.handle, (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.0, 0.25)))
        assert torch.equal(model.forward_u8(good[:4]), model.forward_u8(good[:4].clone()))
    # the ImageNet models keep their own contract
    small = ttnet.TT_vf_19lv3_imgnet_xsmall(args_for("xsmall")).eval()
    with pytest.raises(RuntimeError, match="224"):
        small.forward_u8(good)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------

def test_command_end_to_end(model, dev, tmp_path):
    n = 300
    u8 = images_u8(n)
    labels = (np.arange(n) % 10).astype(np.int64)
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([labels[:, None].astype(np.uint8), u8.reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
    got_x, got_t = cifar.read_cifar10(str(tmp_path))
    assert np.array_equal(got_x, u8.transpose(0, 2, 3, 1)) and np.array_equal(got_t, labels)

    # what the float32 path says of the same images, and which images the two stems disagree on
    xf, t = torch.from_numpy(normalise(u8)), torch.from_numpy(labels)
    cuts = [(0, 128), (128, 256), (256, 300)]
    want = evaluate(model, [(xf[a:b], t[a:b]) for a, b in cuts], dev, metrics="torch")
    differ = 0
    with torch.no_grad():
        for a, b in cuts:
            model(xf[a:b].to(dev))
            rows_f = model.read_stage("features.4", b - a).copy()
            model.forward_u8(hwc(u8[a:b], dev))
            differ += int((model.read_stage("features.4", b - a) != rows_f).reshape(b - a, -1).any(axis=1).sum())
    torch.cuda.synchronize(dev)
    assert differ <= 2, f"{differ} of {n} images differ in features.4 between the uint8 and the float32 stem"

    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    per_class = tmp_path / "C.csv"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "scale_imagenet_amd.cifar", "--data_dir", str(tmp_path),
                        "--synthetic-ckpt", "--eval_batch_size", "128", "--per_class", str(per_class)],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("Acc..")]
    assert len(lines) == 1, r.stdout
    top1, top5 = map(float, re.fullmatch(r"Acc\.\. (\S+) (\S+)", lines[0]).groups())
    # the command counts hits on the device (100 * hits / 300, exact); the torch metrics average float32 batch means, so
    # the two are compared as hit counts
    hits = [v * n / 100.0 for v in (top1, top5)]
    want_hits = [v * n / 100.0 for v in (want.top1, want.top5)]
    print(f"command: Acc.. {top1} {top5}; float32 batches: {want.top1} {want.top5}; stems differ on {differ} images")
    for h, wh in zip(hits, want_hits):
        assert abs(h - round(h)) < 1e-6 and abs(wh - round(wh)) < 1e-3
        assert abs(round(h) - round(wh)) <= differ
    with open(per_class, newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 10 and sum(int(x["images"]) for x in rows) == n
    assert [int(x["images"]) for x in rows] == [30] * 10
    assert sum(int(x["hits1"]) for x in rows) == round(hits[0]) and sum(int(x["hits5"]) for x in rows) == round(hits[1])
