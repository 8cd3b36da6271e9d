"""GPU: ttnet_eval_metrics (csrc/metrics.hip) against numpy float64, its documented edge rules, accumulation and
determinism; evaluate(metrics="device") against the torch path on the real model and across the three batch types;
and the command, single process and self-launched over two ranks."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import GOLD, ROOT, args_for, golden_npz, spec_and_state
from scale_imagenet_amd import _lib, jpeg as J, preprocess, synth, ttnet
from scale_imagenet_amd.evaluate import DeviceMetrics, evaluate

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
INT32_MAX = 2 ** 31 - 1


# ---- numpy float64 reference: the rules of include/ttnet.h -----------------------------------------------------------

def _np_loss(v, t):
    v = v.astype(np.float64)
    m = v.max()
    return np.log(np.exp(v - m).sum()) + m - v[t]


def _np_rank(v, t):
    return int((v > v[t]).sum() + (v[:t] == v[t]).sum())


def _run(logits, targets, dm=None, lane=0):
    """One ttnet_eval_metrics call through DeviceMetrics; returns (dm, per-image loss, per-image rank) on the host."""
    dm = dm or DeviceMetrics(DEV, 1)
    x = logits if isinstance(logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(logits)).to(DEV)
    t = targets if isinstance(targets, torch.Tensor) else torch.from_numpy(np.asarray(targets, dtype=np.int64)).to(DEV)
    loss, rank = dm.update(x, t, lane, per_image=True)
    return dm, loss.cpu().numpy(), rank.cpu().numpy()


def _acc(dm):
    """The raw accumulators: (loss_sum float64 [lanes], int64 [lanes, 4] images / hits1 / hits5 / bad_targets)."""
    torch.cuda.synchronize(DEV)
    host = dm.acc.cpu()
    return host[:, 0].view(torch.float64).numpy().copy(), host[:, 1:5].numpy().copy()


def _model(variant="small", max_batch=256):
    cls = {"small": ttnet.TT_vf_19lv3_imgnet_small}[variant]
    _, st = spec_and_state(variant)
    model = cls(args_for(variant))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return model.to(DEV).eval().reserve(max_batch)


# ---- 4. the kernel against float64 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["small", "full", "valexnet"])
def test_kernel_against_float64(variant):
    g = golden_npz(variant)
    v = g["logits"]
    n, c = v.shape
    for i in range(n):
        assert len(np.unique(v[i])) == c, f"row {i} of ref_{variant} has a duplicate logit"       # the precondition
    order = np.argsort(-v, axis=1, kind="stable")
    targets = np.array([order[i, i % 8] for i in range(n)], dtype=np.int64)          # ranks 0..7: hits and misses for both k
    dm, loss, rank = _run(v, targets)
    want_rank = np.array([_np_rank(v[i], targets[i]) for i in range(n)])
    want_loss = np.array([_np_loss(v[i], targets[i]) for i in range(n)])
    print(f"{variant}: rank {rank.tolist()}, max |loss - float64| {np.abs(loss - want_loss).max():.3e}")
    assert want_rank.tolist() == [i % 8 for i in range(n)]
    assert rank.tolist() == want_rank.tolist()
    assert np.abs(loss - want_loss).max() <= 1e-9
    loss_sum, ints = _acc(dm)
    assert ints[0].tolist() == [n, int((want_rank < 1).sum()), int((want_rank < 5).sum()), 0]
    assert abs(loss_sum[0] - want_loss.sum()) <= 1e-9 * n
    res = dm.result()
    assert res.images == n and res.top1 == 100.0 * (want_rank < 1).sum() / n and res.top5 == 100.0 * (want_rank < 5).sum() / n
    # the fixtures' own targets: the loss the reference captured
    own = synth.synth_targets(n, n_classes=c)
    dm2, _, _ = _run(v, own)
    loss_sum2, _ = _acc(dm2)
    print(f"{variant}: loss {loss_sum2[0] / n!r} vs the reference's {float(g['loss'])!r}")
    assert abs(loss_sum2[0] / n - float(g["loss"])) < 1e-5


# ---- 5. the documented edge rules -------------------------------------------------------------------------------------

def test_tie_across_the_fifth_place_goes_to_the_lower_index():
    v = np.full((3, 16), -1.0, dtype=np.float32)
    v[:, 0:4] = [9.0, 8.0, 7.0, 6.0]                 # four larger values
    v[:, [5, 9, 12]] = 5.0                           # three tied for places 5, 6, 7
    targets = [5, 9, 12]
    dm, _, rank = _run(v, targets)
    assert rank.tolist() == [4, 5, 6] == [_np_rank(v[i], targets[i]) for i in range(3)]
    _, ints = _acc(dm)
    assert ints[0].tolist() == [3, 0, 1, 0]          # only the lowest index of the tie is a top-5 hit
    # ref_xsmall has a row with a duplicated logit: whatever it is, the rule holds on every element of that row
    g = golden_npz("xsmall")["logits"]
    row = next(r for r in g if len(np.unique(r)) < len(r))
    targets = np.arange(len(row), dtype=np.int64)
    _, _, rank = _run(np.repeat(row[None], len(row), axis=0), targets)
    assert rank.tolist() == [_np_rank(row, t) for t in targets]


def test_nan_row_gives_nan_loss_and_no_hit():
    v = golden_npz("small")["logits"][:3].copy()
    t = v.argmax(1).astype(np.int64)
    v[1, 777] = np.nan
    dm, loss, rank = _run(v, t)
    assert rank.tolist() == [0, INT32_MAX, 0]
    assert np.isnan(loss[1]) and np.isfinite(loss[[0, 2]]).all()
    loss_sum, ints = _acc(dm)
    assert np.isnan(loss_sum[0]) and ints[0].tolist() == [3, 2, 2, 0]
    # the NaN at the target itself
    v2 = v.copy()
    v2[1, 777] = 0.0
    v2[1, t[1]] = np.nan
    _, loss, rank = _run(v2, t)
    assert np.isnan(loss[1]) and rank[1] == INT32_MAX


def test_targets_out_of_range_are_counted_and_change_nothing_else():
    v = golden_npz("small")["logits"]
    n, c = v.shape
    t = v.argmax(1).astype(np.int64)
    t[[2, 3]] = np.argsort(-v[[2, 3]], axis=1)[:, 3]                 # two top-5-only hits
    keep = [0, 1, 2, 4, 6, 7]
    dm_ref, _, _ = _run(v[keep], t[keep])
    bad = t.copy()
    bad[3], bad[5] = -1, c
    dm, loss, rank = _run(v, bad)
    assert rank[[3, 5]].tolist() == [-1, -1] and loss[[3, 5]].tolist() == [0.0, 0.0]
    loss_sum, ints = _acc(dm)
    ref_sum, ref_ints = _acc(dm_ref)
    assert ints[0].tolist() == ref_ints[0][:3].tolist() + [2]
    assert abs(loss_sum[0] - ref_sum[0]) <= 1e-9
    with pytest.raises(RuntimeError, match="2 target"):
        dm.result()
    # far out of range: still no read outside the row
    _, _, rank = _run(v, np.array([2 ** 40, -2 ** 40, 2 ** 31, -2 ** 31, 1000, -1, 65536, 2 ** 32 + 5], dtype=np.int64))
    assert rank.tolist() == [-1] * 8


@pytest.mark.parametrize("n_classes", [2, 10, 1000, 1001, 65536])
@pytest.mark.parametrize("n", [1, 255, 4096])
def test_shapes_odd_tails_and_unaligned_pitch(n_classes, n):
    gen = torch.Generator(device=DEV).manual_seed(n_classes * 7 + n)
    x = torch.randn((n, n_classes), device=DEV, generator=gen) * 3.0
    x = (x * 64).round() / 64                                      # a coarse grid: ties do occur
    t = torch.randint(0, n_classes, (n,), device=DEV, generator=gen)
    dm, loss, rank = _run(x, t)
    x64 = x.double()
    vt = x64.gather(1, t[:, None])
    want_loss = (torch.logsumexp(x64, dim=1) - vt[:, 0]).cpu().numpy()
    before = torch.arange(n_classes, device=DEV)[None, :] < t[:, None]
    want_rank = ((x64 > vt).sum(1) + ((x64 == vt) & before).sum(1)).cpu().numpy()
    print(f"n_classes {n_classes} n {n}: max |loss - float64| {np.abs(loss - want_loss).max():.3e}")
    assert np.array_equal(rank, want_rank)
    assert np.abs(loss - want_loss).max() <= 1e-9
    loss_sum, ints = _acc(dm)
    assert ints[0].tolist() == [n, int((want_rank < 1).sum()), int((want_rank < 5).sum()), 0]
    assert abs(loss_sum[0] - want_loss.sum()) <= 1e-9 * n
    if n_classes % 4:                                              # a view that starts off 16 bytes as well
        y = torch.empty(n * n_classes + 1, device=DEV)[1:].view(n, n_classes).copy_(x)
        _, loss2, rank2 = _run(y, t)
        assert np.array_equal(rank2, rank) and np.abs(loss2 - want_loss).max() <= 1e-9


def test_bad_arguments_are_refused():
    lib = _lib.load()
    x = torch.zeros((4, 8), device=DEV)
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    acc = torch.zeros(8, dtype=torch.int64, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())      # noqa: E731
    for n, c in [(0, 8), (65536, 8), (4, 1), (4, 65537)]:
        assert lib.ttnet_eval_metrics(p(x), p(t), n, c, p(acc), None, None) == -1
    assert lib.ttnet_eval_metrics(None, p(t), 4, 8, p(acc), None, None) == -1
    # no per-image buffer: the library's scratch for this accumulator
    _lib.check(lib.ttnet_eval_metrics(p(x), p(t), 4, 8, p(acc), None, None))
    torch.cuda.synchronize(DEV)
    host = acc.cpu()
    assert host[1:5].tolist() == [4, 4, 4, 0] and abs(host[:1].view(torch.float64).item() - 4 * np.log(8.0)) < 1e-9


# ---- 6. accumulation and determinism ----------------------------------------------------------------------------------

def test_accumulation_determinism_and_graph_replay():
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((256, 1000), device=DEV, generator=gen) * 2.0
    t = x.argsort(dim=1, descending=True)[torch.arange(256, device=DEV), torch.arange(256, device=DEV) % 8].contiguous()

    def one():
        dm = DeviceMetrics(DEV, 1)
        dm.update(x, t, 0)
        return _acc(dm)

    def three():
        dm = DeviceMetrics(DEV, 1)
        for a, b in [(0, 100), (100, 200), (200, 256)]:
            dm.update(x[a:b], t[a:b], 0)
        return _acc(dm)

    vt = x.gather(1, t[:, None])
    before = torch.arange(1000, device=DEV)[None, :] < t[:, None]
    rank = (x > vt).sum(1) + ((x == vt) & before).sum(1)
    h1, h5 = int((rank < 1).sum()), int((rank < 5).sum())
    assert 0 < h1 < h5 < 256
    l1, i1 = one()
    l3, i3 = three()
    assert i1[0].tolist() == [256, h1, h5, 0] and np.array_equal(i1, i3)
    assert abs(l1[0] - l3[0]) <= 1e-9
    for f, (l, i) in [(one, (l1, i1)), (three, (l3, i3))]:
        for _ in range(2):
            l2, i2 = f()
            assert l2.tobytes() == l.tobytes() and i2.tobytes() == i.tobytes()

    dm = DeviceMetrics(DEV, 1)
    rec = torch.empty((256, 2), dtype=torch.int64, device=DEV)
    lib = _lib.load()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _lib.check(lib.ttnet_eval_metrics(C.c_void_p(x.data_ptr()), C.c_void_p(t.data_ptr()), 256, 1000,
                                              C.c_void_p(dm.acc.data_ptr()), C.c_void_p(rec.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)))
    torch.cuda.synchronize(DEV)
    assert _acc(dm)[1][0].tolist() == [0, 0, 0, 0]                 # capturing ran nothing
    for _ in range(3):
        graph.replay()
    lg, ig = _acc(dm)
    assert ig[0].tolist() == [3 * 256, 3 * h1, 3 * h5, 0]
    assert abs(lg[0] - 3 * l1[0]) <= 1e-9 * 3


# ---- 7. evaluate(metrics="device") equals metrics="torch" on the real model ----------------------------------------

def test_evaluate_device_equals_torch_on_tt_small():
    model = _model("small")
    x = torch.from_numpy(synth.synth_images(600))
    with torch.no_grad():
        y = torch.cat([model(x[a:b].to(DEV)).cpu() for a, b in [(0, 256), (256, 512), (512, 600)]])
    order = y.argsort(dim=1, descending=True)
    t = order[torch.arange(600), torch.arange(600) % 8].contiguous()             # ranks 0..7, as in the kernel test
    tied = [i for i in range(600) if (y[i] == y[i, t[i]]).sum() > 1]
    print(f"{len(tied)} of 600 targets share their logit with another class")
    batches = [(x[0:256], t[0:256]), (x[256:512], t[256:512]), (x[512:], t[512:])]
    for inflight in (1, 2):
        a = evaluate(model, batches, DEV, inflight=inflight, metrics="torch")
        b = evaluate(model, batches, DEV, inflight=inflight, metrics="device")
        print(f"inflight {inflight}: torch {a}, device {b}, loss difference {abs(a.loss - b.loss):.3e}")
        assert a.images == b.images == 600
        assert b.parts.hits1 == round(a.top1 * 6) and b.parts.hits5 == round(a.top5 * 6)
        assert abs(a.top1 - b.top1) < 1e-9 and abs(a.top5 - b.top5) < 1e-9
        assert 0 < b.parts.hits1 < b.parts.hits5 < 600
        if not tied:
            assert b.parts.hits1 == 75 and b.parts.hits5 == 375
        assert abs(a.loss - b.loss) < 1e-5


# ---- 8. batch types ---------------------------------------------------------------------------------------------------

def _fixture_files():
    with open(os.path.join(GOLD, "ref_jpeg.json")) as f:
        names = [e["name"] for e in json.load(f)["images"]]
    return [os.path.join(GOLD, "jpeg", n + ".jpg") for n in names]


def _pillow(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def test_three_batch_types_give_the_same_bits():
    model = _model("small", 64)
    files = _fixture_files()
    assert len(files) >= 39
    data = [open(f, "rb").read() for f in files]
    pil = [_pillow(f) for f in files]
    with torch.no_grad():
        crops = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8(pil).to(DEV))
        y = model.forward_u8(crops).cpu()
    crops = crops.cpu()
    t = y.argsort(dim=1, descending=True)[torch.arange(len(files)), torch.arange(len(files)) % 8].contiguous()
    cuts = [(0, 16), (16, 32), (32, len(files))]
    as_jpeg = [J.collate_jpeg([(data[i], int(t[i])) for i in range(a, b)]) for a, b in cuts]
    as_u8 = [preprocess.collate_u8([(pil[i], int(t[i])) for i in range(a, b)]) for a, b in cuts]
    as_crop = [(crops[a:b], t[a:b]) for a, b in cuts]
    assert isinstance(as_jpeg[0][0], J.RaggedJpeg) and isinstance(as_u8[0][0], preprocess.RaggedU8)
    kinds = np.concatenate([b[0].descriptors()["kind"] for b in as_jpeg])
    assert (kinds == 0).sum() >= 30 and (kinds == 1).sum() >= 2            # device-decoded and fallback files
    res = [evaluate(model, b, DEV, inflight=2, metrics="device") for b in (as_jpeg, as_u8, as_crop)]
    for r in res:
        print(r, r.parts)
    n = len(files)
    assert 0 < res[0].parts.hits1 < res[0].parts.hits5 < n
    for r in res[1:]:
        assert (r.parts.images, r.parts.hits1, r.parts.hits5) == (res[0].parts.images, res[0].parts.hits1, res[0].parts.hits5)
        assert np.float64(r.parts.loss_sum).tobytes() == np.float64(res[0].parts.loss_sum).tobytes()
    assert res[0].images == n


def test_a_corrupt_file_makes_evaluate_raise():
    model = _model("small", 64)
    files = _fixture_files()[:6]
    data = [open(f, "rb").read() for f in files]
    big = open(os.path.join(GOLD, "jpeg", "s420_q90_500x375_b.jpg"), "rb").read()
    s0 = J.parse_header(big).scan_offset
    data[3] = big[: s0 + (len(big) - s0) // 2]                                # a truncated scan
    batches = [J.collate_jpeg([(d, 0) for d in data])]
    with pytest.raises(RuntimeError, match="corrupt"):
        evaluate(model, batches, DEV, metrics="device")
    J.check_jpeg(DEV)                                                        # (the count was cleared by the raise)
    good = [J.collate_jpeg([(d, 0) for d in data[:3]])]
    assert evaluate(model, good, DEV, metrics="device").images == 3


# ---- 9. the command ---------------------------------------------------------------------------------------------------

def _acc_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("Acc..")]
    assert len(lines) == 1, stdout
    m = re.fullmatch(r"Acc\.\. (\S+) (\S+)", lines[0])
    return float(m.group(1)), float(m.group(2))


def test_command_single_process_and_two_ranks(tmp_path):
    files = _fixture_files()
    val = tmp_path / "data" / "val"
    for c in ("n01", "n02"):
        (val / c).mkdir(parents=True)
    for i, f in enumerate(files):                                             # two classes: indices 0 and 1
        dst = val / ("n01" if i % 3 else "n02") / os.path.basename(f)
        dst.write_bytes(open(f, "rb").read())
    _, st = spec_and_state("small")
    ckpt = tmp_path / "synthetic.pth"
    torch.save({"model_state_dict": {"module." + k: torch.from_numpy(v.copy()) for k, v in st.items()}}, str(ckpt))

    folder = J.FileBytesFolder(str(val))
    assert len(folder) == len(files) and folder.classes == ["n01", "n02"]
    loader = torch.utils.data.DataLoader(folder, batch_size=16, collate_fn=J.collate_jpeg)
    want = evaluate(_model("small", 64), loader, DEV, inflight=2, metrics="device")
    torch.cuda.synchronize(DEV)

    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p),
               TTNET_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    base = ["timeout", "-k", "10", "600", sys.executable, "-m", "scale_imagenet_amd.main", "--data_dir", str(tmp_path / "data"),
            "--ckpt", str(ckpt), "--eval_batch_size", "16", "--num_workers", "2", "--log_interval", "0"]
    for extra in (["--gpu", "0"], ["--gpus", "2"], ["--gpu", "0", "--input", "pillow"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, (extra, r.returncode, r.stderr[-3000:])      # (stops at the first failure)
        got = _acc_line(r.stdout)
        print(extra, got, (want.top1, want.top5))
        assert got == (want.top1, want.top5), (extra, r.stdout, r.stderr[-2000:])
