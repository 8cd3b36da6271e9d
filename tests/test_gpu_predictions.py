"""GPU: ttnet_topk_rows and ttnet_class_counts (csrc/metrics.hip) against the numpy statement of their rules, their
agreement with ttnet_eval_metrics bit for bit, refusal of bad arguments, graph replay; evaluate(topk, per_class) across
the batch types and lane counts; and both commands, single process and self-launched over two ranks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import golden_npz, spec_and_state, ROOT
from scale_imagenet_amd import _lib, jpeg as J, preprocess, report, synth
from scale_imagenet_amd.evaluate import DeviceMetrics, Predictions, evaluate, topk_rows
from test_gpu_eval_metrics import DEV, _acc, _acc_line, _fixture_files, _model, _pillow
from test_predictions_cpu import _np_topk

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _topk(logits, k) -> Predictions:
    rec = topk_rows(_dev(logits, np.float32), k)
    torch.cuda.synchronize(DEV)
    return Predictions.from_records(rec.cpu().numpy())


def _check_against_numpy(v, k, got: Predictions, what=""):
    worst = 0.0
    for i in range(v.shape[0]):
        c, l, p = _np_topk(v[i], k)
        assert got.classes[i].tolist() == c.tolist(), (what, i)
        assert np.array_equal(got.logit[i], l, equal_nan=True), (what, i)
        if np.isnan(p).all():
            assert np.isnan(got.logprob[i]).all(), (what, i)
        else:
            fin = np.isfinite(p)
            assert np.array_equal(got.logprob[i][~fin], p[~fin]), (what, i)       # -inf stays -inf
            if fin.any():
                worst = max(worst, float(np.abs(got.logprob[i][fin] - p[fin]).max()))
    print(f"{what} k {k}: max |logprob - float64| {worst:.3e}")
    assert worst <= 1e-9
    return worst


# ---- the kernel against the rules ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["small", "full", "valexnet"])
def test_kernel_against_np_topk_on_the_golden_logits(variant):
    v = golden_npz(variant)["logits"]
    n, c = v.shape
    assert c in (1000, 10)
    for k in sorted({1, 5, min(10, c), min(32, c)}):
        _check_against_numpy(v, k, _topk(v, k), f"ref_{variant}")


@pytest.mark.parametrize("n_classes", [2, 10, 1000, 1001, 65536])
@pytest.mark.parametrize("n", [1, 255, 4096])
def test_shapes_odd_tails_and_unaligned_pitch(n_classes, n):
    gen = torch.Generator(device=DEV).manual_seed(n_classes * 7 + n)
    x = torch.randn((n, n_classes), device=DEV, generator=gen) * 3.0
    x = (x * 64).round() / 64                                      # a coarse grid: ties do occur
    k = min(5, n_classes)
    got = _topk(x, k)
    # the rules, vectorised in float64 on the device: a stable descending sort is "larger first, lower index first"
    order = torch.sort(x, dim=1, descending=True, stable=True).indices[:, :k]
    want_lp = torch.log_softmax(x.double(), dim=1).gather(1, order).cpu().numpy()
    assert np.array_equal(got.classes, order.cpu().numpy().astype(np.int32))
    assert np.array_equal(got.logit, x.gather(1, order).cpu().numpy())
    worst = np.abs(got.logprob - want_lp).max()
    print(f"n_classes {n_classes} n {n}: max |logprob - float64| {worst:.3e}")
    assert worst <= 1e-9
    rows = [0, n // 2, n - 1]                                      # and the python statement itself on a few rows
    _check_against_numpy(x[rows].cpu().numpy(), k, Predictions(got.classes[rows], got.logit[rows], got.logprob[rows]))
    if n_classes % 4:                                              # a view whose rows start at 4-byte, not 16-byte addresses
        y = torch.empty(n * n_classes + 1, device=DEV)[1:].view(n, n_classes).copy_(x)
        assert y.data_ptr() % 16 == 4
        got2 = _topk(y, k)
        assert got2.classes.tobytes() == got.classes.tobytes() and got2.logit.tobytes() == got.logit.tobytes()
        assert np.abs(got2.logprob - want_lp).max() <= 1e-9


def test_ties_infinities_and_nan():
    v = np.full((3, 16), -1.0, dtype=np.float32)
    v[:, 0:4] = [9.0, 8.0, 7.0, 6.0]                 # four larger values
    v[:, [5, 9, 12]] = 5.0                           # three tied across the fifth place
    got = _topk(v, 7)
    assert got.classes[0].tolist() == [0, 1, 2, 3, 5, 9, 12]
    _check_against_numpy(v, 7, got, "tie across the fifth place")
    assert _topk(v, 5).classes[:, 4].tolist() == [5, 5, 5]
    for c, k in [(16, 16), (1000, 32), (1001, 5), (5000, 32)]:     # an all-equal row: classes 0 .. k-1
        flat = np.full((2, c), 0.25, dtype=np.float32)
        got = _topk(flat, k)
        assert got.classes.tolist() == [list(range(k))] * 2
        assert np.abs(got.logprob + np.log(float(c))).max() <= 1e-9
    g = golden_npz("xsmall")["logits"]
    row = next(r for r in g if len(np.unique(r)) < len(r))         # the duplicated logit of ref_xsmall
    k = min(len(row), 32)
    _check_against_numpy(row[None], k, _topk(np.repeat(row[None], 3, axis=0), k), "ref_xsmall duplicate")
    w = golden_npz("small")["logits"][:4].copy()
    w[0, [3, 500, 999]] = -np.inf
    w[1, :] = -np.inf
    w[1, [7, 8]] = [1.0, 1.0]                                      # two finite values, then -inf by index
    w[2, 777] = np.nan
    w[3, 0] = np.inf
    w3 = w[[0, 1, 2]]
    got = _topk(w3, 10)
    _check_against_numpy(w3, 10, got, "-inf and NaN")
    assert got.classes[1].tolist() == [7, 8, 0, 1, 2, 3, 4, 5, 6, 9] and np.isneginf(got.logprob[1, 2:]).all()
    assert got.classes[2].tolist() == [-1] * 10 and np.isnan(got.logit[2]).all() and np.isnan(got.logprob[2]).all()
    assert _topk(w[3:], 3).classes[0, 0] == 0                      # +inf leads (its logprob is inf - inf: NaN, as the loss is)


def test_agrees_with_eval_metrics_bitwise():
    gen = torch.Generator(device=DEV).manual_seed(5)
    for n, c, k in [(256, 1000, 5), (256, 1000, 32), (64, 10, 10), (33, 4099, 7), (17, 1001, 1)]:
        x = torch.randn((n, c), device=DEV, generator=gen) * 2.0
        x = (x * 32).round() / 32                                  # ties
        t = torch.randint(0, c, (n,), device=DEV, generator=gen)
        best = x.argsort(dim=1, descending=True, stable=True)
        t[::2] = best[torch.arange(n, device=DEV), torch.arange(n, device=DEV) % min(k + 2, c)][::2]     # ranks around k
        dm = DeviceMetrics(DEV, 1)
        loss, rank = dm.update(x, t, 0, per_image=True)
        got = _topk(x, k)
        loss, rank, t = loss.cpu().numpy(), rank.cpu().numpy(), t.cpu().numpy()
        inside = 0
        for i in range(n):
            assert (rank[i] < k) == (t[i] in got.classes[i].tolist()), (n, c, k, i)
            if rank[i] < k:
                inside += 1
                assert got.classes[i, rank[i]] == t[i]
                assert np.float64(-got.logprob[i, rank[i]]).tobytes() == np.float64(loss[i]).tobytes(), (n, c, k, i)
        assert 0 < inside
        print(f"n {n} classes {c} k {k}: {inside} targets inside the top k, all bitwise")


# ---- ttnet_class_counts ---------------------------------------------------------------------------------------------------

def _np_counts(v, t, c):
    counts = np.zeros((c, 4), np.int64)
    conf = np.zeros((c, c), np.int64)
    for i in range(len(t)):
        if not (0 <= t[i] < c):
            continue
        counts[t[i], 0] += 1
        if np.isnan(v[i]).any():
            continue
        rank = int((v[i] > v[i][t[i]]).sum() + (v[i][:t[i]] == v[i][t[i]]).sum())
        counts[t[i], 1] += rank == 0
        counts[t[i], 2] += rank < 5
        top1 = int(_np_topk(v[i], 1)[0][0])
        counts[top1, 3] += 1
        conf[t[i], top1] += 1
    return counts, conf


def test_class_counts_against_numpy():
    rng = np.random.default_rng(7)
    n, c = 300, 40
    v = (rng.standard_normal((n, c)) * 2).round(1).astype(np.float32)
    t = rng.integers(0, c, n).astype(np.int64)
    best = np.argsort(-v, axis=1, kind="stable")
    t[::3] = best[np.arange(n), np.arange(n) % 7][::3]
    t[[5, 50]] = [-1, c]                                          # bad targets
    v[9, 3] = np.nan                                              # a NaN row
    want, want_conf = _np_counts(v, t, c)
    ok = (t >= 0) & (t < c)
    assert np.array_equal(want[:, 0], np.bincount(t[ok], minlength=c))
    nan = np.isnan(v).any(axis=1)
    ref_conf = np.zeros((c, c), np.int64)
    np.add.at(ref_conf, (t[ok & ~nan], best[ok & ~nan, 0]), 1)
    assert np.array_equal(want_conf, ref_conf) and np.array_equal(want[:, 3], ref_conf.sum(0))

    def run(confusion, k, pieces):
        dm = DeviceMetrics(DEV, 1, confusion=confusion)
        for a, b in pieces:
            x, tt = _dev(v[a:b]), _dev(t[a:b])
            dm.update(x, tt, 0, topk=topk_rows(x, k) if k else None, per_class=True)
        return dm, dm.class_counts()

    dm, (counts, conf) = run(True, 5, [(0, n)])
    assert counts.dtype == np.int64 and np.array_equal(counts, want) and np.array_equal(conf, want_conf)
    _, ints = _acc(dm)
    assert counts[:, :3].sum(0).tolist() == ints[0][:3].tolist() and ints[0][3] == 2       # the accumulator's images, hits1, hits5
    assert counts[:, 3].sum() == n - 2 - 1
    # order does not matter; nor does k; twice the same batches, the same bytes
    for pieces, k, confusion in [([(0, 100), (100, 101), (101, n)], 1, True), ([(0, n)], 0, False), ([(0, n)], 5, True)]:
        _, (c2, m2) = run(confusion, k, pieces)
        assert c2.tobytes() == counts.tobytes()
        assert (m2 is None) if not confusion else (m2.tobytes() == conf.tobytes())
    # the counters ADD
    dm.update(_dev(v), _dev(t), 0, per_class=True)
    c3, m3 = dm.class_counts()
    assert np.array_equal(c3, 2 * want) and np.array_equal(m3, 2 * want_conf)


# ---- refusals and graphs --------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused():
    lib = _lib.load()
    x = torch.zeros((4, 8), device=DEV)
    out = torch.full((4 * 33 + 1, 2), -7, dtype=torch.int64, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())      # noqa: E731
    E = -1                                       # TTNET_E_INVALID
    for n, c, k in [(4, 8, 0), (4, 8, 33), (4, 8, 9), (4, 2, 3), (0, 8, 1), (65536, 8, 1), (4, 1, 1), (4, 65537, 1), (4, 8, -1)]:
        assert lib.ttnet_topk_rows(p(x), n, c, k, p(out), None) == E, (n, c, k)
    assert lib.ttnet_topk_rows(None, 4, 8, 1, p(out), None) == E
    assert lib.ttnet_topk_rows(p(x), 4, 8, 1, None, None) == E
    assert lib.ttnet_topk_rows(p(x), 4, 8, 1, C.c_void_p(out.data_ptr() + 4), None) == E      # misaligned output
    assert lib.ttnet_topk_rows(C.c_void_p(x.data_ptr() + 2), 3, 8, 1, p(out), None) == E
    assert "topk_rows" in lib.ttnet_last_error().decode()
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    rec = torch.zeros((4, 2), dtype=torch.int64, device=DEV)
    counts = torch.zeros((8, 4), dtype=torch.int64, device=DEV)
    good = [p(t), p(rec), p(out), 4, 1, 8, p(counts), None, None]
    for i, bad in [(0, None), (1, None), (2, None), (6, None), (3, 0), (4, 0), (4, 33), (4, 9), (5, 1),
                   (6, C.c_void_p(counts.data_ptr() + 4))]:
        args = list(good)
        args[i] = bad
        assert lib.ttnet_class_counts(*args) == E, (i, bad)
    torch.cuda.synchronize(DEV)
    assert (out == -7).all() and (counts == 0).all()              # nothing was launched
    with pytest.raises(ValueError):
        topk_rows(x, 9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        topk_rows(x.cpu(), 1)
    # and the good call
    _lib.check(lib.ttnet_topk_rows(p(x), 4, 8, 8, p(out), None))
    torch.cuda.synchronize(DEV)
    got = Predictions.from_records(out[:32].view(4, 8, 2).cpu().numpy())
    assert got.classes.tolist() == [list(range(8))] * 4 and (out[32:] == -7).all()


def test_captured_in_a_graph_and_replayed_with_new_logits():
    gen = torch.Generator(device=DEV).manual_seed(3)
    n, c, k = 256, 1000, 5
    x = torch.randn((n, c), device=DEV, generator=gen)
    t = torch.randint(0, c, (n,), device=DEV, generator=gen)
    rec = torch.zeros((n, k, 2), dtype=torch.int64, device=DEV)
    per = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    acc = torch.zeros(8, dtype=torch.int64, device=DEV)
    counts = torch.zeros((c, 4), dtype=torch.int64, device=DEV)
    lib = _lib.load()
    p = lambda a: C.c_void_p(a.data_ptr())      # noqa: E731
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
            _lib.check(lib.ttnet_eval_metrics(p(x), p(t), n, c, p(acc), p(per), s))
            _lib.check(lib.ttnet_topk_rows(p(x), n, c, k, p(rec), s))
            _lib.check(lib.ttnet_class_counts(p(t), p(per), p(rec), n, k, c, p(counts), None, s))
    torch.cuda.synchronize(DEV)
    assert (rec == 0).all() and (counts == 0).all()                # capturing ran nothing
    total = np.zeros((c, 4), np.int64)
    for seed in (11, 12):
        x.copy_(torch.randn((n, c), device=DEV, generator=gen.manual_seed(seed)))
        graph.replay()
        torch.cuda.synchronize(DEV)
        v = x.cpu().numpy()
        got = Predictions.from_records(rec.cpu().numpy())
        _check_against_numpy(v, k, got, f"replay {seed}")
        assert got.classes.tobytes() == _topk(x, k).classes.tobytes()
        total += _np_counts(v, t.cpu().numpy(), c)[0]
        assert np.array_equal(counts.cpu().numpy(), total)


# ---- evaluate ---------------------------------------------------------------------------------------------------------------

def _same(a: Predictions, b: Predictions):
    return a.classes.tobytes() == b.classes.tobytes() and a.logit.tobytes() == b.logit.tobytes() and \
        a.logprob.tobytes() == b.logprob.tobytes()


def test_evaluate_topk_per_class_over_the_batch_types_and_lanes():
    model = _model("small", 64)
    files = _fixture_files()
    data = [open(f, "rb").read() for f in files]
    pil = [_pillow(f) for f in files]
    with torch.no_grad():
        crops = preprocess.resize_center_crop_u8_ragged(preprocess.pack_u8(pil).to(DEV))
    n = len(files)
    cuts = [(0, 16), (16, 32), (32, n)]
    with torch.no_grad():
        y = torch.cat([model.forward_u8(crops[a:b]).cpu() for a, b in cuts])     # the batches evaluate() will see
    crops = crops.cpu()
    xf = torch.from_numpy(synth.normalize_u8(np.ascontiguousarray(crops.numpy().transpose(0, 3, 1, 2))))
    t = y.argsort(dim=1, descending=True)[torch.arange(n), torch.arange(n) % 8].contiguous()
    kinds = {
        "jpeg": [J.collate_jpeg([(data[i], int(t[i])) for i in range(a, b)]) for a, b in cuts],
        "u8 ragged": [preprocess.collate_u8([(pil[i], int(t[i])) for i in range(a, b)]) for a, b in cuts],
        "u8 crops": [(crops[a:b], t[a:b]) for a, b in cuts],
    }
    want = Predictions(*(np.stack(c) for c in zip(*[_np_topk(r, 5) for r in y.numpy()])))
    # a run without the options, per lane count (the lanes' float64 loss sums are added in lane order)
    plains = {i: evaluate(model, kinds["jpeg"], DEV, inflight=i, metrics="device") for i in (1, 2)}
    first = None
    for name, batches in kinds.items():
        for inflight in (1, 2):
            r = evaluate(model, batches, DEV, inflight=inflight, metrics="device", topk=5, per_class=True, confusion=True)
            print(name, inflight, r, r.parts)
            plain = plains[inflight]
            assert (r.loss, r.top1, r.top5, r.images) == (plain.loss, plain.top1, plain.top5, plain.images)     # the headline numbers
            assert np.float64(r.parts.loss_sum).tobytes() == np.float64(plain.parts.loss_sum).tobytes()
            assert len(r.predictions) == n
            first = first or r
            assert _same(r.predictions, first.predictions), (name, inflight)
            assert np.array_equal(r.per_class, first.per_class) and np.array_equal(r.confusion, first.confusion)
    pred = first.predictions
    assert np.array_equal(pred.classes, want.classes) and np.array_equal(pred.logit, want.logit)      # dataset order
    assert np.abs(pred.logprob - want.logprob).max() <= 1e-9
    tn = t.numpy()
    counts = first.per_class
    assert np.array_equal(counts[:, 0], np.bincount(tn, minlength=1000))
    assert counts[:, :3].sum(0).tolist() == [n, first.parts.hits1, first.parts.hits5] and counts[:, 3].sum() == n
    assert np.array_equal(counts[:, 3], np.bincount(pred.classes[:, 0], minlength=1000))
    conf = np.zeros((1000, 1000), np.int64)
    np.add.at(conf, (tn, pred.classes[:, 0]), 1)
    assert np.array_equal(first.confusion, conf)
    # float batches of the same images (ToTensor + Normalize on the host): the float stem rounds differently from the
    # uint8 one, so first say how far the logits are apart
    rf = evaluate(model, [(xf[a:b], t[a:b]) for a, b in cuts], DEV, inflight=2, metrics="device", topk=5, per_class=True)
    print("float batches: max |logit - uint8 path's|", float(np.abs(rf.predictions.logit - pred.logit).max()),
          "classes equal:", np.array_equal(rf.predictions.classes, pred.classes))
    assert _same(rf.predictions, pred)
    # the torch metrics with top-k; unlabelled batches
    rt = evaluate(model, kinds["u8 crops"], DEV, inflight=2, metrics="torch", topk=5)
    assert _same(rt.predictions, pred)
    free = evaluate(model, [(b[0], None) for b in kinds["jpeg"]], DEV, inflight=2, topk=5)
    assert free.loss is None and free.images == n and _same(free.predictions, pred)
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluate(model, kinds["u8 crops"], DEV, metrics="torch", per_class=True)


# ---- the commands ---------------------------------------------------------------------------------------------------------

def test_commands_single_process_and_two_ranks(tmp_path):
    files = _fixture_files()
    val = tmp_path / "data" / "val"
    for c in ("n01", "n02"):
        (val / c).mkdir(parents=True)
    for i, f in enumerate(files):
        (val / ("n01" if i % 3 else "n02") / os.path.basename(f)).write_bytes(open(f, "rb").read())
    _, st = spec_and_state("small")
    ckpt = tmp_path / "synthetic.pth"
    torch.save({"model_state_dict": {"module." + k: torch.from_numpy(v.copy()) for k, v in st.items()}}, str(ckpt))
    names = tmp_path / "names.txt"
    names.write_text("".join(f"class {i}\n" for i in range(1000)))

    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p),
               TTNET_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    common = ["--ckpt", str(ckpt), "--eval_batch_size", "16", "--num_workers", "2", "--log_interval", "0"]

    def command(module, data_dir, extra):
        cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", module, "--data_dir", str(data_dir)] + common + extra
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, (module, extra, r.returncode, r.stderr[-3000:])      # (stops at the first failure)
        return r

    outs = {}
    for tag, extra in (("one", ["--gpu", "0"]), ("two", ["--gpus", "2"])):
        # the run without the flags, at the same number of ranks (the gloo rehearsal writes a line of its own to
        # rank 0's standard output; it is the same line with and without the flags)
        plain = command("scale_imagenet_amd.main", tmp_path / "data", extra)
        if outs:
            assert _acc_line(plain.stdout) == first_line
        first_line = _acc_line(plain.stdout)
        f = {k: str(tmp_path / f"{tag}_{k}") for k in ("pred.csv", "class.csv", "conf.npy", "predict.csv", "named.csv")}
        r = command("scale_imagenet_amd.main", tmp_path / "data",
                    extra + ["--topk", "5", "--predictions", f["pred.csv"], "--per_class", f["class.csv"], "--confusion", f["conf.npy"]])
        assert _acc_line(r.stdout) == _acc_line(plain.stdout) and r.stdout == plain.stdout
        command("scale_imagenet_amd.predict", val, extra + ["--topk", "5", "--out", f["predict.csv"]])
        outs[tag] = f
    for k in ("pred.csv", "class.csv", "conf.npy", "predict.csv"):
        assert open(outs["one"][k], "rb").read() == open(outs["two"][k], "rb").read(), k
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]
    folder = J.FileBytesFolder(str(val))
    paths, targets, classes, logprob = report.read_predictions_csv(outs["one"]["pred.csv"])
    assert paths == [p for p, _ in folder.samples] and targets == [str(t) for t in folder.targets]
    assert logprob.shape == (len(files), 5) and (np.diff(logprob, axis=1) <= 0).all()
    # predict: the same files, unlabelled, in sorted path order (which is the folder's here): the same class columns
    p2, t2, c2, l2 = report.read_predictions_csv(outs["one"]["predict.csv"])
    assert p2 == paths and t2 == [""] * len(files) and c2 == classes and l2.tobytes() == logprob.tobytes()
    conf = np.load(outs["one"]["conf.npy"])
    assert conf.dtype == np.int64 and conf.shape == (1000, 1000) and conf.sum() == len(files)
    want = np.zeros_like(conf)
    np.add.at(want, (np.array(folder.targets), np.array([int(c[0]) for c in classes])), 1)
    assert np.array_equal(conf, want)
    rows = open(outs["one"]["class.csv"]).read().splitlines()
    assert rows[0] == "class,images,hits1,hits5,predicted,acc1,acc5" and len(rows) == 1001
    counts = np.array([[int(x) for x in r.split(",")[1:5]] for r in rows[1:]])
    assert counts[:, 0].tolist()[:3] == [folder.targets.count(0), folder.targets.count(1), 0]
    top1, top5 = _acc_line(plain.stdout)
    assert (100.0 * counts[:, 1].sum() / len(files), 100.0 * counts[:, 2].sum() / len(files)) == (top1, top5)
    # names, written to standard output
    r = command("scale_imagenet_amd.predict", val, ["--gpu", "0", "--topk", "2", "--classes", str(names)])
    lines = r.stdout.splitlines()
    assert lines[0] == "path,target,class_1,logprob_1,class_2,logprob_2" and len(lines) == 1 + len(files)
    assert lines[1].split(",")[2] == f"class {classes[0][0]}"
