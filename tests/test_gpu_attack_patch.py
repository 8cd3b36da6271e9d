"""GPU: ttnet_attack_patch_u8 and ttnet_patch_paste_u8 (csrc/attack.hip) against the numpy float64 twin
(``attack.attack_patch_cpu``), against the device's own box certificate, against its forward and against the certified sweep.

Synthetic weights, synthetic images 0, 1 and 7, the classes the float64 oracle gives them, the norms ``cifar`` and ``std16``.
Standard of comparison: fills byte-identical, integers identical, ``m_pred`` within ``1e-9 * sum|A|``; a position is excused only
where the twin's best and second-best distinct predictions of some round lie within that distance, at most 1 % of the positions
compared."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attack_patch_util as U
from _attack_util import NORMS
from _util import args_for, spec_and_state
from scale_imagenet_amd import _lib
from scale_imagenet_amd import attack as AT
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar, synth, ttnet
from test_gpu_attack import images, new_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [((2, 3), 3, 8, 2), ((4, 4), 4, 1, 2), ((8, 8), 8, 255, 2), ((4, 4), 4, 255, 2), ((1, 1), 4, 255, 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def models(dev):
    return {norm: new_model(dev, norm) for norm in NORMS}


def x3(dev):
    return torch.tensor(U.images3()).to(dev)


def c3(dev, norm):
    return torch.from_numpy(U.classes3(norm)).to(dev)


def compare(res, tw):
    """A device result against the twin's.  Returns (excused positions, largest |m_pred - twin|)."""
    n = len(res)
    got, want, near = res.map.reshape(n, -1), tw.map.reshape(n, -1), tw.near
    ok = ~near
    assert near.mean() <= 0.01
    assert (res.fills_numpy() == tw.fills_numpy()).all(axis=2)[ok].all()
    for k in ("round", "unknown", "worst"):
        assert np.array_equal(got[k][ok], want[k][ok]), k
    err = np.abs(got["m_pred"][ok] - want["m_pred"][ok]).max()
    assert err <= U.tolerance(), err
    return int(near.sum()), float(err)


def test_one_pixel_patches_take_the_cut_and_equal_the_twin(models, dev):
    """Images 0, 1, 7 at 1 x 1 / 255 / stride 1 are 3,072 tasks: two launches, read from the library; one round = the corners."""
    py, px, launches, first, last, cap = _lib.launch_partition("patch.attack", 3, 1, 1, 1)
    assert (py, px, launches) == (32, 32, 2) and first == cap and last == 3 * 1024 - cap
    res = models["cifar"].attack_patch_u8(x3(dev), c3(dev, "cifar"), (1, 1), 1, 255, rounds=1)
    excused, err = compare(res, U.twin("cifar", (1, 1), 1, 255, 1))
    print(f"1x1: {excused} positions excused, max |m_pred - twin| = {err:.3g}; falsified {res.rows['falsified'].tolist()}")
    flat = res.map.reshape(3, -1)
    assert (np.abs((flat["m_pred"] < 0).sum(axis=1) - np.array([537, 97, 0])) <= 10).all()
    assert res.rows["status"].tolist() == [AT.FALSIFIED, AT.FALSIFIED, AT.OPEN]


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("patch,stride,amp,rounds", SETTINGS)
def test_search_equals_the_twin_and_its_witnesses_hold(models, dev, norm, patch, stride, amp, rounds):
    model, x, cls = models[norm], x3(dev), c3(dev, norm)
    res = model.attack_patch_u8(x, cls, patch, stride, amp, rounds=rounds)
    excused, err = compare(res, U.twin(norm, patch, stride, amp, rounds))
    print(f"{norm} {patch} stride {stride} amp {amp}: {excused} excused, max |m_pred - twin| = {err:.3g}, falsified {res.rows['falsified'].tolist()}")
    # soundness: every falsified position again, pasted by numpy, through a fresh forward
    n, py, px = res.map.shape
    flat = res.map.reshape(-1)
    tasks = np.flatnonzero(flat["status"] == AT.FALSIFIED)
    assert not (flat["status"] == AT.PREDICTED).any()                    # confirm="all": every prediction met its forward
    if tasks.size:
        wit = AT.paste_cpu(U.images3(), patch, stride, res.fills_numpy(), tasks)
        with torch.no_grad():
            logits = torch.cat([model.forward_u8(torch.from_numpy(wit[a:a + 256]).to(dev)) for a in range(0, len(wit), 256)]).cpu().numpy()
        c = U.classes3(norm)[tasks // (py * px)]
        own = logits[np.arange(len(c)), c]
        logits[np.arange(len(c)), c] = -np.inf
        margin = own - logits.max(axis=1)
        assert (margin < 0).all() and np.array_equal(margin, flat["margin"][tasks])
        diff = np.abs(wit.astype(np.int64) - U.images3()[tasks // (py * px)])
        assert diff.max() <= amp
        for k, t in enumerate(tasks):
            y0, x0 = CF.patch_origins(patch, stride)[t % (py * px)]
            d = diff[k].copy()
            d[y0:y0 + patch[0], x0:x0 + patch[1]] = 0
            assert not d.any()
        assert np.array_equal(res.witness(int(tasks[0] // (py * px)), int(tasks[0] % (py * px))), wit[0])


def test_m_pred_is_the_devices_own_box_certificate(models, dev):
    """256 sampled tasks: ``m_pred`` equals ``lb_interval`` of ``ttnet_certify_box_u8`` on the pasted witness."""
    model, x, cls = models["cifar"], x3(dev), c3(dev, "cifar")
    for patch, stride, amp, rounds in (((1, 1), 1, 255, 2), ((4, 4), 2, 255, 2)):
        rec, fills = AT.patch_search_u8(model, x, cls, patch, stride, amp, rounds)
        P = rec.shape[1]
        tasks = torch.from_numpy(np.random.default_rng(3).choice(3 * P, 256, replace=False)).to(dev)
        wit = AT.paste_u8(model, x, patch, stride, fills, tasks)
        rows = CF.certify_box_u8(model, wit, wit, cls[tasks // P], 0, 0.0).numpy()
        got = rec.cpu().numpy().view(AT.PATCH_RECORD).reshape(-1)[tasks.cpu().numpy()]
        assert (got["round"] > 0).sum() > 32
        assert np.abs(got["m_pred"] - rows["lb_interval"]).max() <= U.tolerance() and np.array_equal(got["worst"], rows["worst"])


@pytest.mark.parametrize("patch,stride,amp", [((2, 3), 3, 8), ((1, 1), 1, 255)])
def test_no_falsified_position_is_certified(models, dev, patch, stride, amp):
    model, x, cls = models["cifar"], x3(dev), c3(dev, "cifar")
    mm = U.LOGIT_TOL
    res = model.attack_patch_u8(x, cls, patch, stride, amp, rounds=2, min_margin=mm)
    cert = model.certify_patch_u8(x, cls, patch, stride, amp, min_margin=mm)
    rows, maps = cert.numpy()
    assert (res.map["status"] == AT.FALSIFIED).any() and (maps["stage"] > 0).any()
    assert not ((res.map["status"] == AT.FALSIFIED) & (maps["stage"] > 0)).any()
    assert (res.map["margin"][res.map["status"] == AT.FALSIFIED] < -mm).all()
    b = AT.patch_robust_bounds(CF.summarise_patch(patch, stride, amp, rows, maps), AT.summarise_patch(res, 2))
    assert b["positions_falsified"] == int(res.rows["falsified"].sum()) and b["certified"] + b["falsified"] + b["open"] == 3


def test_runs_lanes_and_batch_composition_give_the_same_bytes(models, dev):
    model = models["std16"]
    n = 257
    x = images(dev, n)
    with torch.no_grad():
        cls = model.forward_u8(x[:256]).argmax(dim=1)
        cls = torch.cat([cls, model.forward_u8(x[256:]).argmax(dim=1)])
    args = ((2, 3), 3, 255)
    full = model.attack_patch_u8(x, cls, *args)
    assert (full.rows["status"] == AT.FALSIFIED).any() and (full.rows["status"] == AT.OPEN).any()
    again, lane1 = model.attack_patch_u8(x, cls, *args), model.attack_patch_u8(x, cls, *args, lane=1)
    parts = [model.attack_patch_u8(x[a:b], cls[a:b], *args) for a, b in ((0, 128), (128, 256), (256, 257))]
    for other in (again, lane1):
        assert other.map.tobytes() == full.map.tobytes() and torch.equal(other.fills, full.fills) and other.rows.tobytes() == full.rows.tobytes()
    assert np.concatenate([p.map for p in parts]).tobytes() == full.map.tobytes()
    assert torch.equal(torch.cat([p.fills for p in parts]), full.fills)
    best = model.attack_patch_u8(x, cls, *args, confirm="best")
    for k in AT.PATCH_RECORD.names:
        assert np.array_equal(best.map[k], full.map[k])
    judged = ~np.isnan(best.map["margin"])
    assert judged.reshape(n, -1).sum(axis=1).max() == 1 and np.array_equal(best.map["margin"][judged], full.map["margin"][judged])
    assert ((best.map["status"] == AT.FALSIFIED) <= (full.map["status"] == AT.FALSIFIED)).all()
    assert np.array_equal(best.rows["status"], full.rows["status"])
    none = model.attack_patch_u8(x[:3], cls[:3], *args, confirm="none")
    assert np.isnan(none.map["margin"]).all() and (none.map["status"] != AT.FALSIFIED).all()


def test_paste_equals_numpy(models, dev):
    model, x = models["cifar"], x3(dev)
    rng = np.random.default_rng(11)
    for patch, stride in (((1, 1), 1), ((2, 5), 3), ((8, 8), 8), ((3, 8), 7)):
        P = len(CF.patch_origins(patch, stride))
        fills = rng.integers(0, 256, (3, P, AT.FILL_BYTES)).astype(np.uint8)
        tasks = np.concatenate([rng.integers(0, 3 * P, 40), [0, 3 * P - 1, 3 * P, -1, 1 << 40]]).astype(np.int64)
        got = AT.paste_u8(model, x, patch, stride, torch.from_numpy(fills).to(dev), torch.from_numpy(tasks).to(dev)).cpu().numpy()
        assert np.array_equal(got, AT.paste_cpu(U.images3(), patch, stride, fills, tasks))
        assert not got[-3:].any()


def test_c_abi_errors_and_classes_outside_the_range(models, dev):
    model = models["cifar"]
    n = 3
    x = x3(dev)
    cls = torch.tensor([int(U.classes3("cifar")[0]), 10, -3], dtype=torch.int32, device=dev)
    plan = model._plan_for(dev, n)
    lib = plan.lib
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P_ = 64
    rec = torch.zeros((n, P_, 2), dtype=torch.float64, device=dev)
    fills = torch.zeros((n, P_, AT.FILL_BYTES), dtype=torch.uint8, device=dev)
    tasks = torch.arange(4, dtype=torch.int64, device=dev)
    out = torch.zeros((4, 32, 32, 3), dtype=torch.uint8, device=dev)
    P = lambda v: C.c_void_p(v)  # noqa: E731

    def attack(h=plan.handle, lane=0, xp=x.data_ptr(), n=n, c=cls.data_ptr(), ph=4, pw=4, st=4, amp=255, r=2, mm=0.0, m=rec.data_ptr(),
               f=fills.data_ptr()):
        return lib.ttnet_attack_patch_u8(h, lane, P(xp), n, P(c), ph, pw, st, amp, r, mm, P(m), P(f), s)

    def paste(h=plan.handle, xp=x.data_ptr(), n=n, ph=4, pw=4, st=4, f=fills.data_ptr(), t=tasks.data_ptr(), m=4, o=out.data_ptr()):
        return lib.ttnet_patch_paste_u8(h, P(xp), n, ph, pw, st, P(f), P(t), m, P(o), s)
    assert attack() == 0                                                 # a class outside 0..9 is no error
    torch.cuda.synchronize()
    got = rec.cpu().numpy().view(AT.PATCH_RECORD).reshape(n, P_)
    assert np.isfinite(got["m_pred"][0]).all() and np.isneginf(got["m_pred"][1:]).all() and (got["worst"][1:] == -1).all()
    assert not got["round"][1:].any() and not got["unknown"][1:].any()
    clean = AT.paste_cpu(U.images3(), (4, 4), 4, fills.cpu().numpy(), np.arange(P_, 3 * P_))
    assert np.array_equal(clean, np.repeat(U.images3()[1:], P_, axis=0))  # their fills are the clean bytes
    assert paste() == 0
    torch.cuda.synchronize()
    keep = [t.clone() for t in (rec, fills, out)]
    for kw in (dict(lane=2), dict(lane=-1), dict(n=0), dict(n=258), dict(ph=0), dict(ph=9), dict(pw=0), dict(pw=9), dict(st=0), dict(st=33),
               dict(amp=0), dict(amp=256), dict(r=0), dict(r=5), dict(mm=float("nan")), dict(xp=None), dict(c=None), dict(m=None), dict(f=None),
               dict(xp=x.data_ptr() + 1), dict(c=cls.data_ptr() + 2), dict(m=rec.data_ptr() + 4), dict(f=fills.data_ptr() + 2)):
        assert attack(**kw) == -1, kw
        assert lib.ttnet_last_error()
    for kw in (dict(n=0), dict(n=258), dict(ph=0), dict(pw=9), dict(st=0), dict(st=33), dict(m=0), dict(m=-1), dict(xp=None), dict(f=None),
               dict(t=None), dict(o=None), dict(xp=x.data_ptr() + 1), dict(f=fills.data_ptr() + 2), dict(t=tasks.data_ptr() + 4),
               dict(o=out.data_ptr() + 3)):
        assert paste(**kw) == -1, kw
        assert lib.ttnet_last_error()
    small = ttnet._Plan(spec_and_state("small")[0], args_for("small"), 0, 4)
    try:
        assert attack(h=small.handle) == -4 and "affine head" in lib.ttnet_last_error().decode()
        assert paste(h=small.handle) == -4
    finally:
        small.close()
    raw = ttnet._Plan(spec_and_state("valexnet")[0], args_for("valexnet"), 0, 4)
    try:
        assert attack(h=raw.handle) == -2 and "ttnet_attack_patch_u8 before ttnet_plan_finalize" in lib.ttnet_last_error().decode()
        assert paste(h=raw.handle) == -2 and "ttnet_patch_paste_u8 before ttnet_plan_finalize" in lib.ttnet_last_error().decode()
    finally:
        raw.close()
    torch.cuda.synchronize()
    for t, k in zip((rec, fills, out), keep):                             # nothing was launched in any error case
        assert torch.equal(t, k)
    with pytest.raises(ValueError):
        model.attack_patch_u8(x, cls, rounds=5)
    with pytest.raises(ValueError):
        model.attack_patch_u8(x, cls, confirm="some")
    with pytest.raises(RuntimeError):
        model.attack_patch_u8(x.float(), cls)


def test_command_prints_patch_robust_lines(dev, tmp_path):
    model = new_model(dev, max_batch=128)
    n = 150
    u8 = synth.synth_images_u8(n, hw=(32, 32))
    labels = (np.arange(n) % 10).astype(np.int64)
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([labels[:, None].astype(np.uint8), u8.reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
    x = np.ascontiguousarray(u8.transpose(0, 2, 3, 1))
    batches = list(cifar.device_batches(x, labels, 128, dev))
    certs = CF.certify_batches(model, batches, [1.0], min_margin=1e-5)
    pcerts = CF.certify_patch_batches(model, batches, [(4, 4), (1, 2)], 4, 255, min_margin=1e-5)
    found = AT.attack_patch_batches(model, batches, [(4, 4), (1, 2)], 4, 255, 2, 1e-5)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    wit_file = tmp_path / "w.npz"
    base = ["timeout", "-k", "10", "300", sys.executable, "-m", "scale_imagenet_amd.cifar", "--data_dir", str(tmp_path), "--synthetic-ckpt",
            "--eval_batch_size", "128", "--certify", "1", "--certify_min_margin", "1e-5", "--certify_patch", "4x4,1x2", "--patch_stride", "4"]
    r = subprocess.run(base + ["--attack_patch", "--patch_witnesses", str(wit_file)], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == 6 and re.fullmatch(r"Acc\.\. (\S+) (\S+)", out[0])
    assert out[1] == CF.verified_line(certs[0]) and [out[2], out[4]] == [CF.patch_line(s) for s in pcerts]
    assert [out[3], out[5]] == [AT.patch_robust_line(c, a) for c, a in zip(pcerts, found)]
    assert re.fullmatch(r"PatchRobust\.\. size=4x4 amp=255 stride=4 certified \d+/150 <= robust <= \d+/150 \(falsified \d+: wrong at x0 \d+, by search "
                        r"\d+; open \d+; positions certified \d+, falsified \d+, open \d+\)", out[3])
    with np.load(wit_file) as z:
        for a, key in zip(found, ("4x4", "1x2")):
            tasks = np.flatnonzero(a["map"].reshape(-1)["status"] == AT.FALSIFIED)
            assert tasks.size and np.array_equal(z[f"tasks_{key}"], tasks)
            h, w, stride, amp, py, px = z[f"geometry_{key}"]
            fills = np.zeros((n, py * px, AT.FILL_BYTES), np.uint8)
            fills.reshape(-1, AT.FILL_BYTES)[tasks, :3 * h * w] = z[f"fills_{key}"]
            wit = AT.paste_cpu(x, (h, w), stride, fills, tasks[:256])               # the images reproduce their margins
            with torch.no_grad():
                logits = model.forward_u8(torch.from_numpy(wit[:128]).to(dev)).cpu().numpy()
            c = labels[tasks[:128] // (py * px)]
            own = logits[np.arange(len(c)), c]
            logits[np.arange(len(c)), c] = -np.inf
            assert np.array_equal(own - logits.max(axis=1), z[f"margin_{key}"][:128])
    assert sorted(os.listdir(tmp_path)) == ["cifar-10-batches-bin", "w.npz"]
    r2 = subprocess.run(base, capture_output=True, text=True, env=env, cwd=str(tmp_path))    # without the flag: the lines as they were
    assert r2.returncode == 0 and r2.stdout.splitlines() == [out[0], out[1], out[2], out[4]]
