"""GPU: ttnet_certify_u8 (csrc/certify.hip) against its numpy float64 twin (scale_imagenet_amd/certify.py: certify_cpu),
against the device's own forward, and through the C ABI and the command.

Synthetic weights, 64 synthetic images, the classes the float64 oracle gives them.  The stem planes are compared where the
twin's bound is further than 8 x slack from zero (everywhere, for these inputs: checked); the later stages are integer work
and float64 sums, compared with the twin fed the DEVICE's stem planes: bit-identical planes, bounds to 1e-9 * sum|A|."""
import csv
import ctypes as C
import os
import re
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

from _certify_util import normalise, oracle_pre
from _util import ROOT, args_for, scaled_tol, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import cifar, synth, ttnet
from scale_imagenet_amd import certify as CF

pytestmark = pytest.mark.gpu

N = 64
EPS_ALL = (0.0, 0.01, 0.03, 0.1, 1.0, 2.0)
HALF = ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def new_model(dev, state=None, max_batch=257):
    st = state if state is not None else spec_and_state("valexnet")[1]
    m = ttnet.TT_FHE_XSMALL_vAlexnet(args_for("valexnet"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    return m.to(dev).eval().reserve(max_batch)


@pytest.fixture(scope="module")
def model(dev):
    m = new_model(dev).set_lanes(2)
    with torch.no_grad():
        m.forward_u8(images(dev)[:1])                       # (creates the plan: get_table needs one)
    return m


@lru_cache(maxsize=None)
def images_np(n=N):
    a = np.ascontiguousarray(synth.synth_images_u8(n, hw=(32, 32)).transpose(0, 2, 3, 1))
    a.setflags(write=False)
    return a


def images(dev, n=N):
    return torch.tensor(images_np(n)).to(dev)               # (a copy: the cached array is read-only)


@lru_cache(maxsize=None)
def classes_np(n=N):
    spec, st = spec_and_state("valexnet")
    luts, _ = OB.build_all_luts(st, spec)
    pre = oracle_pre(st, normalise(images_np(n).astype(np.float64)))
    return OB.valexnet_from_stem_bits((pre >= 0).astype(np.uint8), st, spec, luts)[1].argmax(axis=1)


_TABLES = {}


def tables(model):
    if not _TABLES:
        _TABLES.update({b.name: model.get_table(b.name) for b in model.spec.block_tts()})
    return _TABLES


_RUNS = {}


def device_run(model, dev, eps, n=N):
    """(records, planes as uint8 bit arrays) of the device for the first n images; one launch per (eps, n)."""
    if (eps, n) not in _RUNS:
        res = model.certify_u8(images(dev, n), torch.from_numpy(classes_np(n)), eps, return_planes=True)
        p = res.planes_numpy()
        _RUNS[(eps, n)] = (res.numpy().copy(), {k: OB.unpack_rows(v, 10 if k.startswith("stem") else 11) for k, v in p.items()})
    return _RUNS[(eps, n)]


def sum_abs_A():
    return float(np.abs(CF.effective_head(spec_and_state("valexnet")[1])[0]).sum())


def compare_rows(got, want, bounds, tol, min_margin=1e-6):
    """Device records against the twin's (``certify_cpu(.., return_bounds=True)``).  Returns (images whose ``worst`` is another
    class than the twin's, each shown here to be a tie within tol; images whose ``lb`` lies within tol of min_margin, for
    which alone the stage may differ)."""
    assert np.array_equal(got["unknown_stem"], want["unknown_stem"]) and np.array_equal(got["unknown_feat"], want["unknown_feat"])
    for col in ("lb_interval", "lb"):
        fin = np.isfinite(want[col])
        assert np.array_equal(fin, np.isfinite(got[col])) and np.array_equal(got[col][~fin], want[col][~fin])
        assert np.abs(got[col][fin] - want[col][fin]).max(initial=0.0) <= tol, col
    clear = np.abs(want["lb"] - min_margin) > tol                        # a bound within tol of the threshold may fall on either side
    assert np.array_equal(got["stage"][clear], want["stage"][clear])
    # stage 2 ran on the same images
    assert np.array_equal((got["lb"] != got["lb_interval"])[clear], (want["lb"] != want["lb_interval"])[clear])
    diff = np.flatnonzero(got["worst"] != want["worst"])
    for i in diff:                                                       # another class only where the twin's own bounds of the two tie
        g, w = int(got["worst"][i]), int(want["worst"][i])
        assert 0 <= g < 10 and 0 <= w < 10, (i, g, w)
        assert np.isfinite(bounds[i, g]) and abs(bounds[i, g] - bounds[i, w]) <= tol, (i, g, w, bounds[i].tolist())
    return diff, np.flatnonzero(~clear)


# ---- 1. stem planes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", EPS_ALL)
def test_stem_planes_equal_the_twin(model, dev, eps):
    _, st = spec_and_state("valexnet")
    _, planes = device_run(model, dev, eps)
    lo, hi = CF.stem_bounds_cpu(st, images_np(), eps)
    sl = CF.stem_slack(st)[None, :, None, None]
    band_lo, band_hi = np.abs(lo - sl) <= 8 * sl, np.abs(hi + sl) <= 8 * sl
    want_lo, want_hi = CF.stem_planes_cpu(st, images_np(), eps)
    bad = int(((planes["stem_lo"] != want_lo) & ~band_lo).sum() + ((planes["stem_hi"] != want_hi) & ~band_hi).sum())
    in_band = int(band_lo.sum() + band_hi.sum())
    print(f"eps {eps}: {in_band} of {2 * lo.size} bounds within 8 x slack of zero; {bad} plane bits differ outside; "
          f"{int((want_lo != want_hi).sum())} unknown stem bits")
    assert bad == 0
    assert in_band < 1e-3 * 2 * lo.size
    assert in_band == 0                                                  # (the twin's own count for these inputs: so the planes are equal)
    assert np.array_equal(planes["stem_lo"], want_lo) and np.array_equal(planes["stem_hi"], want_hi)
    assert (planes["stem_lo"] <= planes["stem_hi"]).all()


# ---- 2. feature planes and records, given the device's stem planes -----------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.01, 0.03, 0.1, 1.0])
def test_block_margin_and_enumeration_equal_the_twin(model, dev, eps):
    _, st = spec_and_state("valexnet")
    rows, planes = device_run(model, dev, eps)
    want, wp, bounds = CF.certify_cpu(st, tables(model), images_np(), classes_np(), eps, stem_planes=(planes["stem_lo"], planes["stem_hi"]),
                                      return_planes=True, return_bounds=True)
    assert np.array_equal(planes["feat_lo"], wp["feat_lo"]) and np.array_equal(planes["feat_hi"], wp["feat_hi"])
    tol = 1e-9 * sum_abs_A()
    ties, masked = compare_rows(rows, want, bounds, tol)
    print(f"eps {eps}: stages {np.bincount(rows['stage'], minlength=3).tolist()}, largest |lb - twin| "
          f"{np.abs(rows['lb'] - want['lb']).max():.2e} (tol {tol:.2e}), {ties.size} images with another worst class (ties), "
          f"{masked.size} with lb within tol of min_margin")
    assert ties.size == 0 and masked.size == 0                          # (for these inputs: nominal margins start at 2.3e-4, tol is 8e-6)
    again = model.certify_u8(images(dev), torch.from_numpy(classes_np()), eps, return_planes=True)
    assert again.numpy().tobytes() == rows.tobytes()
    assert all(np.array_equal(OB.unpack_rows(v, 10 if k.startswith("stem") else 11), planes[k]) for k, v in again.planes_numpy().items())
    if eps == 0.03:                                                      # the prototype's table: stage 2 is exercised
        assert (rows["stage"] == 1).sum() == 32 and (rows["stage"] == 2).sum() >= 1
        assert ((rows["lb"] != rows["lb_interval"])).sum() >= 20


# ---- 3. / 4. the planes contain what the device's forward produces; certified images keep their class ---------------------------

@lru_cache(maxsize=None)
def integer_perturbations(eps: int):
    """[N, 8, 32, 32, 3] uint8: the images moved by random integers within +-eps, clipped."""
    rng = np.random.default_rng(100 + eps)
    d = rng.integers(-eps, eps + 1, size=(N, 8) + images_np().shape[1:])
    return np.clip(images_np()[:, None].astype(np.int64) + d, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("eps", [1, 2])
def test_planes_contain_the_device_forward(model, dev, eps):
    _, st = spec_and_state("valexnet")
    rows, planes = device_run(model, dev, float(eps))
    v = integer_perturbations(eps).reshape(-1, 32, 32, 3)
    pre = oracle_pre(st, normalise(v.astype(np.float64)))
    near = np.abs(pre) < OB.NEAR_TIE
    bits, feats, logits = [], [], []
    with torch.no_grad():
        for a in range(0, v.shape[0], 256):
            n = min(256, v.shape[0] - a)
            logits.append(model.forward_u8(torch.from_numpy(v[a:a + n]).to(dev)).cpu().numpy())
            bits.append(OB.unpack_rows(model.read_stage("features.4", n), 10))
            feats.append(OB.unpack_rows(model.read_stage("features.5", n), 11))
    bits, feats, logits = (np.concatenate(x).reshape((N, 8) + x[0].shape[1:]) for x in (bits, feats, logits))
    near = near.reshape(N, 8, 64, 10, 10)
    out = (bits < planes["stem_lo"][:, None]) | (bits > planes["stem_hi"][:, None])
    clean = ~near.reshape(N, 8, -1).any(axis=2)                          # perturbed images without a near tie of the oracle
    fout = (feats < planes["feat_lo"][:, None]) | (feats > planes["feat_hi"][:, None])
    print(f"eps {eps}: {int(out.sum())} stem bits outside the planes ({int((out & ~near).sum())} away from a near tie), "
          f"{int(fout[clean].sum())} feature bits outside on the {int(clean.sum())} images without a near tie; "
          f"{int((rows['stage'] > 0).sum())} images certified")
    assert not (out & ~near).any()
    assert clean.sum() >= N * 8 // 2 and not fout[clean].any()
    cert = rows["stage"] > 0                                             # (none with these weights at eps >= 1; kept for weights that have some)
    assert (logits.argmax(axis=2) == classes_np()[:, None])[cert].all()


def test_certified_images_keep_their_class_on_the_device(model, dev):
    rows, _ = device_run(model, dev, 0.01)
    with torch.no_grad():
        logits = model.forward_u8(images(dev)).cpu().numpy()
    strong = (rows["stage"] > 0) & (rows["lb"] > 2 * scaled_tol(logits))
    print(f"eps 0.01: {int((rows['stage'] > 0).sum())} certified, {int(strong.sum())} with lb above twice the logit tolerance")
    assert strong.sum() >= 30
    assert np.array_equal(logits.argmax(axis=1)[strong], classes_np()[strong])
    # the same through min_margin: what is certified with that margin is exactly the strong set
    res = model.certify_u8(images(dev), torch.from_numpy(classes_np()), 0.01, min_margin=2 * scaled_tol(logits)).numpy()
    assert np.array_equal(res["stage"] > 0, rows["lb"] > 2 * scaled_tol(logits))


# ---- 5. batch sizes, lanes, constants ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.03, 1.0])
def test_batch_sizes_and_lanes(model, dev, eps):
    rows, _ = device_run(model, dev, eps)
    x, c = images(dev), torch.from_numpy(classes_np())
    for a, b in ((0, 1), (63, 64), (5, 8)):                              # n = 1, 1, 3
        got = model.certify_u8(x[a:b], c[a:b], eps).numpy()
        assert got.tobytes() == rows[a:b].tobytes(), (a, b)
    assert model.certify_u8(x, c, eps, lane=1).numpy().tobytes() == rows.tobytes()
    big, bp = device_run(model, dev, eps, 257)
    assert big[:N].tobytes() == rows.tobytes()
    _, st = spec_and_state("valexnet")
    want, bounds = CF.certify_cpu(st, tables(model), images_np(257), classes_np(257), eps, stem_planes=(bp["stem_lo"], bp["stem_hi"]),
                                  return_bounds=True)
    ties, masked = compare_rows(big, want, bounds, 1e-9 * sum_abs_A())
    print(f"eps {eps}, 257 images: {ties.size} with another worst class (ties within tol), {masked.size} with lb within tol of min_margin")
    want_lo, want_hi = CF.stem_planes_cpu(st, images_np(257), eps)
    assert np.array_equal(bp["stem_lo"], want_lo) and np.array_equal(bp["stem_hi"], want_hi)


def test_input_norm_is_honoured(model, dev):
    x, c = images(dev), torch.from_numpy(classes_np())
    fresh = new_model(dev, max_batch=N).set_input_norm(*HALF)
    want = fresh.certify_u8(x, c, 0.03, return_planes=True)
    model.set_input_norm(*HALF)
    try:
        got = model.certify_u8(x, c, 0.03, return_planes=True)
        assert got.numpy().tobytes() == want.numpy().tobytes()
        _, st = spec_and_state("valexnet")
        lo, hi = CF.stem_planes_cpu(st, images_np(), 0.03, *HALF)
        p = got.planes_numpy()
        assert np.array_equal(OB.unpack_rows(p["stem_lo"], 10), lo) and np.array_equal(OB.unpack_rows(p["stem_hi"], 10), hi)
    finally:
        model.set_input_norm(cifar.CIFAR_MEAN, cifar.CIFAR_STD)
    assert model.certify_u8(x, c, 0.03).numpy().tobytes() == device_run(model, dev, 0.03)[0].tobytes()


# ---- 6. reload -----------------------------------------------------------------------------------------------------------------------

def test_reload_rebuilds_the_effective_head(dev):
    _, st = spec_and_state("valexnet")
    x, c = images(dev), torch.from_numpy(classes_np())
    m = new_model(dev, max_batch=N)
    before = m.certify_u8(x, c, 0.03).numpy().copy()
    st2 = dict(st)
    rng = np.random.default_rng(3)
    st2["features.7.lin2.weight"] = (st["features.7.lin2.weight"] * rng.uniform(0.5, 1.5, st["features.7.lin2.weight"].shape)).astype(np.float32)
    st2["features.7.BN2.weight"] = (st["features.7.BN2.weight"] * rng.uniform(0.5, 1.5, 100)).astype(np.float32)
    st2["features.7.BN2.bias"] = (st["features.7.BN2.bias"] + rng.uniform(-0.1, 0.1, 100)).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st2.items()}, strict=True)
    after = m.certify_u8(x, c, 0.03).numpy().copy()
    fresh = new_model(dev, st2, max_batch=N).certify_u8(x, c, 0.03).numpy()
    assert after.tobytes() == fresh.tobytes()
    assert not np.array_equal(after["lb_interval"], before["lb_interval"])
    want, bounds = CF.certify_cpu(st2, {b.name: m.get_table(b.name) for b in m.spec.block_tts()}, images_np(), classes_np(), 0.03,
                                  return_bounds=True)
    A2 = CF.effective_head(st2)[0]
    ties, masked = compare_rows(after, want, bounds, 1e-9 * float(np.abs(A2).sum()))
    print(f"reloaded head: {ties.size} with another worst class (ties within tol), {masked.size} with lb within tol of min_margin")


# ---- 7. error contract ------------------------------------------------------------------------------------------------------------------

def test_error_contract_of_the_c_abi(model, dev):
    plan = model._any_plan()
    lib = plan.lib
    x, c = images(dev)[:4], torch.from_numpy(classes_np()[:4]).to(dev, torch.int32)
    rows = torch.empty((4, 4), dtype=torch.float64, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(x_ptr=x.data_ptr(), lane=0, n=4, c_ptr=c.data_ptr(), eps=0.03, enum=10, mm=1e-6, r_ptr=rows.data_ptr(), p_ptr=None, h=plan.handle):
        return lib.ttnet_certify_u8(h, lane, C.c_void_p(x_ptr), n, C.c_void_p(c_ptr), eps, enum, mm, C.c_void_p(r_ptr), C.c_void_p(p_ptr), s)
    assert call() == 0
    for kw in (dict(eps=-0.5), dict(eps=float("inf")), dict(eps=float("nan")), dict(enum=-1), dict(enum=13), dict(lane=2), dict(lane=-1),
               dict(n=0), dict(n=258), dict(x_ptr=x.data_ptr() + 1), dict(c_ptr=c.data_ptr() + 2), dict(r_ptr=rows.data_ptr() + 4),
               dict(p_ptr=rows.data_ptr() + 4), dict(x_ptr=None), dict(c_ptr=None), dict(r_ptr=None), dict(mm=float("nan"))):
        assert call(**kw) == -1, kw
        assert lib.ttnet_last_error()
    # a class outside 0..9 is not an error of the call: the record says so
    bad = torch.tensor([int(classes_np()[0]), 10, -1, 1 << 20], dtype=torch.int32, device=dev)
    got = model.certify_u8(x, bad, 0.03).numpy()
    assert got[0].tobytes() == device_run(model, dev, 0.03)[0][0].tobytes()
    assert got["stage"][1:].tolist() == [0, 0, 0] and got["worst"][1:].tolist() == [-1, -1, -1]
    assert (got["lb"][1:] == -np.inf).all() and (got["lb_interval"][1:] == -np.inf).all()
    assert np.array_equal(got["unknown_stem"], device_run(model, dev, 0.03)[0]["unknown_stem"][:4])
    # any other variant: -4, and the message names the reason
    small = ttnet._Plan(spec_and_state("small")[0], args_for("small"), 0, 2)
    try:
        assert call(h=small.handle) == -4
        msg = lib.ttnet_last_error().decode()
        assert "affine head" in msg and "8 inputs" in msg
    finally:
        small.close()
    # a plan that was never finalized: -2, and the message names this call
    raw = ttnet._Plan(spec_and_state("valexnet")[0], args_for("valexnet"), 0, 4)
    try:
        assert call(h=raw.handle) == -2
        assert "ttnet_certify_u8 before ttnet_plan_finalize" in lib.ttnet_last_error().decode()
    finally:
        raw.close()
    with pytest.raises(RuntimeError, match="vAlexnet"):
        ttnet.TT_vf_19lv3_imgnet_xsmall(args_for("xsmall")).eval().certify_u8(x, c, 0.03)
    with pytest.raises(ValueError):
        model.certify_u8(x, c, 0.03, enum_bits=13)
    with pytest.raises(RuntimeError):
        model.certify_u8(x.cpu(), c, 0.03)


# ---- 8. the command ----------------------------------------------------------------------------------------------------------------------

def test_command_prints_verified_lines(model, dev, tmp_path, capsys):
    n = 300
    u8 = synth.synth_images_u8(n, hw=(32, 32))
    labels = (np.arange(n) % 10).astype(np.int64)
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([labels[:, None].astype(np.uint8), u8.reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
    x = np.ascontiguousarray(u8.transpose(0, 2, 3, 1))
    sums = CF.certify_batches(model, cifar.device_batches(x, labels, 128, dev), [0.03, 1.0])
    assert [s["images"] for s in sums] == [n, n] and sums[0]["certified"] == sums[0]["interval"] + sums[0]["enumeration"]
    whole = model.certify_u8(torch.from_numpy(x[:257]).to(dev), torch.from_numpy(labels[:257]), 0.03).numpy()
    assert sums[0]["rows"][:257].tobytes() == whole.tobytes()            # dataset order across the batches
    capsys.readouterr()
    assert cifar.main(["--data_dir", str(tmp_path), "--synthetic-ckpt", "--eval_batch_size", "128"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert len(plain) == 1 and re.fullmatch(r"Acc\.\. (\S+) (\S+)", plain[0])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    rows_file = tmp_path / "r.csv"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "scale_imagenet_amd.cifar", "--data_dir", str(tmp_path),
                        "--synthetic-ckpt", "--eval_batch_size", "128", "--certify", "0.03,1", "--certify_rows", str(rows_file)],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert out == [plain[0]] + [CF.verified_line(s) for s in sums], r.stdout
    assert out[1].startswith(f"Verified.. eps=0.03 {sums[0]['certified']}/{n} ")
    with open(rows_file, newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 2 * n
    for s, part in zip(sums, (got[:n], got[n:])):
        assert np.array_equal(np.array([float(g["lb"]) for g in part]), s["rows"]["lb"])
        assert [int(g["stage"]) for g in part] == s["rows"]["stage"].tolist()
        assert [int(g["class"]) for g in part] == labels.tolist()
    assert sorted(os.listdir(tmp_path)) == ["cifar-10-batches-bin", "r.csv"]
