"""GPU: ttnet_certify_box_u8 and ttnet_certify_patch_u8 (csrc/certify.hip) against ttnet_certify_u8, against the numpy float64
twins (scale_imagenet_amd/certify.py: certify_box_cpu, certify_patch_cpu), against each other, and against the device's forward.

Synthetic weights, synthetic images 0, 1 and 7, the classes the float64 oracle gives them.  Standard of comparison, as in
test_gpu_certify.py: integers identical, bounds within 1e-9 * sum|A|; a stage may differ only where a bound lies within that
distance of min_margin, which happens nowhere for these inputs (asserted: zero excused positions)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from _util import args_for, scaled_tol, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import ttnet
from test_gpu_certify import classes_np, compare_rows, images, images_np, new_model, sum_abs_A, tables

pytestmark = pytest.mark.gpu

IMGS = (0, 1, 7)
SWEEPS = (((1, 1), 1, 255), ((4, 4), 4, 1), ((2, 3), 3, 8), ((2, 5), 3, 255), ((8, 8), 8, 255))
# (certified by stage 1, by stage 2, open) of images 0, 1, 7: the prototype's table for this checkpoint
TABLE = {((1, 1), 1, 255): ((78, 56, 890), (153, 80, 791), (330, 2, 692)), ((4, 4), 4, 1): ((22, 22, 20), (60, 4, 0), (64, 0, 0)),
         ((2, 3), 3, 8): ((6, 18, 86), (34, 20, 56), (80, 0, 30))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    m = new_model(dev).set_lanes(2)
    with torch.no_grad():
        m.forward_u8(images(dev)[:1])                       # (creates the plan: get_table needs one)
    return m


def x3_np():
    return images_np()[list(IMGS)]


def c3_np():
    return classes_np()[list(IMGS)]


_TWIN = {}


def twin_of(model, patch, stride, amp, enum_bits=10):
    """(rows, map) of certify_patch_cpu for the three images; computed once per setting."""
    key = (patch, stride, amp, enum_bits)
    if key not in _TWIN:
        _TWIN[key] = CF.certify_patch_cpu(spec_and_state("valexnet")[1], tables(model), x3_np(), c3_np(), patch, stride, amp, enum_bits=enum_bits)
    return _TWIN[key]


def compare_maps(got, want, tol, min_margin=1e-6):
    """Device position records against reference records of the same shape.  Returns the number of positions whose bound lies
    within tol of min_margin (for which alone the stage may differ)."""
    assert got.shape == want.shape
    assert np.array_equal(got["unknown_stem"], want["unknown_stem"])
    fin = np.isfinite(want["lb"])
    assert np.array_equal(fin, np.isfinite(got["lb"])) and np.array_equal(got["lb"][~fin], want["lb"][~fin])
    err = np.abs(got["lb"][fin] - want["lb"][fin]).max(initial=0.0)
    assert err <= tol, err
    clear = np.abs(want["lb"] - min_margin) > tol
    assert np.array_equal(got["stage"][clear], want["stage"][clear])
    assert np.array_equal(got["worst"][clear], want["worst"][clear])
    return int((~clear).sum()), err


# ---- 1. / 2. the box certificate -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [1, 2])
def test_box_of_an_eps_equals_certify_u8(model, dev, eps):
    x, c = images(dev), torch.from_numpy(classes_np())
    want = model.certify_u8(x, c, float(eps), return_planes=True)
    lo = (x.to(torch.int16) - eps).clamp(0, 255).to(torch.uint8)
    hi = (x.to(torch.int16) + eps).clamp(0, 255).to(torch.uint8)
    got = model.certify_box_u8(lo, hi, c, return_planes=True)
    assert got.numpy().tobytes() == want.numpy().tobytes()
    for k, v in want.planes_numpy().items():
        assert np.array_equal(got.planes_numpy()[k], v), k
    assert model.certify_box_u8(x, x, c).numpy().tobytes() == model.certify_u8(x, c, 0.0).numpy().tobytes()
    with pytest.raises(ValueError):
        model.certify_box_u8(hi, lo, c)


@lru_cache(maxsize=None)
def odd_boxes():
    """257 boxes that are no eps boxes: 200 of the 1x1 / 255 sweep of image 0 (every fifth position) and 57 2x5 / 255 patches of
    image 1."""
    lo0, hi0 = CF.patch_boxes(images_np()[0], (1, 1), 1, 255)
    lo1, hi1 = CF.patch_boxes(images_np()[1], (2, 5), 3, 255)
    lo, hi = np.concatenate([lo0[::5][:200], lo1[:57]]), np.concatenate([hi0[::5][:200], hi1[:57]])
    cls = np.concatenate([np.full(200, classes_np()[0]), np.full(57, classes_np()[1])])
    assert lo.shape[0] == 257
    return lo, hi, cls


def test_box_of_patches_equals_the_twin(model, dev):
    _, st = spec_and_state("valexnet")
    lo, hi, cls = odd_boxes()
    res = model.certify_box_u8(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev), torch.from_numpy(cls), return_planes=True)
    rows = res.numpy()
    planes = {k: OB.unpack_rows(v, 10 if k.startswith("stem") else 11) for k, v in res.planes_numpy().items()}
    want_lo, want_hi = CF.stem_planes_box_cpu(st, lo, hi)
    assert np.array_equal(planes["stem_lo"], want_lo) and np.array_equal(planes["stem_hi"], want_hi)
    want, wp, bounds = CF.certify_box_cpu(st, tables(model), lo, hi, cls, stem_planes=(planes["stem_lo"], planes["stem_hi"]),
                                          return_planes=True, return_bounds=True)
    assert np.array_equal(planes["feat_lo"], wp["feat_lo"]) and np.array_equal(planes["feat_hi"], wp["feat_hi"])
    ties, masked = compare_rows(rows, want, bounds, 1e-9 * sum_abs_A())
    print(f"257 patch boxes: stages {np.bincount(rows['stage'], minlength=3).tolist()}, {ties.size} ties, {masked.size} within tol of min_margin")
    assert ties.size == 0 and masked.size == 0
    assert (rows["stage"] == 1).any() and (rows["stage"] == 2).any() and (rows["stage"] == 0).any()


# ---- 3. the sweep against its twin --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("patch,stride,amp", SWEEPS)
def test_sweep_equals_the_twin(model, dev, patch, stride, amp):
    x, c = torch.from_numpy(x3_np()).to(dev), torch.from_numpy(c3_np())
    rows, maps = model.certify_patch_u8(x, c, patch, stride, amp).numpy()
    want_rows, want = twin_of(model, patch, stride, amp)
    tol = 1e-9 * sum_abs_A()
    excused, err = compare_maps(maps, want, tol)
    counts = [tuple(int((maps[i]["stage"] == s).sum()) for s in (1, 2, 0)) for i in range(3)]
    print(f"{patch} stride {stride} amp {amp}: {maps[0].size} positions, (stage 1, stage 2, open) {counts}, largest |lb - twin| {err:.2e} "
          f"(tol {tol:.2e}), {excused} excused, unknown stem bits at most {int(maps['unknown_stem'].max())}")
    assert excused == 0
    if (patch, stride, amp) in TABLE:
        assert tuple(counts) == TABLE[(patch, stride, amp)]
    mine = CF.patch_rows_from_map(maps)                                  # the image rows, recomputed from the device's map
    assert rows.tobytes() == mine.tobytes()
    assert np.array_equal(rows["positions"], np.full(3, maps[0].size))
    assert np.array_equal(rows["certified"], want_rows["certified"])


# ---- 4. the sweep against the device's own box certificate -----------------------------------------------------------------------

def test_sweep_equals_the_box_certificate_of_every_position(model, dev):
    x, c = images(dev)[:1], torch.from_numpy(classes_np()[:1])
    _, maps = model.certify_patch_u8(x, c, (1, 1), 1, 255).numpy()
    lo, hi = CF.patch_boxes(images_np()[0], (1, 1), 1, 255)
    cls = torch.full((256,), int(classes_np()[0]), dtype=torch.int64)
    parts = [model.certify_box_u8(torch.from_numpy(lo[a:a + 256]).to(dev), torch.from_numpy(hi[a:a + 256]).to(dev), cls).numpy().copy()
             for a in range(0, 1024, 256)]
    box = np.concatenate(parts)
    want = np.zeros(1024, dtype=CF.MAP_RECORD)
    for col in want.dtype.names:
        want[col] = box[col]
    excused, err = compare_maps(maps.reshape(-1), want, 1e-9 * sum_abs_A())
    print(f"1x1 / 255 of image 0 against 1,024 box certificates: largest |lb difference| {err:.2e}, {excused} excused")
    assert excused == 0


# ---- 5. soundness through the device's forward --------------------------------------------------------------------------------------

@pytest.mark.parametrize("img,patch,stride,amp,limit", [(7, (2, 3), 3, 8, None), (0, (1, 1), 1, 255, 64)])
def test_certified_positions_keep_the_class_on_the_device(model, dev, img, patch, stride, amp, limit):
    x0 = images_np()[img]
    c = int(classes_np()[img])
    _, maps = model.certify_patch_u8(torch.from_numpy(x0[None].copy()).to(dev), torch.tensor([c]), patch, stride, amp).numpy()
    org = CF.patch_origins(patch, stride)
    cert = np.flatnonzero(maps.reshape(-1)["stage"] > 0)[:limit]
    assert cert.size >= (64 if limit else 80)
    rng = np.random.default_rng(17)
    h, w = patch
    v = np.broadcast_to(x0, (cert.size, 8, 32, 32, 3)).copy()
    for k, p in enumerate(cert):
        y0, xx = org[p]
        b = x0[y0:y0 + h, xx:xx + w].astype(np.int64)
        lo, hi = np.maximum(0, b - amp), np.minimum(255, b + amp)
        v[k, 0, y0:y0 + h, xx:xx + w], v[k, 1, y0:y0 + h, xx:xx + w] = lo, hi
        v[k, 2:, y0:y0 + h, xx:xx + w] = rng.integers(lo, hi + 1, size=(6,) + b.shape)
    v = v.reshape(-1, 32, 32, 3)
    with torch.no_grad():
        logits = np.concatenate([model.forward_u8(torch.from_numpy(v[a:a + 256]).to(dev)).cpu().numpy() for a in range(0, len(v), 256)])
    tol = scaled_tol(logits)
    own = logits[:, c].copy()
    logits[:, c] = -np.inf
    margin = own - logits.max(axis=1)
    print(f"image {img} {patch} amp {amp}: {cert.size} certified positions, {len(v)} fills, smallest device margin {margin.min():.3e} "
          f"(tolerance {tol:.1e})")
    assert (margin > -tol).all()


# ---- 6. determinism, lanes, independence of the batch ------------------------------------------------------------------------------------

def test_same_bytes_on_every_run_lane_and_batch(model, dev):
    x, c = torch.from_numpy(x3_np()).to(dev), torch.from_numpy(c3_np())
    first = model.certify_patch_u8(x, c, (2, 3), 3, 8)
    rows, maps = (a.copy() for a in first.numpy())
    for lane in (0, 1):
        r2, m2 = model.certify_patch_u8(x, c, (2, 3), 3, 8, lane=lane).numpy()
        assert r2.tobytes() == rows.tobytes() and m2.tobytes() == maps.tobytes()
    r1, m1 = model.certify_patch_u8(x[1:2], c[1:2], (2, 3), 3, 8).numpy()             # image 1 alone: index 0 of 1, index 1 of 3
    assert m1[0].tobytes() == maps[1].tobytes() and r1[0].tobytes() == rows[1].tobytes()
    order = [2, 0, 1]
    r3, m3 = model.certify_patch_u8(x[order], c[order], (2, 3), 3, 8).numpy()
    assert m3[2].tobytes() == maps[1].tobytes() and m3[0].tobytes() == maps[2].tobytes()


# ---- 7. classes outside 0..9, no stage 2, the error list ----------------------------------------------------------------------------------------

def test_bad_classes_enum_zero_and_errors(model, dev):
    x, c = torch.from_numpy(x3_np()).to(dev), torch.from_numpy(c3_np())
    good = model.certify_patch_u8(x, c, (4, 4), 4, 1).numpy()[1].copy()
    bad = torch.tensor([10, int(c3_np()[1]), -1])
    rows, maps = model.certify_patch_u8(x, bad, (4, 4), 4, 1).numpy()
    assert maps[1].tobytes() == good[1].tobytes()
    for i in (0, 2):
        assert (maps[i]["stage"] == 0).all() and (maps[i]["worst"] == -1).all() and (maps[i]["lb"] == -np.inf).all()
        assert np.array_equal(maps[i]["unknown_stem"], good[i]["unknown_stem"])
        assert rows[i]["certified"] == 0 and rows[i]["worst"] == -1 and rows[i]["lb_min"] == -np.inf and rows[i]["pos_min"] == 0
    _, m0 = model.certify_patch_u8(x, c, (4, 4), 4, 1, enum_bits=0).numpy()            # no stage 2: the table's first figures
    assert [int((m0[i]["stage"] == 1).sum()) for i in range(3)] == [22, 60, 64] and not (m0["stage"] == 2).any()
    want0 = twin_of(model, (4, 4), 4, 1, enum_bits=0)[1]
    assert compare_maps(m0, want0, 1e-9 * sum_abs_A())[0] == 0

    plan = model._any_plan()
    lib = plan.lib
    ci = c.to(dev, torch.int32)
    rows_t = torch.zeros((3, 4), dtype=torch.float64, device=dev)
    map_t = torch.zeros((3, 64, 2), dtype=torch.float64, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(x_ptr=x.data_ptr(), lane=0, n=3, c_ptr=ci.data_ptr(), h=4, w=4, stride=4, amp=1, enum=10, mm=1e-6, r_ptr=rows_t.data_ptr(),
             m_ptr=map_t.data_ptr(), handle=plan.handle):
        return lib.ttnet_certify_patch_u8(handle, lane, C.c_void_p(x_ptr), n, C.c_void_p(c_ptr), h, w, stride, amp, enum, mm,
                                          C.c_void_p(r_ptr), C.c_void_p(m_ptr), s)

    def call_box(lo_ptr=x.data_ptr(), hi_ptr=x.data_ptr(), handle=plan.handle, enum=10):
        return lib.ttnet_certify_box_u8(handle, 0, C.c_void_p(lo_ptr), C.c_void_p(hi_ptr), 3, C.c_void_p(ci.data_ptr()), enum, 1e-6,
                                        C.c_void_p(rows_t.data_ptr()), C.c_void_p(None), s)
    torch.cuda.synchronize(dev)
    for kw in (dict(h=0), dict(h=9), dict(w=0), dict(w=9), dict(stride=0), dict(stride=33), dict(amp=0), dict(amp=256), dict(enum=-1),
               dict(enum=13), dict(lane=2), dict(lane=-1), dict(n=0), dict(n=258), dict(x_ptr=x.data_ptr() + 1), dict(c_ptr=ci.data_ptr() + 2),
               dict(r_ptr=rows_t.data_ptr() + 4), dict(m_ptr=map_t.data_ptr() + 4), dict(x_ptr=None), dict(c_ptr=None), dict(r_ptr=None),
               dict(m_ptr=None), dict(mm=float("nan"))):
        assert call(**kw) == -1, kw
        assert lib.ttnet_last_error()
    for kw in (dict(hi_ptr=None), dict(lo_ptr=None), dict(hi_ptr=x.data_ptr() + 2), dict(enum=13)):
        assert call_box(**kw) == -1, kw
    torch.cuda.synchronize(dev)
    assert not rows_t.any() and not map_t.any()                          # nothing was launched
    assert call() == 0 and call_box() == 0
    small = ttnet._Plan(spec_and_state("small")[0], args_for("small"), 0, 4)
    try:
        assert call(handle=small.handle) == -4 and "affine head" in lib.ttnet_last_error().decode()
        assert call_box(handle=small.handle) == -4
    finally:
        small.close()
    raw = ttnet._Plan(spec_and_state("valexnet")[0], args_for("valexnet"), 0, 4)
    try:
        assert call(handle=raw.handle) == -2 and "ttnet_certify_patch_u8 before ttnet_plan_finalize" in lib.ttnet_last_error().decode()
        assert call_box(handle=raw.handle) == -2
        # the plan's state is judged before what only these entries take, as for every other argument
        assert call(handle=raw.handle, m_ptr=None) == -2 and call(handle=raw.handle, h=9) == -2 and call_box(handle=raw.handle, hi_ptr=None) == -2
    finally:
        raw.close()
    with pytest.raises(RuntimeError, match="vAlexnet"):
        ttnet.TT_vf_19lv3_imgnet_xsmall(args_for("xsmall")).eval().certify_patch_u8(x, c, (2, 2))
    for kw in (dict(patch=(0, 1)), dict(patch=(9, 1)), dict(patch=(2,)), dict(stride=0), dict(amp=0), dict(amp=256), dict(enum_bits=13),
               dict(amp=1.5)):
        with pytest.raises(ValueError):
            model.certify_patch_u8(x, c, **{"patch": (2, 2), **kw})


# ---- 8. batches and the command ----------------------------------------------------------------------------------------------------------------

def test_batches_and_the_command_print_patch_lines(model, dev, tmp_path, capsys):
    import csv
    import os
    import subprocess
    import sys

    from _util import ROOT
    from scale_imagenet_amd import cifar, synth
    n = 300
    u8 = synth.synth_images_u8(n, hw=(32, 32))
    labels = (np.arange(n) % 10).astype(np.int64)
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([labels[:, None].astype(np.uint8), u8.reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
    x = np.ascontiguousarray(u8.transpose(0, 2, 3, 1))
    sums = CF.certify_patch_batches(model, cifar.device_batches(x, labels, 128, dev), [(4, 4), (2, 3)], 4, 8)   # batches of 128, 128, 44
    assert [s["images"] for s in sums] == [n, n] and [s["positions"] for s in sums] == [n * 64, n * 64]
    assert sums[0]["map"].shape == (n, 8, 8) and sums[1]["map"].shape == (n, 8, 8) and sums[0]["rows"].shape == (n,)
    for s, p in zip(sums, ((4, 4), (2, 3))):                             # dataset order across the batches: one whole call of 257
        rows, maps = model.certify_patch_u8(torch.from_numpy(x[:257]).to(dev), torch.from_numpy(labels[:257]), p, 4, 8).numpy()
        assert s["rows"][:257].tobytes() == rows.tobytes() and s["map"][:257].tobytes() == maps.tobytes()
        assert s["certified"] == int((s["rows"]["certified"] == 64).sum()) and s["positions_certified"] == s["interval"] + s["enumeration"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    base = ["timeout", "-k", "10", "300", sys.executable, "-m", "scale_imagenet_amd.cifar", "--data_dir", str(tmp_path), "--synthetic-ckpt",
            "--eval_batch_size", "128", "--certify", "0.03"]
    rows_file, map_file = tmp_path / "r.csv", tmp_path / "m.npz"
    capsys.readouterr()
    assert cifar.main(base[7:]) == 0                                     # the same command without the patch flags, in this process
    old = capsys.readouterr().out.splitlines()
    r = subprocess.run(base + ["--certify_patch", "4x4,2x3", "--patch_stride", "4", "--patch_amp", "8", "--patch_rows", str(rows_file),
                               "--patch_map", str(map_file)], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(old) == 2 and old[0].startswith("Acc.. ") and old[1].startswith("Verified.. eps=0.03 ")
    assert out == old + [CF.patch_line(s) for s in sums], r.stdout      # the lines of before, unchanged, then one per size
    assert out[2].startswith(f"Patch.. size=4x4 amp=8 stride=4 sampled {sums[0]['certified']}/{n} ")
    with open(rows_file, newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 2 * n and [int(g["class"]) for g in got[:n]] == labels.tolist()
    assert np.array_equal(np.array([float(g["lb_min"]) for g in got[n:]]), sums[1]["rows"]["lb_min"])
    with np.load(map_file) as z:
        assert np.array_equal(z["lb_4x4"], sums[0]["map"]["lb"]) and np.array_equal(z["stage_2x3"], sums[1]["map"]["stage"])
    assert sorted(os.listdir(tmp_path)) == ["cifar-10-batches-bin", "m.npz", "r.csv"]
