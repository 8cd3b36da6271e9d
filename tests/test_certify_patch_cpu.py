"""CPU: the numpy float64 twins of the box certificate and of the patch sweep (scale_imagenet_amd/certify.py: certify_box_cpu,
certify_patch_cpu) on the synthetic vAlexnet checkpoint and synthetic images 0, 1 and 7 -- the eps box as a case of the box
certificate, the incremental sweep against the box certificate of every materialised position, the prototype's counts,
soundness by sampling through the float64 oracle, the edges, and the command's flags, line and files.

The counts pinned here are facts about the synthetic checkpoint, not about a trained network."""
import csv
import os
from functools import lru_cache

import numpy as np
import pytest

from _certify_util import normalise, oracle_pre
from _util import spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar, synth
from scale_imagenet_amd.valexnet_block import field_span, patch_positions

IMGS = (0, 1, 7)
# patch, stride, amp -> (certified by stage 1, by stage 2, left open) of images 0, 1, 7: the prototype's table
TABLE = {((1, 1), 1, 255): ((78, 56, 890), (153, 80, 791), (330, 2, 692)),
         ((1, 1), 1, 16): ((438, 286, 300), (931, 86, 7), (1023, 1, 0)),
         ((4, 4), 4, 1): ((22, 22, 20), (60, 4, 0), (64, 0, 0)),
         ((2, 3), 3, 8): ((6, 18, 86), (34, 20, 56), (80, 0, 30)),
         ((3, 3), 1, 255): ((1, 2, 897), (1, 2, 897), (25, 0, 875))}
SWEEPS = tuple(TABLE) + (((2, 5), 3, 255), ((8, 8), 8, 255))


@lru_cache(maxsize=None)
def setup():
    spec, st = spec_and_state("valexnet")
    luts, near = OB.build_all_luts(st, spec)
    assert not any(v.any() for v in near.values())
    x = np.ascontiguousarray(synth.synth_images_u8(8, hw=(32, 32)).transpose(0, 2, 3, 1))
    x.setflags(write=False)
    pre = oracle_pre(st, normalise(x.astype(np.float64)))
    cls = OB.valexnet_from_stem_bits((pre >= 0).astype(np.uint8), st, spec, luts)[1].argmax(axis=1)
    return spec, st, luts, x, cls


def sweep_with_planes(patch, stride, amp, img=None):
    """certify_patch_cpu of images 0, 1, 7 (img None) or of one image, with the planes of every position (76 MB per 1,024
    positions: not kept)."""
    _, st, luts, x, cls = setup()
    sel = list(IMGS) if img is None else [img]
    return CF.certify_patch_cpu(st, luts, x[sel], cls[sel], patch, stride, amp, return_planes=True)


@lru_cache(maxsize=None)
def sweep(patch, stride, amp, img=None):
    """(rows, map) of the same; computed once."""
    _, st, luts, x, cls = setup()
    sel = list(IMGS) if img is None else [img]
    return CF.certify_patch_cpu(st, luts, x[sel], cls[sel], patch, stride, amp)


def tol():
    return 1e-9 * float(np.abs(CF.effective_head(setup()[1])[0]).sum())


# ---- 1. the eps box is a case of the box certificate -------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0, 1, 2])
def test_box_of_an_eps_equals_certify_cpu(eps):
    _, st, luts, x, cls = setup()
    lo = np.clip(x.astype(np.int64) - eps, 0, 255).astype(np.uint8)
    hi = np.clip(x.astype(np.int64) + eps, 0, 255).astype(np.uint8)
    assert eps > 0 or np.array_equal(lo, hi)
    want, wp = CF.certify_cpu(st, luts, x, cls, float(eps), return_planes=True)
    got, gp = CF.certify_box_cpu(st, luts, lo, hi, cls, return_planes=True)
    assert got.tobytes() == want.tobytes()
    assert all(np.array_equal(gp[k], wp[k]) for k in wp)


# ---- 2. / 3. the incremental sweep against the box certificate of every position; the prototype's counts ---------------------------

@pytest.mark.parametrize("patch,stride,amp", SWEEPS)
def test_sweep_equals_the_box_certificate_of_every_position(patch, stride, amp):
    _, st, luts, x, cls = setup()
    excused, worst_err, closest = 0, 0.0, np.inf
    for i in IMGS:
        rows, maps, planes = sweep_with_planes(patch, stride, amp, i)
        got, planes = maps[0].reshape(-1), planes[0]
        lo, hi = CF.patch_boxes(x[i], patch, stride, amp)
        assert lo.shape[0] == got.size == patch_positions(patch[0], stride) * patch_positions(patch[1], stride)
        for a in range(0, got.size, 256):
            n = min(256, got.size - a)
            want, wp = CF.certify_box_cpu(st, luts, lo[a:a + n], hi[a:a + n], np.full(n, cls[i]), return_planes=True)
            for k in wp:                                                 # the same three-valued planes
                assert np.array_equal(planes[k][a:a + n], wp[k]), (i, k, a)
            g = got[a:a + n]
            assert np.array_equal(g["unknown_stem"], want["unknown_stem"])
            err = np.abs(g["lb"] - want["lb"]).max()
            assert err <= tol(), (i, a, err)
            # the box twin decides: the twin's stage 2 takes the first of equal minima, as the box twin's does, so no count moves
            assert np.array_equal(g["worst"], want["worst"]) and np.array_equal(g["stage"], want["stage"])
            excused += int((np.abs(want["lb"] - 1e-6) <= tol()).sum())
            worst_err, closest = max(worst_err, float(err)), min(closest, float(np.abs(want["lb"] - 1e-6).min()))
        assert rows.tobytes() == CF.patch_rows_from_map(maps).tobytes()
        if (patch, stride, amp) in TABLE:
            s = got["stage"]
            assert (int((s == 1).sum()), int((s == 2).sum()), int((s == 0).sum())) == TABLE[(patch, stride, amp)][IMGS.index(i)], i
            assert (rows["interval"][0], rows["enumeration"][0], rows["positions"][0]) == (int((s == 1).sum()), int((s == 2).sum()), s.size)
    print(f"{patch} stride {stride} amp {amp}: largest |lb - box twin| {worst_err:.2e} (tol {tol():.2e}), closest bound to min_margin "
          f"{closest:.2e}, {excused} excused")
    assert excused == 0 and closest >= 8e-5


def test_whole_image_certificates_and_unknown_bits():
    """Stage 1, stage 2, open positions and whole-image certificates all occur."""
    for key, img in ((((4, 4), 4, 1), 7), (((1, 1), 1, 16), 7), (((4, 4), 4, 1), 1)):
        rows = sweep(*key, img)[0]
        assert rows["certified"][0] == rows["positions"][0], (key, img)
    rows, maps = sweep((4, 4), 4, 1, 1)
    assert (rows["interval"][0], rows["enumeration"][0]) == (60, 4)
    rows, maps = sweep((1, 1), 1, 255, 0)
    assert (rows["interval"][0], rows["enumeration"][0], rows["certified"][0], rows["positions"][0]) == (78, 56, 134, 1024)
    assert rows["lb_min"][0] == maps["lb"].min() and maps.reshape(-1)["lb"][rows["pos_min"][0]] == rows["lb_min"][0]
    kmax = [int(sweep((1, 1), 1, 255, i)[1]["unknown_stem"].max()) for i in IMGS]
    assert min(kmax) == 36 and max(kmax) == 45
    assert int(sweep((4, 4), 4, 1)[1]["unknown_stem"].max()) == 8
    s = CF.summarise_patch((4, 4), 4, 1, *sweep((4, 4), 4, 1))
    assert (s["images"], s["certified"], s["positions"], s["positions_certified"]) == (3, 2, 192, 172)


# ---- 4. soundness by sampling through the float64 oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize("patch,stride,amp", [((1, 1), 1, 255), ((2, 3), 3, 8)])
@pytest.mark.parametrize("img", [0, 7])
def test_sampled_fills_stay_inside(patch, stride, amp, img):
    spec, st, luts, x, cls = setup()
    rows, maps, planes = sweep_with_planes(patch, stride, amp, img)
    maps, planes, c = maps[0].reshape(-1), planes[0], int(cls[img])
    cert = np.flatnonzero(maps["stage"] > 0)
    assert cert.size >= 20
    org = CF.patch_origins(patch, stride)
    h, w = patch
    rng = np.random.default_rng(40 + img)
    v = np.broadcast_to(x[img].astype(np.float64), (cert.size, 16, 32, 32, 3)).copy()
    for k, p in enumerate(cert):
        y0, x0 = org[p]
        b = x[img, y0:y0 + h, x0:x0 + w].astype(np.float64)
        lo, hi = np.maximum(0.0, b - amp), np.minimum(255.0, b + amp)
        fills = np.empty((16,) + b.shape)
        fills[0], fills[1] = lo, hi
        fills[2:8] = np.where(rng.integers(0, 2, size=(6,) + b.shape) == 1, hi, lo)       # random corners
        fills[8:] = rng.uniform(lo, hi, size=(8,) + b.shape)                              # random interior
        v[k, :, y0:y0 + h, x0:x0 + w] = fills
    pre = oracle_pre(st, normalise(v.reshape(-1, 32, 32, 3)))
    bits = (pre >= 0).astype(np.uint8)
    y, logits = OB.valexnet_from_stem_bits(bits, st, spec, luts)
    bits, y, logits = bits.reshape(cert.size, 16, 64, 10, 10), y.reshape(cert.size, 16, 256, 11, 11), logits.reshape(cert.size, 16, 10)
    assert (bits >= planes["stem_lo"][cert][:, None]).all() and (bits <= planes["stem_hi"][cert][:, None]).all()
    assert (y >= planes["feat_lo"][cert][:, None]).all() and (y <= planes["feat_hi"][cert][:, None]).all()
    own = logits[:, :, c].copy()
    logits[:, :, c] = -np.inf
    margin = own - logits.max(axis=2)
    print(f"image {img} {patch} amp {amp}: {cert.size} certified positions, smallest sampled margin minus lb "
          f"{float((margin - maps['lb'][cert][:, None]).min()):.3e}")
    assert (margin >= maps["lb"][cert][:, None] - 1e-9).all()


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------

def test_field_spans_and_position_counts():
    for y0 in range(32):
        for h in range(1, 9):
            if y0 + h > 32:
                continue
            cells = [py for py in range(10) if 3 * py - 1 <= y0 + h - 1 and 3 * py + 3 >= y0]
            first, count = field_span(y0, h)
            assert count == len(cells) <= 4 and (not cells or first == cells[0]), (y0, h)
    assert field_span(31, 1) == (10, 0) and field_span(0, 1) == (0, 1) and field_span(2, 8) == (0, 4)
    assert patch_positions(1, 1) == 32 and patch_positions(8, 8) == 4 and patch_positions(4, 4) == 8 and patch_positions(2, 3) == 11
    assert patch_positions(8, 32) == 1 and patch_positions(3, 3) == 10
    org = CF.patch_origins((2, 5), 3)
    assert org.shape == (11 * 10, 2) and org[0].tolist() == [0, 0] and org[1].tolist() == [0, 3] and org[-1].tolist() == [30, 27]


def test_corner_and_the_row_and_column_no_field_reaches():
    _, st, luts, x, cls = setup()
    rows, maps = sweep((1, 1), 1, 255, 0)
    clean = CF.certify_cpu(st, luts, x[:1], cls[:1], 0.0)[0]
    m = maps[0]
    # row 31 and column 31 lie in no field: the clean record, bit for bit
    for rec in list(m[31, :]) + list(m[:, 31]):
        assert rec["lb"] == clean["lb"] and rec["worst"] == clean["worst"] and rec["stage"] == clean["stage"]
        assert rec["unknown_stem"] == clean["unknown_stem"] == 0
    # a patch at (0, 0) moves cell (0, 0) only, which has the zero padding above and to the left of it
    _, _, planes = sweep_with_planes((1, 1), 1, 255, 0)
    lo, hi = planes[0]["stem_lo"][0], planes[0]["stem_hi"][0]
    un = lo != hi
    assert un.any() and not un[:, 1:, :].any() and not un[:, :, 1:].any()
    lo_b, hi_b = CF.patch_boxes(x[0], (1, 1), 1, 255)
    want = CF.certify_box_cpu(st, luts, lo_b[:1], hi_b[:1], cls[:1])[0]
    assert m[0, 0]["stage"] == want["stage"] and m[0, 0]["unknown_stem"] == want["unknown_stem"] and abs(m[0, 0]["lb"] - want["lb"]) <= tol()


def test_amp_clips_at_black_and_white():
    _, st, luts, _, _ = setup()
    x = np.stack([np.zeros((32, 32, 3), np.uint8), np.full((32, 32, 3), 255, np.uint8), np.full((32, 32, 3), 3, np.uint8)])
    lo, hi = CF.patch_boxes(x[0], (2, 2), 16, 5)
    assert lo.max() == 0 and hi.max() == 5 and (hi[0, :2, :2] == 5).all() and hi[0].sum() == 5 * 12
    lo, hi = CF.patch_boxes(x[1], (2, 2), 16, 5)
    assert hi.min() == 255 and lo.min() == 250
    lo, hi = CF.patch_boxes(x[2], (1, 1), 8, 255)
    assert lo.min() == 0 and hi.max() == 255 and (lo <= hi).all()
    pre = oracle_pre(st, normalise(x.astype(np.float64)))
    cls = OB.valexnet_from_stem_bits((pre >= 0).astype(np.uint8), st, setup()[0], luts)[1].argmax(axis=1)
    _, maps = CF.certify_patch_cpu(st, luts, x, cls, (2, 2), 16, 5)
    for i in range(3):
        lo, hi = CF.patch_boxes(x[i], (2, 2), 16, 5)
        want = CF.certify_box_cpu(st, luts, lo, hi, np.full(4, cls[i]))
        got = maps[i].reshape(-1)
        assert np.array_equal(got["stage"], want["stage"]) and np.array_equal(got["unknown_stem"], want["unknown_stem"])
        assert np.abs(got["lb"] - want["lb"]).max() <= tol()


def test_transposed_patches_give_transposed_position_counts():
    _, st, luts, x, cls = setup()
    for (h, w), s in (((2, 5), 3), ((1, 8), 5), ((3, 2), 1)):
        a = CF.certify_patch_cpu(st, luts, x[:1], cls[:1], (h, w), s, 1, enum_bits=0)[1]
        b = CF.certify_patch_cpu(st, luts, x[:1], cls[:1], (w, h), s, 1, enum_bits=0)[1]
        assert a.shape[1:] == b.shape[1:][::-1] == (patch_positions(h, s), patch_positions(w, s))


def test_invalid_arguments_raise():
    _, st, luts, x, cls = setup()
    for kw in (dict(patch=(0, 1)), dict(patch=(1, 9)), dict(patch=(2,)), dict(patch=2), dict(stride=0), dict(stride=33), dict(amp=0),
               dict(amp=256), dict(amp=2.5), dict(enum_bits=13), dict(enum_bits=-1)):
        with pytest.raises(ValueError):
            CF.certify_patch_cpu(st, luts, x[:1], cls[:1], **{"patch": (2, 2), **kw})
    with pytest.raises(ValueError):
        CF.certify_patch_cpu(st, luts, x[:2], cls[:1], (2, 2))
    with pytest.raises(ValueError):
        CF.certify_patch_cpu(st, luts, x[:1].astype(np.float64), cls[:1], (2, 2))
    lo, hi = CF.patch_boxes(x[0], (2, 2), 16, 5)
    with pytest.raises(ValueError):
        CF.certify_box_cpu(st, luts, hi, lo, np.full(4, cls[0]))                         # lo > hi
    with pytest.raises(ValueError):
        CF.certify_box_cpu(st, luts, lo, hi[:3], np.full(4, cls[0]))
    rows, maps = CF.certify_patch_cpu(st, luts, x[:2], [10, -1], (4, 4), 4, 1)           # a class outside 0..9 is a record, not an error
    assert (maps["stage"] == 0).all() and (maps["worst"] == -1).all() and (maps["lb"] == -np.inf).all()
    assert (rows["certified"] == 0).all() and (rows["positions"] == 64).all() and (rows["pos_min"] == 0).all()
    assert np.array_equal(maps["unknown_stem"], sweep((4, 4), 4, 1)[1][:2]["unknown_stem"])      # (images 0 and 1 lead both)


def test_command_flags_line_and_files(tmp_path):
    p = cifar.build_parser()
    a = p.parse_args([])
    assert (a.certify_patch, a.patch_stride, a.patch_amp, a.patch_map, a.patch_rows) == (None, 1, 255, None, None)
    a = p.parse_args(["--certify_patch", "1x1,2x3", "--patch_stride", "3", "--patch_amp", "8", "--patch_map", "m.npz", "--patch_rows", "r.csv"])
    assert cifar.certify_patch_list(a.certify_patch) == [(1, 1), (2, 3)] and (a.patch_stride, a.patch_amp) == (3, 8)
    for bad in ("x", "1x", "0x1", "9x1", "2x2x2", "1x1,,2x2", "3"):
        with pytest.raises(SystemExit):
            cifar.certify_patch_list(bad)
    for argv in (["--certify_patch", "9x9"], ["--certify_patch", "1x1", "--patch_stride", "0"], ["--certify_patch", "1x1", "--patch_amp", "256"],
                 ["--patch_map", "m.npz"], ["--patch_rows", "r.csv"], ["--certify_patch", "1x1", "--certify_enum", "13"]):
        with pytest.raises(SystemExit):
            cifar.main(["--data_dir", "/nonexistent"] + argv)
    cls = setup()[4][list(IMGS)]
    sums = [CF.summarise_patch(patch, stride, amp, *sweep(patch, stride, amp)) for patch, stride, amp in (((4, 4), 4, 1), ((2, 3), 3, 8))]
    median = float(np.median(sums[0]["map"]["unknown_stem"]))             # (of all 192 positions)
    assert CF.patch_line(sums[0]) == ("Patch.. size=4x4 amp=1 stride=4 sampled 2/3 66.67 (positions 172/192 certified: interval 146, "
                                      f"enumeration 26; unknown stem bits median {median:g} max 8)")
    one = CF.summarise_patch((1, 1), 1, 16, *sweep((1, 1), 1, 16, 7))
    assert CF.patch_line(one).startswith("Patch.. size=1x1 amp=16 stride=1 1/1 100.00 (positions 1024/1024 certified: interval 1023, enumeration 1;")
    assert "sampled" not in CF.patch_line(one)
    rows_file, map_file = tmp_path / "r.csv", tmp_path / "m.npz"
    CF.write_patch_rows_csv(str(rows_file), sums, cls.tolist())
    CF.write_patch_map_npz(str(map_file), sums)
    assert sorted(os.listdir(tmp_path)) == ["m.npz", "r.csv"]                             # (no temporary file left)
    with open(rows_file, newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 6 and list(got[0]) == CF.PATCH_ROWS_HEADER
    assert [g["size"] for g in got] == ["4x4"] * 3 + ["2x3"] * 3 and [int(g["class"]) for g in got] == cls.tolist() * 2
    assert [int(g["patch_certified"]) for g in got[:3]] == [0, 1, 1] and [int(g["certified"]) for g in got[:3]] == [44, 64, 64]
    assert np.array_equal(np.array([float(g["lb_min"]) for g in got[3:]]), sums[1]["rows"]["lb_min"])
    with np.load(map_file) as z:
        assert sorted(z.files) == sorted(f"{k}_{s}" for k in ("lb", "stage", "worst", "unknown_stem") for s in ("4x4", "2x3"))
        assert z["lb_4x4"].shape == (3, 8, 8) and z["stage_2x3"].shape == (3, 11, 10)
        assert np.array_equal(z["lb_2x3"], sums[1]["map"]["lb"]) and np.array_equal(z["stage_4x4"], sums[0]["map"]["stage"])
    with pytest.raises(ValueError):
        CF.write_patch_rows_csv(str(tmp_path / "bad.csv"), sums, cls.tolist()[:-1])
    assert sorted(os.listdir(tmp_path)) == ["m.npz", "r.csv"]


def test_command_runs_the_sweep_after_the_lines_it_printed_before(tmp_path, capsys, monkeypatch):
    """``cifar.main`` end to end with the device stubbed: the model is a shell, ``evaluate`` prints its line, and
    ``certify.certify_patch_u8`` answers from the twin, batch by batch.  What runs for real: the flags' way into the calls,
    ``certify_patch_batches`` over three batches (dataset order, the records' views), the lines and their order, the files."""
    import torch

    from scale_imagenet_amd import evaluate as EV
    from scale_imagenet_amd import ttnet
    spec, st, luts, x, cls = setup()
    n = 5
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([cls[:n, None].astype(np.uint8), x[:n].transpose(0, 3, 1, 2).reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
    calls = []

    class Shell:
        def __init__(self, args):
            self.spec = spec

        def load_state_dict(self, sd, strict=True):
            return self

        def to(self, device):
            return self

        def eval(self):
            return self

        def reserve(self, n):
            return self

    def fake_patch_u8(model, xb, tb, patch, stride, amp, enum_bits, min_margin, lane=0):
        calls.append((xb.shape[0], tuple(patch), stride, amp, enum_bits, min_margin))
        rows, maps = CF.certify_patch_cpu(st, luts, xb.numpy(), tb.numpy(), patch, stride, amp, enum_bits, min_margin)
        return CF.PatchResult(torch.from_numpy(rows.view(np.float64).reshape(-1, 4).copy()),
                              torch.from_numpy(maps.view(np.float64).reshape(maps.shape + (2,)).copy()), patch, stride, amp)

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)
    monkeypatch.setattr(ttnet, "TT_FHE_XSMALL_vAlexnet", Shell)
    monkeypatch.setattr(EV, "evaluate", lambda model, batches, device, **kw: print("Acc.. 100.0 100.0"))
    real_batches = cifar.device_batches
    monkeypatch.setattr(cifar, "device_batches", lambda images, targets, bs, device: real_batches(images, targets, bs, torch.device("cpu")))
    monkeypatch.setattr(CF, "certify_patch_u8", fake_patch_u8)
    rows_file, map_file = tmp_path / "r.csv", tmp_path / "m.npz"
    argv = ["--data_dir", str(tmp_path), "--synthetic-ckpt", "--eval_batch_size", "2", "--certify_patch", "4x4,2x5", "--patch_stride", "4",
            "--patch_amp", "1", "--certify_enum", "9", "--certify_min_margin", "2e-6", "--patch_rows", str(rows_file), "--patch_map", str(map_file)]
    assert cifar.main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    whole = [CF.summarise_patch(p, 4, 1, *CF.certify_patch_cpu(st, luts, x[:n], cls[:n], p, 4, 1, 9, 2e-6)) for p in ((4, 4), (2, 5))]
    assert out == ["Acc.. 100.0 100.0"] + [CF.patch_line(s) for s in whole]                # after the unchanged line, one per size
    assert out[1].startswith("Patch.. size=4x4 amp=1 stride=4 sampled ") and out[2].startswith("Patch.. size=2x5 amp=1 stride=4 sampled ")
    assert calls == [(b, p, 4, 1, 9, 2e-6) for b in (2, 2, 1) for p in ((4, 4), (2, 5))]    # three batches, both sizes on each
    with np.load(map_file) as z:
        assert z["lb_4x4"].shape == (n, 8, 8) and z["lb_2x5"].shape == (n, 8, 7)
        for s, key in zip(whole, ("4x4", "2x5")):                                         # dataset order across the batches
            assert np.array_equal(z[f"lb_{key}"], s["map"]["lb"]) and np.array_equal(z[f"stage_{key}"], s["map"]["stage"])
            assert np.array_equal(z[f"unknown_stem_{key}"], s["map"]["unknown_stem"])
    with open(rows_file, newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 2 * n and [int(g["index"]) for g in got] == list(range(n)) * 2 and [int(g["class"]) for g in got] == cls[:n].tolist() * 2
    assert [int(g["certified"]) for g in got[:n]] == whole[0]["rows"]["certified"].tolist()
    assert sorted(os.listdir(tmp_path)) == ["cifar-10-batches-bin", "m.npz", "r.csv"]
    assert cifar.main(argv[:5]) == 0                                                     # no --certify_patch: the one line, as before
    assert capsys.readouterr().out.splitlines() == ["Acc.. 100.0 100.0"] and len(calls) == 6


def test_the_library_states_the_sweeps_launch_cut():
    """``ttnet_launch_partition("patch.sweep", ..)`` answers without a GPU: positions, launches and their sizes, as
    csrc/partition.h cuts them and ttnet_certify_patch_u8 launches them."""
    from scale_imagenet_amd import _lib
    from scale_imagenet_amd.build import build_lib
    build_lib(verbose=False)
    q = lambda *a: list(_lib.launch_partition("patch.sweep", *a))  # noqa: E731
    py, px, launches, first, last, cap = q(3, 1, 1, 1)
    assert (py, px, cap) == (32, 32, 2048) and (launches, first, last) == (2, 2048, 1024)   # the GPU suite's 3 x 1,024: the cut runs
    assert q(1, 1, 1, 1)[2:5] == [1, 1024, 1024] and q(2, 1, 1, 1)[2:5] == [1, 2048, 2048] and q(256, 1, 1, 1)[2:5] == [128, 2048, 2048]
    assert q(3, 8, 8, 8)[:5] == [4, 4, 1, 48, 48] and q(5, 2, 5, 3)[:2] == [11, 10] and q(1, 8, 1, 32)[:2] == [1, 1]
    for n, h, w, s in ((1, 1, 1, 1), (7, 2, 3, 3), (257, 1, 1, 1), (100, 3, 3, 1)):
        py, px, launches, first, last, cap = q(n, h, w, s)
        assert (py, px) == (patch_positions(h, s), patch_positions(w, s))
        assert (launches - 1) * cap + last == n * py * px and 1 <= last <= cap and first == min(cap, n * py * px)
    for bad in ((0, 1, 1, 1), (1, 9, 1, 1), (1, 1, 9, 1), (1, 1, 1, 33), (1, 0, 1, 1), (1, 1, 1, 0)):
        with pytest.raises(_lib.TTNetError):
            q(*bad)
