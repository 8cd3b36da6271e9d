"""CPU: the numpy float64 twin of the patch search (``attack.attack_patch_cpu``) through the float64 oracle forward: its
predictions against the box certificate's twin and against the oracle's margins, the 1 x 1 corner counts, the search against
random corners at the same budget, its consistency with the certified sweep, the edges, and the command with the device stubbed
by the twin."""
import os

import numpy as np
import pytest

import _attack_patch_util as U
from _attack_util import NORMS, images_np, nominal, oracle_forward, setup
from scale_imagenet_amd import _lib
from scale_imagenet_amd import attack as AT
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar
from scale_imagenet_amd.valexnet_block import field_span

SETTINGS = [((4, 4), 4, 255), ((2, 3), 3, 8), ((4, 4), 4, 1), ((8, 8), 8, 255)]
CORNERS = {"cifar": (537, 97, 0), "std16": (515, 9, 0)}      # positions of images 0, 1, 7 that one of a pixel's eight corner colours flips (float64 oracle)


def clean_fills(res):
    n, py, px = res.map.shape
    h, w = res.patch
    x = np.asarray(res.x0)
    org = CF.patch_origins(res.patch, res.stride)
    return np.stack([[x[i, a:a + h, b:b + w].reshape(-1) for a, b in org] for i in range(n)])


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("patch,stride,amp", SETTINGS)
def test_m_pred_is_the_box_certificate_of_the_witness(norm, patch, stride, amp):
    """``m_pred`` of every kept fill is ``lb_interval`` of ``certify_box_cpu`` on the degenerate box of the pasted image (two
    summation orders of one real number: within ``1e-9 sum|A|``), and where no recomputed cell lies within the slack it is the
    oracle's float64 margin within the logit tolerance."""
    _, st, luts = setup()
    mean, std = NORMS[norm]
    res = U.twin(norm, patch, stride, amp)
    w = U.witnesses(res)
    P = res.map.shape[1] * res.map.shape[2]
    cls = np.repeat(U.classes3(norm), P)
    rows = CF.certify_box_cpu(st, luts, w, w, cls, 0, 0.0, mean, std)
    flat = res.map.reshape(-1)
    err = np.abs(flat["m_pred"] - rows["lb_interval"]).max()
    print(f"{norm} {patch} stride {stride} amp {amp}: max |m_pred - lb_interval| = {err:.3g} (tolerance {U.tolerance():.3g})")
    assert err <= U.tolerance() and np.array_equal(flat["worst"], rows["worst"])
    exact = flat["unknown"] == 0
    assert exact.any()
    assert np.abs(flat["m_pred"][exact] - U.oracle_margins(norm, w[exact], cls[exact])).max() <= U.LOGIT_TOL
    assert res.near.mean() <= 0.01                              # the inputs of the device comparison stay under its cap


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("patch,stride,amp", SETTINGS + [((1, 1), 1, 255)])
def test_fills_lie_in_the_box_and_leave_the_rest_alone(norm, patch, stride, amp):
    res = U.twin(norm, patch, stride, amp, 1 if patch == (1, 1) else 2)
    h, w = patch
    clean = clean_fills(res).astype(np.int64)
    fills = res.fills_numpy()
    assert np.abs(fills[:, :, :3 * h * w].astype(np.int64) - clean).max() <= amp and not fills[:, :, 3 * h * w:].any()
    changed = (fills[:, :, :3 * h * w] != clean).any(axis=2).reshape(res.map.shape)
    assert np.array_equal(changed, res.map["round"] > 0)        # a kept candidate is no copy of the clean bytes
    wit, x = U.witnesses(res), U.images3()
    P = len(CF.patch_origins(patch, stride))
    for t, (y0, x0) in enumerate(np.tile(CF.patch_origins(patch, stride), (3, 1))):
        inside = np.zeros((32, 32), bool)
        inside[y0:y0 + h, x0:x0 + w] = True
        assert np.array_equal(wit[t][~inside], x[t // P][~inside])
    assert np.array_equal(res.witness(1, P - 1), wit[2 * P - 1])
    # every status occurs over the three images where the patch can do anything at all
    if amp == 255:
        assert (res.map["status"] == AT.FALSIFIED).any() and (res.map["status"] == AT.OPEN).any()


@pytest.mark.parametrize("norm", sorted(NORMS))
def test_one_pixel_corner_counts(norm):
    """1 x 1 / 255 / stride 1 / one round: the eight corners of the pixel are the search.  The positions with ``m_pred < 0`` are
    the float64 oracle's counts; a position may differ only where the witness's oracle margin lies within the logit tolerance of
    zero, at most 1 % of an image's positions."""
    res = U.twin(norm, (1, 1), 1, 255, 1)
    flat = res.map.reshape(3, -1)
    got = (flat["m_pred"] < 0).sum(axis=1)
    print(f"{norm}: positions with m_pred < 0: {got.tolist()}, the oracle's {list(CORNERS[norm])}")
    margins = U.oracle_margins(norm, U.witnesses(res), np.repeat(U.classes3(norm), 1024)).reshape(3, -1)
    ties = (np.abs(margins) <= U.LOGIT_TOL).sum(axis=1)
    assert (np.abs(got - np.array(CORNERS[norm])) <= np.minimum(ties, 10)).all()
    assert np.array_equal(res.rows["falsified"], ((margins.astype(np.float32) < 0) & (flat["round"] > 0) & (flat["m_pred"] < 1e-5)).sum(axis=1))   # the forward judged each of them
    # a position that touches only row or column 31 lies in no field: nothing moves, nothing is searched
    edge = np.array([field_span(int(y), 1)[1] == 0 or field_span(int(x), 1)[1] == 0 for y, x in CF.patch_origins((1, 1), 1)])
    assert edge.sum() == 63 and not flat["round"][:, edge].any() and not flat["status"][:, edge].any()
    assert (flat["m_pred"][:, edge] == flat["m_pred"][:, edge][:, :1]).all()      # the clean value


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("patch,stride,amp", [((4, 4), 4, 255), ((2, 3), 3, 8)])
def test_search_finds_no_fewer_than_random_corners(norm, patch, stride, amp):
    """Per image, the positions the oracle forward confirms number no fewer than those that ``8 * rounds`` random per-byte corners
    per position falsify (fixed seed, the same budget of forwards)."""
    rounds = 2
    res = U.twin(norm, patch, stride, amp, rounds)
    rnd = U.random_corner_falsified(norm, patch, stride, amp, 8 * rounds).sum(axis=1)
    print(f"{norm} {patch} stride {stride} amp {amp}: search {res.rows['falsified'].tolist()}, random corners {rnd.tolist()}")
    assert (res.rows["falsified"] >= rnd).all()


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("patch,stride,amp", [((2, 3), 3, 8), ((4, 4), 4, 1)])
def test_no_certified_position_is_falsified(norm, patch, stride, amp):
    _, st, luts = setup()
    mean, std = NORMS[norm]
    res = U.twin(norm, patch, stride, amp, 2, U.LOGIT_TOL)
    rows, maps = CF.certify_patch_cpu(st, luts, U.images3(), U.classes3(norm), patch, stride, amp, 10, U.LOGIT_TOL, mean, std)
    cs = CF.summarise_patch(patch, stride, amp, rows, maps)
    as_ = AT.summarise_patch(res, 2)
    b = AT.patch_robust_bounds(cs, as_)
    assert b["positions_certified"] == int((maps["stage"] > 0).sum()) and b["positions_falsified"] == int(res.rows["falsified"].sum())
    assert b["certified"] + b["falsified"] + b["open"] == 3
    line = AT.patch_robust_line(cs, as_)
    assert line.startswith(f"PatchRobust.. size={patch[0]}x{patch[1]} amp={amp} stride={stride} certified {b['certified']}/3 <= robust <= {3 - b['falsified']}/3 (")
    # a doctored pair: a position both certified and falsified, then an image both
    bad = dict(as_, map=as_["map"].copy())
    pos = np.argwhere(maps["stage"] > 0)[0]
    bad["map"]["status"][tuple(pos)] = AT.FALSIFIED
    with pytest.raises(ValueError, match="both certified and falsified"):
        AT.patch_robust_bounds(cs, bad)
    full = np.flatnonzero(rows["certified"] == rows["positions"])
    if full.size:
        bad = dict(as_, rows=as_["rows"].copy())
        bad["rows"]["status"][full[0]] = AT.FALSIFIED
        with pytest.raises(ValueError, match="both patch-certified and falsified"):
            AT.patch_robust_bounds(cs, bad)
    with pytest.raises(ValueError):
        AT.patch_robust_bounds(dict(cs, map=maps[:2]), as_)


def test_classes_outside_the_range_and_images_wrong_at_x0():
    _, st, luts = setup()
    x = U.images3()
    c = U.classes3("cifar")
    wrong = int((c[0] + 1) % 10)
    res = AT.attack_patch_cpu(st, luts, x, [wrong, -1, 10], (2, 3), 3, 8, 2, 0.0, forward=oracle_forward("cifar"))
    flat = res.map.reshape(3, -1)
    assert res.rows["status"].tolist() == [AT.WRONG, AT.OPEN, AT.OPEN] and not res.rows["falsified"].any()
    assert not flat["round"].any() and not flat["status"].any() and np.isnan(flat["margin"]).all()
    assert (flat["m_pred"][0] < 0).all() and (flat["m_pred"][0] == flat["m_pred"][0][0]).all()      # the clean value, already lost
    assert np.isneginf(flat["m_pred"][1:]).all() and (flat["worst"][1:] == -1).all() and not flat["unknown"][1:].any()
    assert np.array_equal(res.fills_numpy()[:, :, :18], clean_fills(res))


def test_confirm_modes_and_arguments():
    full, best, none = (U.twin("cifar", (4, 4), 4, 255, 2, 0.0, mode) for mode in AT.CONFIRM)
    for k in AT.PATCH_RECORD.names:
        assert np.array_equal(full.map[k], best.map[k]) and np.array_equal(full.map[k], none.map[k])
    f, b = full.map.reshape(3, -1), best.map.reshape(3, -1)
    judged = ~np.isnan(b["margin"])
    assert judged.sum(axis=1).max() == 1 and np.array_equal(b["margin"][judged], f["margin"][judged])
    assert ((b["status"] == AT.FALSIFIED) <= (f["status"] == AT.FALSIFIED)).all()
    assert np.array_equal(best.rows["status"], full.rows["status"])                     # enough for the accuracy bracket
    assert (none.map["status"] != AT.FALSIFIED).all() and (none.map["status"] == AT.PREDICTED).sum() == ((f["round"] > 0) & (f["m_pred"] < 1e-5)).sum()
    _, st, luts = setup()
    for kw in (dict(rounds=0), dict(rounds=5), dict(rounds=True), dict(patch=(9, 1)), dict(stride=0), dict(amp=256), dict(confirm="some"),
               dict(min_margin=float("nan"))):
        args = dict(patch=(1, 1), stride=1, amp=255, rounds=2, min_margin=0.0, confirm="all")
        args.update(kw)
        with pytest.raises(ValueError):
            AT.attack_patch_cpu(st, luts, U.images3(), U.classes3("cifar"), forward=oracle_forward("cifar"), **args)


def test_gains_and_scores_are_those_of_the_propose_twin():
    """The restricted sums of the patch twin are ``gains_cpu`` / ``scores_cpu`` with ``unknown`` := the movable bits, byte for byte."""
    _, st, luts = setup()
    tw = AT._PatchTwin(st, luts, *NORMS["cifar"])
    bits, feat, _, cls = nominal("cifar")
    i, rng = 0, np.random.default_rng(5)
    unknown = np.zeros((1, 64, 10, 10), bool)
    unknown[0, :, 2:5, 6:9] = rng.integers(0, 2, (64, 3, 3)).astype(bool)
    j = int((cls[i] + 3) % 10)
    g = AT.gains_cpu(tw.A, tw.words, bits[i:i + 1], feat[i:i + 1], unknown, [cls[i]], [j])
    pi, ch, y, x = np.nonzero(unknown)
    mine = tw.gains(np.pad(bits[i:i + 1].astype(np.int64), ((0, 0), (0, 0), (1, 1), (1, 1))), pi, ch, y, x, int(cls[i]), np.full(pi.size, j))
    assert np.array_equal(mine.view(np.int64), g[pi, ch, y, x].view(np.int64)) and np.abs(mine).max() > 0
    sc = AT.scores_cpu(g, bits[i:i + 1], unknown, tw.scale, tw.Wsum)                     # [1, 2, 32, 32, 3]
    sgn = np.where(bits[i:i + 1] == 0, 1.0, -1.0) * np.where(tw.scale >= 0, 1.0, -1.0)[None, :, None, None]
    wt1 = np.where(unknown, -g * sgn, 0.0)
    wt = np.stack([np.where(g < 0, wt1, 0.0), wt1])
    for y0, x0, h, w in ((6, 17, 8, 8), (8, 20, 2, 3), (5, 26, 4, 4)):
        got = tw.scores(wt, np.array([y0]), np.array([x0]), h, w)
        assert np.array_equal(got[:, 0].view(np.int64), sc[0, :, y0:y0 + h, x0:x0 + w].view(np.int64))


def test_paste_and_hash():
    x = images_np(2)
    fills = np.arange(2 * 4 * 192, dtype=np.int64).reshape(2, 4, 192).astype(np.uint8)
    out = AT.paste_cpu(x, (8, 8), 8, np.tile(fills, (1, 4, 1)), [0, 17, -1, 32, 5])
    assert not out[2].any() and not out[3].any() and np.array_equal(out[0][:8, :8].reshape(-1), fills[0, 0])
    assert np.array_equal(out[1][:8, 8:16].reshape(-1), fills[1, 1]) and np.array_equal(out[1][8:], x[1][8:])
    assert np.array_equal(out[4][8:16, 8:16].reshape(-1), fills[0, 1]) and np.array_equal(out[4][:8], x[0][:8])
    h = AT.hash_corner(np.arange(1024)[:, None], 1, 14, np.arange(192)[None, :])
    assert 0.45 < h.mean() < 0.55 and not np.array_equal(h, AT.hash_corner(np.arange(1024)[:, None], 2, 14, np.arange(192)[None, :]))


def test_the_library_states_the_searchs_launch_cut():
    """``ttnet_launch_partition("patch.attack", ..)`` answers without a GPU and cuts as the sweep does."""
    for a in ((3, 1, 1, 1), (1, 1, 1, 1), (256, 8, 8, 8), (2, 1, 1, 1), (257, 4, 4, 4)):
        assert _lib.launch_partition("patch.attack", *a) == _lib.launch_partition("patch.sweep", *a)
    assert _lib.launch_partition("patch.attack", 3, 1, 1, 1) == (32, 32, 2, 2048, 1024, 2048)
    with pytest.raises(_lib.TTNetError, match="patch.attack"):
        _lib.launch_partition("patch.attack", 1, 9, 1, 1)


def test_command_prints_the_bracket_after_each_patch_line(tmp_path, capsys, monkeypatch):
    """``cifar.main`` end to end with the device stubbed: ``certify_patch_u8`` and ``attack_patch_u8`` answer from the twins, batch by
    batch.  The earlier lines are unchanged, one ``PatchRobust..`` line follows each ``Patch..`` line, the witness file holds the
    falsified positions, and without the flag the output is what it was."""
    import torch

    from scale_imagenet_amd import evaluate as EV
    from scale_imagenet_amd import ttnet
    spec, st, luts = setup()
    x, cls = np.ascontiguousarray(images_np()[:5]), np.asarray(nominal("cifar")[3])[:5]
    n = 5
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([cls[:, None].astype(np.uint8), x.transpose(0, 3, 1, 2).reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
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
        rows, maps = CF.certify_patch_cpu(st, luts, xb.numpy(), tb.numpy(), patch, stride, amp, enum_bits, min_margin)
        return CF.PatchResult(torch.from_numpy(rows.view(np.float64).reshape(-1, 4).copy()),
                              torch.from_numpy(maps.view(np.float64).reshape(maps.shape + (2,)).copy()), patch, stride, amp)

    def fake_attack_patch_u8(model, xb, tb, patch, stride, amp, rounds, min_margin, confirm, confirm_slack, lane=0):
        calls.append((xb.shape[0], tuple(patch), stride, amp, rounds, min_margin, confirm))
        return AT.attack_patch_cpu(st, luts, xb.numpy(), tb.numpy(), patch, stride, amp, rounds, min_margin, forward=oracle_forward("cifar"),
                                   confirm=confirm, confirm_slack=confirm_slack)

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda dev: None)
    monkeypatch.setattr(ttnet, "TT_FHE_XSMALL_vAlexnet", Shell)
    monkeypatch.setattr(EV, "evaluate", lambda model, batches, device, **kw: print("Acc.. 100.0 100.0"))
    real_batches = cifar.device_batches
    monkeypatch.setattr(cifar, "device_batches", lambda images, targets, bs, device: real_batches(images, targets, bs, torch.device("cpu")))
    monkeypatch.setattr(CF, "certify_patch_u8", fake_patch_u8)
    monkeypatch.setattr(AT, "attack_patch_u8", fake_attack_patch_u8)
    wit = tmp_path / "w.npz"
    base = ["--data_dir", str(tmp_path), "--synthetic-ckpt", "--eval_batch_size", "2", "--certify_patch", "4x4,2x5", "--patch_stride", "4",
            "--patch_amp", "255", "--certify_min_margin", "1e-5"]
    assert cifar.main(base) == 0
    before = capsys.readouterr().out
    assert cifar.main(base + ["--attack_patch", "--attack_patch_rounds", "1", "--attack_patch_confirm", "best", "--patch_witnesses", str(wit)]) == 0
    out = capsys.readouterr().out.splitlines()
    assert [l for l in out if not l.startswith("PatchRobust..")] == before.splitlines() and len(before.splitlines()) == 3
    assert [l[:12] for l in out] == ["Acc.. 100.0 ", "Patch.. size", "PatchRobust.", "Patch.. size", "PatchRobust."]
    assert calls == [(b, p, 4, 255, 1, 1e-5, "best") for b in (2, 2, 1) for p in ((4, 4), (2, 5))]
    whole = [AT.attack_patch_cpu(st, luts, x, cls, p, 4, 255, 1, 1e-5, forward=oracle_forward("cifar"), confirm="best") for p in ((4, 4), (2, 5))]
    cert = [CF.summarise_patch(p, 4, 255, *CF.certify_patch_cpu(st, luts, x, cls, p, 4, 255, 10, 1e-5)) for p in ((4, 4), (2, 5))]
    assert [out[2], out[4]] == [AT.patch_robust_line(c, AT.summarise_patch(w, 1)) for c, w in zip(cert, whole)]
    assert out[2].startswith("PatchRobust.. size=4x4 amp=255 stride=4 certified 0/5 <= robust <= ") and "by search" in out[2]
    with np.load(wit) as z:
        assert sorted(z.files) == sorted(f"{k}_{s}" for k in ("tasks", "fills", "margin", "m_pred", "geometry") for s in ("4x4", "2x5"))
        for w, key in zip(whole, ("4x4", "2x5")):                                         # dataset order across the batches
            tasks = np.flatnonzero(w.map.reshape(-1)["status"] == AT.FALSIFIED)
            assert tasks.size and np.array_equal(z[f"tasks_{key}"], tasks) and (z[f"margin_{key}"] < -1e-5).all()
            h, ww, stride, amp, py, px = z[f"geometry_{key}"]
            fills = np.zeros((n, py * px, AT.FILL_BYTES), np.uint8)
            fills.reshape(-1, AT.FILL_BYTES)[tasks, :3 * h * ww] = z[f"fills_{key}"]
            images = AT.paste_cpu(x, (h, ww), stride, fills, tasks)                       # the witnesses reproduce their margins
            assert np.array_equal(U.oracle_margins("cifar", images, cls[tasks // (py * px)]).astype(np.float32), z[f"margin_{key}"])
    assert sorted(os.listdir(tmp_path)) == ["cifar-10-batches-bin", "w.npz"]
    for argv in (["--attack_patch"], ["--certify_patch", "1x1", "--patch_witnesses", "w.npz"],
                 ["--certify_patch", "1x1", "--attack_patch", "--attack_patch_rounds", "5"],
                 ["--certify_patch", "1x1", "--attack_patch", "--attack_patch_rounds", "0"]):
        with pytest.raises(SystemExit):
            cifar.main(["--data_dir", "/nonexistent"] + argv)
