"""CPU: the numpy float64 twin of the witness search (scale_imagenet_amd/attack.py) on the synthetic vAlexnet checkpoint and
the 64 synthetic images of test_certify_cpu.py -- flip gains against brute force, the candidates' invariants, the select
step, a bracket with something on both sides, the search against random box corners, and the command's flags and files.

The oracle is float64: ``oracle_pre`` and ``OB.valexnet_from_stem_bits`` (tests/_attack_util.py: ``oracle_forward``).  The
counts printed are facts about the synthetic checkpoint, not about a trained network."""
import csv
import os

import numpy as np
import pytest

import _attack_util as U
from oracle import ttnet_bits as OB
from scale_imagenet_amd import attack as AT
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar

N = U.N


def proposal(norm: str, eps: int, n: int = N):
    """(unknown, gains, scores, candidates) of round 1 for the first n images."""
    _, st, luts = U.setup()
    bits, y, logits, cls = U.nominal(norm)
    lo, hi = CF.stem_planes_cpu(st, U.images_np()[:n], float(eps), *U.NORMS[norm])
    A = AT.head_cpu(st)
    worst = U.runner_up(logits, cls)
    g = AT.gains_cpu(A, AT._words(luts), bits[:n], y[:n], lo != hi, cls[:n], worst[:n])
    s = AT.scores_cpu(g, bits[:n], lo != hi, CF.fold_bn(st, "features.2")[0], AT.wsum_cpu(st))
    return lo != hi, g, s, AT.candidates_cpu(s, U.images_np()[:n], U.images_np()[:n], eps)


# ---- 1. gains against brute force ----------------------------------------------------------------------------------------

def test_gains_equal_brute_force():
    spec, st, luts = U.setup()
    bits, y, logits, cls = U.nominal("cifar")
    n = 4
    lo, hi = CF.stem_planes_cpu(st, U.images_np()[:n], 1.0)
    unknown = lo != hi
    A = AT.head_cpu(st)
    worst = U.runner_up(logits, cls)
    g, changed = AT.gains_cpu(A, AT._words(luts), bits[:n], y[:n], unknown, cls[:n], worst[:n], return_changed=True)
    reach = AT.reached_features()
    assert (g[~unknown] == 0).all()
    total = 0
    for i in range(n):
        D = A[cls[i]] - A[worst[i]]
        where = np.argwhere(unknown[i])
        flipped = np.broadcast_to(bits[i], (len(where), 64, 10, 10)).copy()
        flipped[np.arange(len(where)), where[:, 0], where[:, 1], where[:, 2]] ^= 1
        y2, _ = OB.valexnet_from_stem_bits(flipped, st, spec, luts)
        delta = y2.reshape(len(where), -1).astype(np.float64) - y[i].reshape(-1).astype(np.float64)[None]
        brute = delta @ D
        got = g[i][unknown[i]]
        assert np.abs(got - brute).max() <= 1e-12 * np.abs(D).sum(), (i, np.abs(got - brute).max())
        for q, (ch, py, px) in enumerate(where):
            mine = set(reach[:, ch, py, px][changed[i, :, ch, py, px]].tolist())
            assert -1 not in mine and mine == set(np.flatnonzero(delta[q]).tolist()), (i, ch, py, px)
        total += len(where)
    print(f"{total} unknown stem bits of {n} images at eps 1; {int((g < 0).sum())} with a negative gain")
    assert total >= 100 and (g < 0).any() and (g > 0).any()


def test_wsum_is_the_pooled_stem_response():
    """Raising one input byte by one normalised unit raises the nine convolution outputs of a pooled cell by Wsum in total."""
    _, st, _ = U.setup()
    W = AT.wsum_cpu(st)
    w = st["features.0.weight"].astype(np.float64)
    rng = np.random.default_rng(2)
    for _ in range(20):
        ch, k, r, q = int(rng.integers(64)), int(rng.integers(3)), int(rng.integers(5)), int(rng.integers(5))
        want = sum(w[ch, k, r - dy, q - dx] for dy in range(3) for dx in range(3) if 0 <= r - dy < 3 and 0 <= q - dx < 3)
        assert abs(W[ch, k, r, q] - want) <= 1e-15 * np.abs(w[ch, k]).sum()


# ---- 2. candidates -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [1, 2, 5])
def test_candidates_stay_in_the_box_and_keep_unselected_bytes(eps):
    x0 = U.images_np().copy()
    x0[0, :8] = 0                                                        # bytes forced to the ends of the range
    x0[0, 8:16] = 255
    _, st, luts = U.setup()
    fwd = U.oracle_forward("cifar")
    bits, y, logits = fwd(x0[:8])
    cls = logits.argmax(axis=1)
    lo_bit, hi_bit = CF.stem_planes_cpu(st, x0[:8], float(eps))
    unknown = lo_bit != hi_bit
    g = AT.gains_cpu(AT.head_cpu(st), AT._words(luts), bits, y, unknown, cls, U.runner_up(logits, cls))
    s = AT.scores_cpu(g, bits, unknown, CF.fold_bn(st, "features.2")[0], AT.wsum_cpu(st))
    rng = np.random.default_rng(eps)
    lo, hi = U.box(x0[:8], eps)
    xcur = rng.integers(lo.astype(np.int64), hi.astype(np.int64) + 1).astype(np.uint8)      # any image inside the box
    cand = AT.candidates_cpu(s, x0[:8], xcur, eps)
    assert cand.shape == (8, 8, 32, 32, 3) and cand.dtype == np.uint8
    assert (cand >= lo[:, None]).all() and (cand <= hi[:, None]).all()
    M = np.abs(s).reshape(8, 2, -1).max(axis=2)
    for m in range(2):
        for t, tau in enumerate(AT.TAUS):
            c = cand[:, 4 * m + t]
            sel = (s[:, m] != 0) & (np.abs(s[:, m]) > tau * M[:, m, None, None, None])
            assert np.array_equal(c[~sel], xcur[~sel])
            assert np.array_equal(c[sel], np.where(s[:, m] > 0, hi, lo)[sel])
            if t:
                assert sel.sum() <= prev.sum() and not (sel & ~prev).any()           # a higher threshold selects a subset
            prev = sel
    assert np.array_equal(cand[:, :, 31], np.broadcast_to(xcur[:, None, 31], cand[:, :, 31].shape))
    assert np.array_equal(cand[:, :, :, 31], np.broadcast_to(xcur[:, None, :, 31], cand[:, :, :, 31].shape))
    assert (s[:, :, 31] == 0).all() and (s[:, :, :, 31] == 0).all()
    assert (cand != xcur[:, None]).any()
    # mode 0 pushes a subset of what mode 1 pushes
    assert ((s[:, 0] != 0) <= (s[:, 1] != 0)).all()


def test_candidates_without_anything_to_move():
    unknown, g, s, cand = proposal("cifar", 1, 4)
    x0 = U.images_np()[:4]
    xcur = np.minimum(254, x0) + 1
    same = AT.candidates_cpu(s, x0, x0, 0)                              # eps 0 and x_cur = x0: nothing changes
    assert np.array_equal(same, np.broadcast_to(x0[:, None], same.shape))
    none = AT.candidates_cpu(np.zeros_like(s), x0, xcur, 2)             # an image without unknown bits has no score
    assert np.array_equal(none, np.broadcast_to(xcur[:, None], none.shape))
    off = AT.candidates_cpu(s, x0, xcur, 2, active=[0, 1, 0, 1])         # an image that left the active set
    assert np.array_equal(off[0], np.broadcast_to(xcur[0], off[0].shape)) and (off[1] != xcur[1]).any()
    # gains of an image whose class or runner-up is no class are zero
    _, st, luts = U.setup()
    bits, y, logits, cls = U.nominal("cifar")
    g2 = AT.gains_cpu(AT.head_cpu(st), AT._words(luts), bits[:4], y[:4], unknown, [int(cls[0]), 10, -1, int(cls[3])],
                      [int(U.runner_up(logits, cls)[0]), 1, 1, -1])
    assert np.array_equal(g2[0], g[0]) and (g2[1:] == 0).all()


def test_threshold_ties_are_rare_in_the_twin():
    """What the GPU comparison may exclude: bytes whose score lies within 2^-40 M of a decision threshold."""
    for norm, eps in (("cifar", 1), ("cifar", 2), ("std16", 1)):
        _, _, s, _ = proposal(norm, eps)
        band = U.threshold_band(s)
        print(f"{norm} eps {eps}: {int(band.sum())} of {band.size} scores within 2^-40 M of a threshold")
        assert band.sum() <= 1e-4 * band.size


# ---- 3. select ---------------------------------------------------------------------------------------------------------------

def _select_case(n_cand):
    rng = np.random.default_rng(40 + n_cand)
    n = 6
    x0 = U.images_np()[:n]
    lo, hi = U.box(x0, 2)
    cand = rng.integers(lo[:, None].astype(np.int64), hi[:, None].astype(np.int64) + 1, size=(n, n_cand, 32, 32, 3)).astype(np.uint8)
    logits = rng.normal(size=(n, n_cand, 10)).astype(np.float32)
    classes = np.array([3, 0, 9, 10, 5, 2])
    return x0, cand, logits, classes


@pytest.mark.parametrize("n_cand", [1, 8])
def test_select_picks_the_smallest_margin(n_cand):
    x0, cand, logits, classes = _select_case(n_cand)
    n = len(classes)
    rows, xcur, worst, active = AT.new_state(n)
    first = np.zeros((n, 1, 10), np.float32)
    first[np.arange(n), 0, np.minimum(classes, 9)] = 1.0                 # round 0: every image right by a margin of 1
    first[4, 0] = [0, 0, 0, 0, 0, 0, 0, 2, 0, 0]                         # .. but image 4, wrong at x0
    AT.select_cpu(x0[:, None], first, 1, classes, 0.25, x0, xcur, rows, worst, active, 0)
    assert np.array_equal(xcur, x0) and rows["tried"].tolist() == [1, 1, 1, 0, 1, 1]
    assert rows["status"].tolist() == [0, 0, 0, 0, AT.WRONG, 0] and active.tolist() == [1, 1, 1, 0, 0, 1]
    assert rows["margin0"].tolist() == [1, 1, 1, -np.inf, -2, 1] and rows["best"].tolist() == [1, 1, 1, -np.inf, -2, 1]
    assert rows["worst"].tolist() == [0, 1, 0, -1, 7, 0] and worst.tolist() == [0, 1, 0, -1, 7, 0]
    logits[0, :, 3] = 5.0                                                # image 0: no candidate below the best so far
    logits[1] = 0.0                                                      # image 1: all margins tie at 0 < 1: the lowest index, runner-up 1
    logits[2, 0] = np.nan                                                # image 2: candidate 0 is skipped
    if n_cand == 8:
        logits[2, 1:, 9] = 0.0
        logits[2, 1:, :9] = -1.0
        logits[2, 5, 4] = logits[2, 6, 4] = 0.5                          # candidates 5 and 6 tie at -0.5: 5 wins
    logits[5, :, 2] = 3.0
    logits[5, n_cand - 1, 6] = 3.1                                       # image 5: the last candidate, margin -0.1: below best, not falsified
    before = rows.copy()
    AT.select_cpu(cand, logits.reshape(-1, 10), n_cand, classes, 0.25, x0, xcur, rows, worst, active, 2)
    assert rows[3] == before[3] and rows[4] == before[4]                 # inactive images are left alone
    assert np.array_equal(xcur[3], x0[3]) and np.array_equal(xcur[4], x0[4])
    assert rows["tried"].tolist() == [1 + n_cand, 1 + n_cand, 1 + n_cand, 0, 1, 1 + n_cand]
    assert rows[0]["best"] == 1 and rows[0]["round"] == 0 and np.array_equal(xcur[0], x0[0]) and active[0] == 1
    assert rows[1]["best"] == 0 and rows[1]["worst"] == 1 and rows[1]["round"] == 2 and np.array_equal(xcur[1], cand[1, 0])
    assert rows[1]["status"] == 0 and active[1] == 1                     # 0 is not below -0.25
    if n_cand == 8:
        assert rows[2]["best"] == -0.5 and rows[2]["worst"] == 4 and np.array_equal(xcur[2], cand[2, 5])
        assert rows[2]["status"] == AT.FALSIFIED and active[2] == 0
    else:
        assert rows[2]["best"] == 1 and rows[2]["round"] == 0 and np.array_equal(xcur[2], x0[2])   # its only candidate was NaN
    assert abs(rows[5]["best"] + 0.1) < 1e-6 and rows[5]["worst"] == 6 and rows[5]["status"] == 0 and active[5] == 1
    assert np.array_equal(xcur[5], cand[5, n_cand - 1])
    for i in (1, 5):                                                     # changed and linf, recounted from the bytes
        d = np.abs(xcur[i].astype(int) - x0[i].astype(int))
        assert rows[i]["changed"] == (d != 0).sum() and rows[i]["linf"] == d.max() and rows[i]["linf"] <= 2
    assert AT.RECORD.itemsize == 32


# ---- 4. / 5. the bracket, and the search against guessing ------------------------------------------------------------------------

def test_bracket_has_both_sides():
    for eps in (1, 2):
        cert = U.twin_certify("std16", float(eps))
        rows, wit = U.twin_attack("std16", eps)
        a, f, o = AT.robust_bounds(cert, rows)                           # raises on an image in both
        by_round = AT.summarise(eps, rows, 3)["by_round"]
        print(f"std 16, eps {eps}: certified {a}, falsified {f} (by round {by_round}), open {o}")
        assert a + f + o == N
        lo, hi = U.box(U.images_np(), eps)
        assert (wit >= lo).all() and (wit <= hi).all()
        logits = U.oracle_forward("std16")(wit)[2]
        assert np.array_equal(logits.argmax(axis=1) != U.nominal("std16")[3], rows["status"] > 0)    # min_margin 0: falsified = another class
        d = np.abs(wit.astype(int) - U.images_np().astype(int)).reshape(N, -1)
        assert np.array_equal(rows["changed"], (d != 0).sum(axis=1)) and np.array_equal(rows["linf"], d.max(axis=1))
        if eps == 1:
            assert a >= 8 and f >= 8
    print("line:", AT.robust_line(2.0, U.twin_certify("std16", 2.0), U.twin_attack("std16", 2)[0]))


@pytest.mark.parametrize("norm", ["cifar", "std16"])
def test_search_is_not_worse_than_random_corners(norm):
    rows, _ = U.twin_attack(norm, 1)
    cls = U.nominal(norm)[3]
    fwd = U.oracle_forward(norm)
    lo, hi = U.box(U.images_np(), 1)
    rng = np.random.default_rng(7)
    hit = np.zeros(N, dtype=bool)
    for _ in range(48):
        corner = np.where(rng.integers(0, 2, size=lo.shape) == 1, hi, lo)
        hit |= fwd(corner)[2].argmax(axis=1) != cls
    print(f"{norm}, eps 1: the search falsifies {int((rows['status'] > 0).sum())} of {N}, 48 random corners per image {int(hit.sum())}")
    assert (rows["status"] > 0).sum() >= hit.sum()


def test_rounds_zero_and_eps_zero():
    _, st, luts = U.setup()
    cls = U.nominal("cifar")[3].copy()
    cls[5] = (cls[5] + 1) % 10                                          # one image is wrong at x0
    cls[6] = 11
    for kw in (dict(eps=1.0, rounds=0), dict(eps=0.5, rounds=2)):
        rows, wit = AT.attack_cpu(st, luts, U.images_np()[:8], cls[:8], min_margin=0.0, forward=U.oracle_forward("cifar"), **kw)
        assert np.array_equal(wit, U.images_np()[:8])
        assert rows["status"].tolist() == [0, 0, 0, 0, 0, AT.WRONG, 0, 0] and (rows["changed"] == 0).all()
        assert rows[6]["worst"] == -1 and rows[6]["best"] == -np.inf and rows[6]["tried"] == 0
    for bad in (dict(eps=-1.0), dict(eps=float("nan")), dict(eps=65.0), dict(eps=1.0, rounds=9)):
        with pytest.raises(ValueError):
            AT.attack_cpu(st, luts, U.images_np()[:2], cls[:2], forward=U.oracle_forward("cifar"), **bad)


# ---- 6. flags, the line, the rows file -------------------------------------------------------------------------------------------

def test_parser_flags_and_refusals():
    p = cifar.build_parser()
    a = p.parse_args([])
    assert (a.attack, a.attack_rounds, a.attack_rows, a.attack_witnesses) == (False, 3, None, None)
    a = p.parse_args(["--certify", "1,2.5", "--attack", "--attack_rounds", "2", "--attack_rows", "a.csv", "--attack_witnesses", "w.npz"])
    assert a.attack and a.attack_rounds == 2 and a.attack_rows == "a.csv" and a.attack_witnesses == "w.npz"
    for argv in (["--attack"], ["--certify", "1", "--attack_rows", "a.csv"], ["--certify", "1", "--attack", "--attack_rounds", "9"],
                 ["--certify", "1", "--attack", "--attack_rounds", "-1"], ["--certify", "70", "--attack"]):
        with pytest.raises(SystemExit):
            cifar.main(["--data_dir", "/nonexistent"] + argv)
    assert AT.eps_levels(2.5) == 2 and AT.eps_levels(0.99) == 0 and AT.eps_levels(64.0) == 64


def test_robust_line_and_rows_csv(tmp_path):
    cert = U.twin_certify("std16", 1.0)
    rows, _ = U.twin_attack("std16", 1)
    a, f, o = AT.robust_bounds(cert, rows)
    w = int((rows["status"] == AT.WRONG).sum())
    assert AT.robust_line(1.0, cert, rows) == (f"Robust.. eps=1 certified {a}/{N} <= robust <= {N - f}/{N} (falsified {f}: wrong at x0 {w}, "
                                               f"by search {f - w}; open {o})")
    clash = rows.copy()
    clash["status"][np.flatnonzero(cert["stage"] > 0)[0]] = AT.FALSIFIED
    with pytest.raises(ValueError, match="both certified and falsified"):
        AT.robust_bounds(cert, clash)
    with pytest.raises(ValueError):
        AT.robust_bounds(cert[:-1], rows)
    cls = U.nominal("std16")[3].tolist()
    sums = [AT.summarise(1.0, rows, 3), AT.summarise(2.0, U.twin_attack("std16", 2)[0], 3)]
    assert sums[0]["falsified"] == f and sums[0]["wrong"] == w and sum(sums[0]["by_round"]) == f - w
    path = tmp_path / "a.csv"
    AT.write_rows_csv(str(path), sums, cls)
    assert os.listdir(tmp_path) == ["a.csv"]
    with open(path, newline="") as fh:
        got = list(csv.DictReader(fh))
    assert len(got) == 2 * N and list(got[0]) == ["eps"] + AT.ROWS_HEADER
    for s, part in zip(sums, (got[:N], got[N:])):
        r = s["rows"]
        assert [float(g["eps"]) for g in part] == [s["eps"]] * N and [int(g["class"]) for g in part] == cls
        assert np.array_equal(np.array([float(g["best"]) for g in part], dtype=np.float32), r["best"])
        assert np.array_equal(np.array([float(g["margin0"]) for g in part], dtype=np.float32), r["margin0"])
        for col in ("status", "worst", "round", "changed", "linf", "tried"):
            assert [int(g[col]) for g in part] == r[col].tolist()
        assert [int(g["falsified"]) for g in part] == (r["status"] > 0).astype(int).tolist()
    with pytest.raises(ValueError):
        AT.write_rows_csv(str(tmp_path / "bad.csv"), sums, cls[:-1])
    assert os.listdir(tmp_path) == ["a.csv"]
