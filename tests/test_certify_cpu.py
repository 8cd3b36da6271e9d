"""CPU: the numpy float64 twin of the robustness certificate (scale_imagenet_amd/certify.py: certify_cpu) on the synthetic
vAlexnet checkpoint and 64 synthetic images -- soundness by sampling, the selector-word lookup against brute force, stage 2
against brute force, eps = 0, monotonicity in eps, the stem's edge cases, and the command's flags and rows file.

The oracle here is float64: the stem restated with torch double ops (``oracle_pre``, the first lines of
``OF.forward_valexnet``) and ``OB.valexnet_from_stem_bits`` behind it.  The counts pinned in test 3 are facts about the
synthetic checkpoint (the prototype's table), not about a trained network."""
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

N = 64
EPS_ALL = (0.0, 0.001, 0.01, 0.03, 0.1, 1.0, 2.0)
TOTENSOR = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@lru_cache(maxsize=None)
def setup():
    spec, st = spec_and_state("valexnet")
    luts, near = OB.build_all_luts(st, spec)
    assert not any(v.any() for v in near.values()), "a near-tie table entry: the tables would not be a float64 fact"
    x = np.ascontiguousarray(synth.synth_images_u8(N, hw=(32, 32)).transpose(0, 2, 3, 1))
    x.setflags(write=False)
    return spec, st, luts, x


def oracle_forward(v: np.ndarray, mean=cifar.CIFAR_MEAN, std=cifar.CIFAR_STD):
    """(pre, stem bits, feature bits, float64 logits) of real-valued byte levels."""
    spec, st, luts, _ = setup()
    pre = oracle_pre(st, normalise(v, mean, std))
    bits = (pre >= 0).astype(np.uint8)
    y, logits = OB.valexnet_from_stem_bits(bits, st, spec, luts)
    return pre, bits, y, logits


@lru_cache(maxsize=None)
def nominal():
    _, _, _, x = setup()
    _, _, _, logits = oracle_forward(x.astype(np.float64))
    cls = logits.argmax(axis=1)
    srt = np.sort(logits, axis=1)
    return cls, srt[:, -1] - srt[:, -2]


@lru_cache(maxsize=None)
def certified(eps: float, enum_bits: int = 10):
    _, st, luts, x = setup()
    return CF.certify_cpu(st, luts, x, nominal()[0], eps, enum_bits=enum_bits, return_planes=True)


def perturbed(x: np.ndarray, eps: float, k: int, seed: int) -> np.ndarray:
    """[n, k, 32, 32, 3] real byte levels inside the clipped box: all +eps, all -eps, random sign corners, and (the second
    half) points drawn uniformly inside."""
    rng = np.random.default_rng(seed)
    b = x.astype(np.float64)[:, None]
    d = np.empty((x.shape[0], k) + x.shape[1:])
    d[:, 0], d[:, 1] = eps, -eps
    d[:, 2:k // 2] = rng.choice([-eps, eps], size=d[:, 2:k // 2].shape)
    d[:, k // 2:] = rng.uniform(-eps, eps, size=d[:, k // 2:].shape)
    return np.clip(b + d, 0.0, 255.0)


# ---- 1. soundness by sampling ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.01, 0.03, 0.1])
def test_sampled_perturbations_stay_inside(eps):
    _, _, _, x = setup()
    cls, _ = nominal()
    rows, planes = certified(eps)
    v = perturbed(x, eps, 32, seed=int(eps * 1000))
    _, bits, y, logits = oracle_forward(v.reshape((-1,) + x.shape[1:]))
    bits, y, logits = bits.reshape(N, 32, 64, 10, 10), y.reshape(N, 32, 256, 11, 11), logits.reshape(N, 32, 10)
    assert (planes["stem_lo"] <= planes["stem_hi"]).all() and (planes["feat_lo"] <= planes["feat_hi"]).all()
    assert (bits >= planes["stem_lo"][:, None]).all() and (bits <= planes["stem_hi"][:, None]).all()
    assert (y >= planes["feat_lo"][:, None]).all() and (y <= planes["feat_hi"][:, None]).all()
    own = np.take_along_axis(logits, cls[:, None, None].repeat(32, 1), axis=2)[..., 0]
    others = logits.copy()
    np.put_along_axis(others, cls[:, None, None].repeat(32, 1), -np.inf, axis=2)
    margin = own - others.max(axis=2)                                   # [N, 32]
    cert = rows["stage"] > 0
    print(f"eps {eps}: {int(cert.sum())} certified ({int((rows['stage'] == 2).sum())} by enumeration); smallest sampled margin "
          f"minus lb over them {float((margin - rows['lb'][:, None])[cert].min()) if cert.any() else float('nan'):.3e}")
    assert cert.any()
    assert (logits.argmax(axis=2) == cls[:, None])[cert].all()
    assert (margin[cert] >= rows["lb"][cert, None] - 1e-9).all()
    assert (margin >= rows["lb_interval"][:, None] - 1e-9).all()        # the interval bound holds for every image, certified or not


# ---- 2. the selector-word lookup ------------------------------------------------------------------------------------------

def test_selector_words_equal_brute_force():
    spec, _, luts, _ = setup()
    rng = np.random.default_rng(5)
    for b in spec.block_tts():
        n = b.fan_in_bits
        words = CF.table_words(luts[b.name], n)                          # [G, cout, W]
        for _ in range(300):
            g, o = int(rng.integers(b.groups)), int(rng.integers(b.cout_g))
            state = rng.choice(3, size=n, p=[0.35, 0.35, 0.3])           # 0, 1, unknown
            lo, hi = (state == 1).astype(np.uint8), (state >= 1).astype(np.uint8)
            free = np.flatnonzero(state == 2)
            seen = set()
            for a in range(1 << free.size):
                w = lo.copy()
                w[free] = (a >> np.arange(free.size)) & 1
                canon = sum(int(w[p]) << (n - 1 - p) for p in range(n))  # inputs MSB first (OB.window_index)
                seen.add(int(luts[b.name][g, canon, o]))
            ylo, yhi = CF.lookup3(words[g, o], lo, hi)
            assert (int(ylo), int(yhi)) == (int(0 not in seen), int(1 in seen)), (b.name, g, o, state)


# ---- 3. stage 2 against brute force -----------------------------------------------------------------------------------------

def test_enumeration_equals_brute_force():
    spec, st, luts, _ = setup()
    cls, _ = nominal()
    rows, planes = certified(0.03)
    stage1 = CF.certify_cpu(st, luts, setup()[3], cls, 0.03, enum_bits=0)
    A, c0 = CF.effective_head(st)
    words = [CF.table_words(luts[b.name], b.fan_in_bits) for b in spec.block_tts()]
    k = rows["unknown_stem"]
    small = np.flatnonzero((k >= 1) & (k <= 10))
    ran = np.flatnonzero((stage1["stage"] == 0) & (k >= 1) & (k <= 10))
    by_enum = 0
    for i in small:
        lo, hi = planes["stem_lo"][i], planes["stem_hi"][i]
        free = np.argwhere(lo != hi)
        a = np.arange(1 << len(free))
        comp = np.broadcast_to(lo, (a.size, 64, 10, 10)).copy()
        comp[:, free[:, 0], free[:, 1], free[:, 2]] = (a[:, None] >> np.arange(len(free))[None, :]) & 1
        _, logits = OB.valexnet_from_stem_bits(comp, st, spec, luts)
        diff = logits[:, cls[i]][:, None] - logits
        diff[:, cls[i]] = np.inf
        brute = diff.min()
        got, _ = CF.enumerate_cpu(A, c0, words, lo, hi, planes["feat_lo"][i], int(cls[i]))
        assert abs(got - brute) <= 1e-9, (i, got, brute)
        assert got >= rows["lb_interval"][i] - 1e-9
        by_enum += got > 1e-6
        if i in ran:
            assert rows["lb"][i] == got and rows["stage"][i] == (2 if got > 1e-6 else 0)
        else:
            assert rows["lb"][i] == rows["lb_interval"][i] and rows["stage"][i] == stage1["stage"][i]
    only2 = int(((rows["stage"] == 2) & (stage1["stage"] == 0)).sum())
    print(f"eps 0.03: {small.size} images with 1 <= k <= 10, {int(by_enum)} of them certified by enumeration, {ran.size} took stage 2, "
          f"{only2} certified by stage 2 alone, {int((stage1['stage'] == 1).sum())} by stage 1")
    assert ran.size >= 20 and only2 >= 1
    # the prototype's table for this checkpoint and these images
    assert small.size == 62 and int(by_enum) == 40 and int((stage1["stage"] == 1).sum()) == 32


# ---- 4. eps = 0 ------------------------------------------------------------------------------------------------------------

def test_eps_zero_is_the_nominal_margin():
    rows, planes = certified(0.0)
    _, margin = nominal()
    assert (rows["unknown_stem"] == 0).all() and (rows["unknown_feat"] == 0).all()
    assert (planes["stem_lo"] == planes["stem_hi"]).all()
    assert np.abs(rows["lb"] - margin).max() <= 1e-9 and (rows["lb"] == rows["lb_interval"]).all()
    assert (rows["stage"] == (margin > 1e-6)).all()


# ---- 5. monotonicity ---------------------------------------------------------------------------------------------------------

def test_planes_nest_and_the_bound_falls_with_eps():
    prev = None
    for eps in EPS_ALL:
        rows, planes = certified(eps)
        if prev is not None:
            prows, pp = prev
            for kind in ("stem", "feat"):
                assert (planes[kind + "_lo"] <= pp[kind + "_lo"]).all() and (planes[kind + "_hi"] >= pp[kind + "_hi"]).all(), (eps, kind)
            assert (rows["lb_interval"] <= prows["lb_interval"] + 1e-9).all(), eps
            assert (rows["unknown_stem"] >= prows["unknown_stem"]).all()
        prev = (rows, planes)
    table = {eps: int((certified(eps)[0]["stage"] == 1).sum()) for eps in EPS_ALL}
    print("certified by the interval bound:", table)
    assert table[0.001] == 63 and table[0.01] == 48 and table[0.1] == 5 and table[1.0] == 0 and table[2.0] == 0


# ---- 6. the stem's edge cases --------------------------------------------------------------------------------------------------

def _stem_case(st, x, eps, mean, std, seed):
    """Containment of sampled corners, and tightness of the upper bound at a few outputs: the corner that maximises one
    convolution output (minimises it under a negative BatchNorm scale) reaches that output's bound; the pooled upper bound is
    the largest of the nine."""
    lo, hi = CF.stem_bounds_cpu(st, x, eps, mean, std)
    sl = CF.stem_slack(st, mean, std)[None, :, None, None]
    assert (lo <= hi).all()
    v = perturbed(x, eps, 8, seed)[:, :4]                                # the four corners
    pre = oracle_pre(st, normalise(v.reshape((-1,) + x.shape[1:]), mean, std)).reshape(x.shape[0], 4, 64, 10, 10)
    assert (pre >= (lo - sl)[:, None]).all() and (pre <= (hi + sl)[:, None]).all()
    lo_bit, hi_bit = CF.stem_planes_cpu(st, x, eps, mean, std)
    bits = pre >= 0
    assert (bits >= lo_bit[:, None]).all() and (bits <= hi_bit[:, None]).all()
    w = st["features.0.weight"].astype(np.float64)
    scale, _ = CF.fold_bn(st, "features.2")
    rng = np.random.default_rng(seed)
    b = x.astype(np.float64)
    for _ in range(6):
        i, ch, py, px = int(rng.integers(x.shape[0])), int(rng.integers(64)), int(rng.integers(10)), int(rng.integers(10))
        best = -np.inf
        for dy in range(3):
            for dx in range(3):
                up = np.ones((32, 32, 3))                                # +1: the byte goes up
                for kh in range(3):
                    for kw in range(3):
                        r, q = 3 * py + dy + kh - 1, 3 * px + dx + kw - 1
                        if 0 <= r < 32 and 0 <= q < 32:
                            up[r, q] = np.where(w[ch, :, kh, kw] * scale[ch] >= 0, 1.0, -1.0)
                corner = np.clip(b[i] + eps * up, 0.0, 255.0)[None]
                best = max(best, oracle_pre(st, normalise(corner, mean, std))[0, ch, py, px])
        assert abs(best - hi[i, ch, py, px]) <= 1e-9 * max(1.0, abs(best)), (i, ch, py, px, best, hi[i, ch, py, px])
    return lo, hi


def test_stem_negative_batchnorm_scale_swaps_the_bounds():
    _, st, _, x = setup()
    st2 = dict(st)
    wt = st["features.2.weight"].copy()
    wt[::3] = -wt[::3]
    st2["features.2.weight"] = wt
    assert (CF.fold_bn(st2, "features.2")[0] < 0).sum() >= 20
    _stem_case(st2, x[:8], 1.0, cifar.CIFAR_MEAN, cifar.CIFAR_STD, 11)
    _stem_case(st2, x[:8], 0.03, cifar.CIFAR_MEAN, cifar.CIFAR_STD, 12)


def test_stem_clipping_at_black_and_white():
    _, st, _, _ = setup()
    x = np.stack([np.zeros((32, 32, 3), np.uint8), np.full((32, 32, 3), 255, np.uint8)])
    lo, hi = _stem_case(st, x, 2.0, cifar.CIFAR_MEAN, cifar.CIFAR_STD, 13)
    # an all-0 image cannot go down and an all-255 image cannot go up: one side of the box is the image itself
    pre = oracle_pre(st, normalise(x.astype(np.float64)))
    free_lo, free_hi = CF.stem_bounds_cpu(st, np.full((1, 32, 32, 3), 128, np.uint8), 2.0)
    assert (hi - lo).max() < (free_hi - free_lo).max()
    assert (pre >= lo - 1e-9).all() and (pre <= hi + 1e-9).all()


def test_stem_totensor_normalisation():
    _, st, _, x = setup()
    _stem_case(st, x[:8], 1.0, *TOTENSOR, 14)
    a = CF.stem_slack(st, *TOTENSOR)
    b = CF.stem_slack(st)
    assert a.shape == (64,) and (a > 0).all() and (a < b).all()        # X = 1 against ~2.5 under the CIFAR constants


# ---- 7. flags, rows file, return code ---------------------------------------------------------------------------------------------

def test_parser_flags_and_defaults():
    p = cifar.build_parser()
    a = p.parse_args([])
    assert (a.certify, a.certify_enum, a.certify_min_margin, a.certify_rows) == (None, 10, 1e-6, None)
    a = p.parse_args(["--certify", "0.03,1", "--certify_enum", "4", "--certify_min_margin", "2e-5", "--certify_rows", "r.csv"])
    assert cifar.certify_eps_list(a.certify) == [0.03, 1.0] and a.certify_enum == 4 and a.certify_min_margin == 2e-5
    assert a.certify_rows == "r.csv"
    for bad in ("x", "1,-2", "nan", "1,,2"):
        with pytest.raises(SystemExit):
            cifar.certify_eps_list(bad)
    for argv in (["--certify", "1", "--certify_enum", "13"], ["--certify_rows", "r.csv"], ["--certify", "-1"]):
        with pytest.raises(SystemExit):
            cifar.main(["--data_dir", "/nonexistent"] + argv)


def test_rows_csv_and_verified_line(tmp_path):
    cls, _ = nominal()
    sums = [CF.summarise(eps, certified(eps)[0]) for eps in (0.03, 1.0)]
    path = tmp_path / "r.csv"
    CF.write_rows_csv(str(path), sums, cls.tolist())
    assert os.listdir(tmp_path) == ["r.csv"]                             # (no temporary file left)
    with open(path, newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 2 * N and list(got[0]) == ["eps"] + CF.ROWS_HEADER
    for s, part in zip(sums, (got[:N], got[N:])):
        r = s["rows"]
        assert [float(g["eps"]) for g in part] == [s["eps"]] * N and [int(g["index"]) for g in part] == list(range(N))
        assert [int(g["class"]) for g in part] == cls.tolist()
        assert np.array_equal(np.array([float(g["lb"]) for g in part]), r["lb"])
        assert np.array_equal(np.array([float(g["lb_interval"]) for g in part]), r["lb_interval"])
        for col in ("stage", "worst", "unknown_stem", "unknown_feat"):
            assert [int(g[col]) for g in part] == r[col].tolist()
        assert [int(g["certified"]) for g in part] == (r["stage"] > 0).astype(int).tolist()
    assert CF.verified_line(sums[0]) == ("Verified.. eps=0.03 41/64 64.06 (interval 32, enumeration 9; unknown stem bits median 6 "
                                         f"max {int(sums[0]['rows']['unknown_stem'].max())})")
    with pytest.raises(ValueError):
        CF.write_rows_csv(str(tmp_path / "bad.csv"), sums, cls.tolist()[:-1])
    assert os.listdir(tmp_path) == ["r.csv"]


def test_main_without_certify_returns_as_before(tmp_path, capsys):
    """No --certify: the command goes the way it went (here: to its refusal of a missing dataset directory), and a dataset
    that is there is read before any device is asked for."""
    with pytest.raises(SystemExit) as e:
        cifar.main(["--data_dir", str(tmp_path / "nowhere"), "--synthetic-ckpt"])
    assert "is not a directory" in str(e.value)
    assert capsys.readouterr().out == ""


def test_argument_checks_of_the_twin():
    _, st, luts, x = setup()
    cls, _ = nominal()
    for kw in (dict(eps=-1.0), dict(eps=float("nan")), dict(eps=1.0, enum_bits=13)):
        with pytest.raises(ValueError):
            CF.certify_cpu(st, luts, x[:2], cls[:2], **kw)
    rows = CF.certify_cpu(st, luts, x[:3], [int(cls[0]), 10, -1], 0.01)
    assert rows["stage"].tolist()[1:] == [0, 0] and (rows["lb"][1:] == -np.inf).all() and rows["worst"].tolist()[1:] == [-1, -1]
    assert rows["stage"][0] == certified(0.01)[0]["stage"][0]
