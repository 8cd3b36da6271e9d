"""GPU: the witness search (csrc/attack.hip; scale_imagenet_amd/attack.py) against its numpy float64 twin fed the device's
own bits, against the device's own forward and the float64 oracle, and through the C ABI and the command.

Synthetic weights, the 64 synthetic images, the classes the float64 oracle gives them; CIFAR mean / std and the wide
std (16, 16, 16) at which integer eps leaves certified, falsified and open images at once."""
import csv
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attack_util as U
from _util import ROOT, args_for, scaled_tol, spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import attack as AT
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar, synth, ttnet

pytestmark = pytest.mark.gpu

N = U.N


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def new_model(dev, norm="cifar", state=None, max_batch=257, lanes=2):
    st = state if state is not None else spec_and_state("valexnet")[1]
    m = ttnet.TT_FHE_XSMALL_vAlexnet(args_for("valexnet"))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(max_batch).set_lanes(lanes)
    if norm != "cifar":
        m.set_input_norm(*U.NORMS[norm])
    return m


@pytest.fixture(scope="module")
def models(dev):
    return {norm: new_model(dev, norm) for norm in U.NORMS}


def images(dev, n=N):
    return torch.tensor(U.images_np(n)).to(dev)


def classes(dev, norm, n=N):
    return torch.from_numpy(U.nominal(norm, n)[3][:n]).to(dev, torch.int32)


def tables(model):
    return {b.name: model.get_table(b.name) for b in model.spec.block_tts()}


def device_forward(model, dev, lane=0, chunk=AT.FORWARD_ROWS):
    """``forward`` for ``attack_cpu`` through the device: logits of ``forward_u8`` and the lane's stage buffers, in forwards of
    at most ``chunk`` images as ``attack_u8`` issues them (beyond that lin1's split-K count, and with it the last bits of a
    logit, depends on the batch size)."""
    def forward(x_u8):
        x_u8 = np.ascontiguousarray(x_u8)
        bits, feats, logits = [], [], []
        with torch.no_grad():
            for a in range(0, x_u8.shape[0], chunk):
                part = torch.tensor(x_u8[a:a + chunk]).to(dev)      # (a copy: the cached images are read-only)
                logits.append(model.forward_u8(part, lane=lane).cpu().numpy())
                bits.append(OB.unpack_rows(model.read_stage("features.4", part.shape[0]), 10))
                feats.append(OB.unpack_rows(model.read_stage("features.5", part.shape[0]), 11))
        return np.concatenate(bits), np.concatenate(feats), np.concatenate(logits)
    return forward


def stem_planes(model, x, cls, eps):
    """The certificate's stem planes: the int64 tensor [2, n, 64, 10] that propose takes, and the unknown bits as a bool array."""
    p = model.certify_u8(x, cls, float(eps), 0, return_planes=True).planes
    t = torch.stack([p["stem_lo"], p["stem_hi"]]).contiguous()
    lo, hi = (OB.unpack_rows(v.cpu().numpy().view(np.uint64), 10) for v in (p["stem_lo"], p["stem_hi"]))
    return t, lo != hi, (p["stem_lo"], p["stem_hi"])


def state(dev, n):
    return (torch.empty((n, 8), dtype=torch.int32, device=dev), torch.empty((n, 32, 32, 3), dtype=torch.uint8, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))


def same_rows(a, b):
    return all(np.array_equal(a[f], b[f], equal_nan=True) for f in AT.RECORD.names)


# ---- 1. propose equals the twin ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm,eps", [("cifar", 1), ("cifar", 2), ("std16", 1)])
def test_propose_equals_the_twin(models, dev, norm, eps):
    model = models[norm]
    _, st = spec_and_state("valexnet")
    x, cls = images(dev), classes(dev, norm)
    fwd = device_forward(model, dev)
    planes, unknown, _ = stem_planes(model, x, cls, eps)
    A, words = AT.head_cpu(st), AT._words(tables(model))
    scale, Wsum = CF.fold_bn(st, "features.2")[0], AT.wsum_cpu(st)
    rows, xcur, worst, active = state(dev, N)
    bits, feats, logits = fwd(U.images_np())                            # the lane now holds the forward of x0
    AT.select_u8(model, x, torch.from_numpy(logits).to(dev), N, 1, cls, 0.0, x, xcur, rows, worst, active, 0)
    excluded = 0
    for rnd in (1, 2):
        cand, gains = AT.propose_u8(model, x, xcur, cls, worst, planes, eps, active, 0, return_gains=True)
        want_g = AT.gains_cpu(A, words, bits, feats, unknown, cls.cpu().numpy(), worst.cpu().numpy())
        want_g[active.cpu().numpy() == 0] = 0.0
        got_g = gains.cpu().numpy()
        assert got_g.tobytes() == want_g.tobytes(), (rnd, int((got_g != want_g).sum()))
        scores = AT.scores_cpu(want_g, bits, unknown, scale, Wsum)
        want_c = AT.candidates_cpu(scores, U.images_np(), xcur.cpu().numpy(), eps, active.cpu().numpy())
        got_c = cand.cpu().numpy()
        band = U.threshold_band(scores)                                 # bytes whose twin score is within 2^-40 M of a threshold
        near = np.concatenate([np.repeat(band[:, m:m + 1], 4, axis=1) for m in range(2)], axis=1)
        assert band.sum() <= 1e-4 * band.size
        assert np.array_equal(got_c[~near], want_c[~near]), (rnd, int((got_c != want_c).sum()))
        excluded += int(near.sum())
        if rnd == 1 or norm == "std16":                                 # (at CIFAR std round 1 falsifies all but one image at most)
            assert (want_g != 0).any() and (want_c != xcur.cpu().numpy()[:, None]).any()
        if rnd == 1:                                                    # a second round from images that are no longer x0
            _, _, cl = fwd(got_c.reshape(-1, 32, 32, 3))
            AT.select_u8(model, cand, torch.from_numpy(cl).to(dev), N, 8, cls, 0.0, x, xcur, rows, worst, active, 1)
            bits, feats, _ = fwd(xcur.cpu().numpy())
            assert (xcur != x).any()
    print(f"{norm} eps {eps}: gains byte-identical in two rounds; {excluded} candidate bytes excluded as threshold ties; "
          f"{int(unknown.sum())} unknown stem bits, {int((active == 0).sum())} images falsified after round 1")


def test_propose_gains_at_hand_placed_unknown_bits(models, dev):
    """Unknown bits placed on the corners, the edges and one interior cell of channels 0, 7, 8 and 63 -- where a wrong border
    or conv3 group boundary in the reach of a stem bit shows -- and nowhere else."""
    model = models["cifar"]
    _, st = spec_and_state("valexnet")
    n = 3
    x = images(dev, n)
    bits, feats, logits = device_forward(model, dev)(U.images_np(n))    # lane 0 now holds the forward of x
    cls = logits.argmax(axis=1)
    worst = U.runner_up(logits, cls)
    unknown = np.zeros((n, 64, 10, 10), dtype=bool)
    for ch in (0, 7, 8, 63):
        for y, xx in [(0, 0), (0, 9), (9, 0), (9, 9), (0, 5), (9, 5), (5, 0), (5, 9), (5, 5)]:
            unknown[:, ch, y, xx] = True
    # lo, hi: the forward's own bits, the marked ones 0 in lo and 1 in hi (unknown = where the planes differ)
    planes = torch.from_numpy(np.stack([OB.pack_rows(bits & ~unknown), OB.pack_rows(bits | unknown)]).view(np.int64)).to(dev)
    as_i32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)     # noqa: E731
    _, gains = AT.propose_u8(model, x, x.clone(), as_i32(cls), as_i32(worst), planes, 1, as_i32(np.ones(n)), 0, return_gains=True)
    got = gains.cpu().numpy()
    want = AT.gains_cpu(AT.head_cpu(st), AT._words(tables(model)), bits, feats, unknown, cls, worst)
    assert got.shape == (n, 64, 10, 10) and got.tobytes() == want.tobytes(), int((got != want).sum())
    assert (got[~unknown] == 0).all() and (got[unknown] != 0).any()


# ---- 2. select equals the twin -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cand", [1, 8])
def test_select_equals_the_twin(models, dev, n_cand):
    model = models["cifar"]
    rng = np.random.default_rng(70 + n_cand)
    n = 9
    x0 = U.images_np()[:n]
    lo, hi = U.box(x0, 2)
    cand = rng.integers(lo[:, None].astype(np.int64), hi[:, None].astype(np.int64) + 1, size=(n, n_cand, 32, 32, 3)).astype(np.uint8)
    cls = np.array([3, 0, 9, 10, 5, 2, -1, 7, 7], dtype=np.int32)
    first = rng.normal(size=(n, 10)).astype(np.float32)
    first[np.arange(n), np.clip(cls, 0, 9)] += 4.0
    first[4] = [0, 0, 0, 0, 0, 0, 0, 2, 0, 0]                            # wrong at x0
    first[7] = 0.0
    first[7, 7], first[7, 2] = 1.0, 1.0                                  # a margin of exactly 0 at x0: not below -min_margin
    nxt = rng.normal(size=(n, n_cand, 10)).astype(np.float32)
    nxt[1] = 0.0                                                         # all margins tie: the lowest index, runner-up 1
    nxt[2, 0, 4] = np.nan                                                # a NaN logit: the candidate is skipped
    nxt[0, :, 3] += 9.0                                                  # nothing below the best so far
    if n_cand == 8:
        nxt[5, :, 2] = 1.0
        nxt[5, 2, 6] = nxt[5, 6, 6] = 1.5                                # candidates 2 and 6 tie at the bottom: 2 wins
        nxt[8, :, :] = np.inf                                            # inf - inf: NaN margins, never below anything
    xd, cd = torch.tensor(x0).to(dev), torch.from_numpy(cls).to(dev)
    rows, xcur, worst, active = state(dev, n)
    trow, tx, tw, ta = AT.new_state(n)
    for rnd, c_np, l_np, k in ((0, x0[:, None], first, 1), (3, cand, nxt.reshape(-1, 10), n_cand), (4, cand, nxt.reshape(-1, 10)[::-1].copy(), n_cand)):
        c_dev = xd if rnd == 0 else torch.from_numpy(c_np).to(dev)
        AT.select_u8(model, c_dev, torch.from_numpy(l_np).to(dev), n, k, cd, 0.25, xd, xcur, rows, worst, active, rnd)
        AT.select_cpu(c_np, l_np, k, cls, 0.25, x0, tx, trow, tw, ta, rnd)
        got = rows.cpu().numpy().view(AT.RECORD).reshape(-1)
        assert same_rows(got, trow), (rnd, got, trow)
        assert np.array_equal(xcur.cpu().numpy(), tx) and np.array_equal(worst.cpu().numpy(), tw) and np.array_equal(active.cpu().numpy(), ta)
        if rnd == 0:
            assert trow["status"].tolist() == [0, 0, 0, 0, AT.WRONG, 0, 0, 0, 0] and ta.tolist() == [1, 1, 1, 0, 0, 1, 0, 1, 1]
            assert trow["margin0"][7] == 0 and trow["best"][7] == 0
    if n_cand == 8:
        assert (trow["status"] == AT.FALSIFIED).any()


# ---- 3. the whole search: every witness is one -----------------------------------------------------------------------------------

@pytest.mark.parametrize("norm,eps", [("cifar", 2), ("std16", 1), ("std16", 2)])
def test_witnesses_are_valid(models, dev, norm, eps):
    model = models[norm]
    _, st = spec_and_state("valexnet")
    x, cls = images(dev), classes(dev, norm)
    with torch.no_grad():
        mm = 2 * scaled_tol(model.forward_u8(x).cpu().numpy())
    res = model.attack_u8(x, cls, eps, rounds=3, min_margin=mm)
    rows, wit = res.numpy(), res.witnesses.cpu().numpy()
    cert = model.certify_u8(x, cls, float(eps), min_margin=mm).numpy()
    a, f, o = AT.robust_bounds(cert, rows)                               # raises on an image in both
    lo, hi = U.box(U.images_np(), eps)
    assert (wit >= lo).all() and (wit <= hi).all()
    fals = rows["status"] > 0
    assert np.array_equal(fals, res.falsified.cpu().numpy())
    c_np = cls.cpu().numpy()
    with torch.no_grad():
        fresh = model.forward_u8(torch.from_numpy(wit[fals]).to(dev), lane=1).cpu().numpy()   # the witnesses alone, on the other lane
    own = fresh[np.arange(fals.sum()), c_np[fals]]
    rest = fresh.copy()
    rest[np.arange(fals.sum()), c_np[fals]] = -np.inf
    assert (own - rest.max(axis=1) < -mm).all()
    oracle = U.oracle_forward(norm)(wit[fals])[2]
    assert (oracle.argmax(axis=1) != c_np[fals]).all()
    d = np.abs(wit.astype(int) - U.images_np().astype(int)).reshape(N, -1)
    assert np.array_equal(rows["changed"], (d != 0).sum(axis=1)) and np.array_equal(rows["linf"], d.max(axis=1)) and (rows["linf"] <= eps).all()
    # the twin through the device's own forward walks the same path
    _, _, planes = stem_planes(model, x, cls, eps)
    lo_b, hi_b = (OB.unpack_rows(v.cpu().numpy().view(np.uint64), 10) for v in planes)
    trows, twit = AT.attack_cpu(st, tables(model), U.images_np(), c_np, eps, 3, mm, forward=device_forward(model, dev), planes=(lo_b, hi_b))
    print(f"{norm} eps {eps}: device certified {a}, falsified {f} (wrong at x0 {int((rows['status'] == 1).sum())}, by round "
          f"{AT.summarise(eps, rows, 3)['by_round']}), open {o}; twin on the device's forward falsified {int((trows['status'] > 0).sum())} "
          f"(by round {AT.summarise(eps, trows, 3)['by_round']}); min_margin {mm:.2e}")
    assert same_rows(rows, trows) and np.array_equal(wit, twit)
    if (norm, eps) == ("std16", 1):
        assert a >= 8 and f >= 8


# ---- 4. shapes and repeatability ---------------------------------------------------------------------------------------------------

def test_shapes_lanes_and_repeatability(models, dev):
    model = models["std16"]
    n = 257
    x, cls = images(dev, n), classes(dev, "std16", n)
    full = model.attack_u8(x, cls, 1)                                    # 2,056 candidates: chunked forwards, two parts
    rows, wit = full.numpy().copy(), full.witnesses.cpu().numpy()
    assert (rows["status"] == AT.FALSIFIED).sum() >= 8 and (rows["status"] == 0).sum() >= 8
    other = model.attack_u8(x, cls, 1, lane=1)
    assert other.numpy().tobytes() == rows.tobytes() and np.array_equal(other.witnesses.cpu().numpy(), wit)
    again = model.attack_u8(x, cls, 1)
    assert again.numpy().tobytes() == rows.tobytes() and np.array_equal(again.witnesses.cpu().numpy(), wit)


def test_sub_batches_equal_the_full_run(models, dev):
    """n = 1, 1 (another image), 3 and the last image alone against the run of 257 images on a plan with max_batch 257: equal
    records and witnesses.  The search forwards at most ``FORWARD_ROWS`` images at a time, up to which lin1's split-K
    count, and so every bit of a logit, does not depend on the batch size (the next test checks the forward for that)."""
    model = models["std16"]
    n = 257
    x, cls = images(dev, n), classes(dev, "std16", n)
    full = model.attack_u8(x, cls, 1)
    rows, wit = full.numpy().copy(), full.witnesses.cpu().numpy()
    for a, b in ((0, 1), (200, 201), (5, 8), (256, 257)):
        part = model.attack_u8(x[a:b], cls[a:b], 1)
        got = part.numpy()
        differ = [f for f in AT.RECORD.names if not np.array_equal(got[f], rows[a:b][f], equal_nan=True)]
        print(f"images {a}..{b - 1}: fields that differ from the run of {n}: {differ or 'none'}")
        assert np.array_equal(part.witnesses.cpu().numpy(), wit[a:b]), (a, b)
        assert got.tobytes() == rows[a:b].tobytes(), (a, b)
    # planes handed in, for the whole batch and for a part of it
    cert = model.certify_u8(x, cls, 1.0, 0, return_planes=True).planes
    given = model.attack_u8(x, cls, 1, planes=(cert["stem_lo"], cert["stem_hi"]))
    assert given.numpy().tobytes() == rows.tobytes() and np.array_equal(given.witnesses.cpu().numpy(), wit)
    given = model.attack_u8(x[250:], cls[250:], 1, planes=(cert["stem_lo"][250:], cert["stem_hi"][250:]))
    assert given.numpy().tobytes() == rows[250:].tobytes()


def test_forward_does_not_depend_on_the_batch_size_up_to_forward_rows(models, dev):
    """What ``attack.FORWARD_ROWS`` rests on: every image of a forward of 256 gets the bytes it gets in a smaller forward."""
    model = models["std16"]
    x = images(dev, AT.FORWARD_ROWS)
    with torch.no_grad():
        ref = model.forward_u8(x).cpu().numpy()
        for a, b in ((0, 1), (0, 3), (0, 8), (0, 24), (0, 129), (200, 201), (5, 8), (100, 256)):
            for _ in range(3):                                           # plain launches, then the replayed graph
                got = model.forward_u8(x[a:b]).cpu().numpy()
            assert got.tobytes() == ref[a:b].tobytes(), (a, b)


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------

def test_edges(models, dev):
    model = models["std16"]
    x = images(dev)
    good = U.nominal("std16")[3]
    cls = good.copy()
    cls[5] = (cls[5] + 1) % 10                                          # wrong at x0
    cls[6], cls[7] = 10, -3                                             # no class
    cd = torch.from_numpy(cls).to(dev)
    for kw in (dict(eps=0.0), dict(eps=0.9), dict(eps=1.0, rounds=0)):
        res = model.attack_u8(x, cd, **kw)
        r = res.numpy()
        assert np.array_equal(res.witnesses.cpu().numpy(), U.images_np()), kw
        assert (r["status"] == AT.WRONG).tolist() == [i == 5 for i in range(N)] and (r["status"] != AT.FALSIFIED).all() and (r["changed"] == 0).all()
        assert r["worst"][6:8].tolist() == [-1, -1] and (r["best"][6:8] == -np.inf).all() and r["tried"][6:8].tolist() == [0, 0]
        assert r["tried"][0] == 1 + 8 * (0 if kw.get("rounds") == 0 else 3)
    r = model.attack_u8(x, cd, 1.0).numpy()
    assert r["status"][5] == AT.WRONG and (r["status"][6:8] == 0).all() and (r["status"] == AT.FALSIFIED).sum() >= 8
    # the plan's input constants are honoured: the std-16 plan against a default plan on the same bytes
    base = models["cifar"].attack_u8(x, torch.from_numpy(good).to(dev), 1.0).numpy()
    wide = model.attack_u8(x, torch.from_numpy(good).to(dev), 1.0).numpy()
    fresh = new_model(dev, "std16").attack_u8(x, torch.from_numpy(good).to(dev), 1.0).numpy()
    assert wide.tobytes() == fresh.tobytes() and (base["status"] > 0).sum() > (wide["status"] > 0).sum()
    with pytest.raises(ValueError):
        model.attack_u8(x, cd, 1.0, rounds=9)
    with pytest.raises(ValueError):
        model.attack_u8(x, cd, 65.0)
    with pytest.raises(RuntimeError, match="vAlexnet"):
        ttnet.TT_vf_19lv3_imgnet_xsmall(args_for("xsmall")).eval().attack_u8(x, cd, 1.0)


def test_reload_rebuilds_wsum_with_the_head(dev):
    _, st = spec_and_state("valexnet")
    x, cls = images(dev), classes(dev, "cifar")
    m = new_model(dev, max_batch=N, lanes=1)
    planes, _, _ = stem_planes(m, x, cls, 1)

    def gains_and_candidates(cls, planes):
        rows, xcur, worst, active = state(dev, N)
        with torch.no_grad():
            logits = m.forward_u8(x)
        AT.select_u8(m, x, logits, N, 1, cls, 0.0, x, xcur, rows, worst, active, 0)
        assert int(active.sum()) == N
        cand, g = AT.propose_u8(m, x, xcur, cls, worst, planes, 1, active, 0, return_gains=True)
        return g.cpu().numpy(), cand.cpu().numpy(), worst.cpu().numpy()
    g0, c0, _ = gains_and_candidates(cls, planes)
    st2 = dict(st)
    st2["features.0.weight"] = st["features.0.weight"][:, ::-1].copy()   # the colour channels swapped: another Wsum, other stem bits
    rng = np.random.default_rng(3)
    st2["features.7.lin2.weight"] = (st["features.7.lin2.weight"] * rng.uniform(0.5, 1.5, st["features.7.lin2.weight"].shape)).astype(np.float32)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st2.items()}, strict=True)
    with torch.no_grad():
        cls = m.forward_u8(x).argmax(dim=1).to(torch.int32)             # the reloaded network's own classes: every image is open
    planes, unknown, _ = stem_planes(m, x, cls, 1)
    g1, c1, worst = gains_and_candidates(cls, planes)
    bits, feats = OB.unpack_rows(m.read_stage("features.4", N), 10), OB.unpack_rows(m.read_stage("features.5", N), 11)
    want_g = AT.gains_cpu(AT.head_cpu(st2), AT._words(tables(m)), bits, feats, unknown, cls.cpu().numpy(), worst)
    assert g1.tobytes() == want_g.tobytes() and not np.array_equal(g1, g0)
    scores = AT.scores_cpu(want_g, bits, unknown, CF.fold_bn(st2, "features.2")[0], AT.wsum_cpu(st2))
    want_c = AT.candidates_cpu(scores, U.images_np(), U.images_np(), 1)
    near = np.concatenate([np.repeat(U.threshold_band(scores)[:, k:k + 1], 4, axis=1) for k in range(2)], axis=1)
    assert near.sum() <= 1e-4 * near.size and np.array_equal(c1[~near], want_c[~near]) and not np.array_equal(c1, c0)


# ---- 6. error contract ----------------------------------------------------------------------------------------------------------------

def test_error_contract_of_the_c_abi(models, dev):
    model = models["cifar"]
    n = 4
    x, cls = images(dev)[:n].contiguous(), classes(dev, "cifar")[:n].contiguous()
    plan = model._plan_for(dev, n)
    lib = plan.lib
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    planes, _, _ = stem_planes(model, x, cls, 1)
    rows, xcur, worst, active = state(dev, n)
    cand = torch.zeros((n, 8, 32, 32, 3), dtype=torch.uint8, device=dev)
    gains = torch.zeros((n, 6400), dtype=torch.float64, device=dev)
    logits = torch.zeros((8 * n, 10), dtype=torch.float32, device=dev)
    with torch.no_grad():
        l0 = model.forward_u8(x)
    AT.select_u8(model, x, l0, n, 1, cls, 0.0, x, xcur, rows, worst, active, 0)
    P = lambda v: C.c_void_p(v)

    def propose(h=plan.handle, lane=0, x0=x.data_ptr(), xc=xcur.data_ptr(), n=n, c=cls.data_ptr(), w=worst.data_ptr(), pl=planes.data_ptr(),
                e=1, a=active.data_ptr(), cd=cand.data_ptr(), g=gains.data_ptr()):
        return lib.ttnet_attack_propose_u8(h, lane, P(x0), P(xc), n, P(c), P(w), P(pl), e, P(a), P(cd), P(g), s)

    def select(h=plan.handle, cd=cand.data_ptr(), lg=logits.data_ptr(), n=n, k=8, c=cls.data_ptr(), mm=0.0, x0=x.data_ptr(), xc=xcur.data_ptr(),
               r=rows.data_ptr(), w=worst.data_ptr(), a=active.data_ptr(), rnd=1):
        return lib.ttnet_attack_select_u8(h, P(cd), P(lg), n, k, P(c), mm, P(x0), P(xc), P(r), P(w), P(a), rnd, s)
    assert propose() == 0 and propose(g=None) == 0
    torch.cuda.synchronize()
    keep = [t.clone() for t in (cand, gains, rows, xcur, worst, active)]
    for kw in (dict(lane=2), dict(lane=-1), dict(n=0), dict(n=258), dict(e=-1), dict(e=65), dict(x0=None), dict(xc=None), dict(c=None),
               dict(w=None), dict(pl=None), dict(a=None), dict(cd=None), dict(x0=x.data_ptr() + 1), dict(xc=xcur.data_ptr() + 2),
               dict(c=cls.data_ptr() + 2), dict(w=worst.data_ptr() + 1), dict(a=active.data_ptr() + 3), dict(cd=cand.data_ptr() + 1),
               dict(pl=planes.data_ptr() + 4), dict(g=gains.data_ptr() + 4)):
        assert propose(**kw) == -1, kw
        assert lib.ttnet_last_error()
    assert propose(n=3) == -2                                            # the forward on the lane ran 4 images
    assert "last forward" in lib.ttnet_last_error().decode()
    for kw in (dict(n=0), dict(n=258), dict(k=0), dict(k=9), dict(rnd=-1), dict(mm=float("nan")), dict(cd=None), dict(lg=None), dict(c=None),
               dict(x0=None), dict(xc=None), dict(r=None), dict(w=None), dict(a=None), dict(cd=cand.data_ptr() + 1), dict(lg=logits.data_ptr() + 2),
               dict(r=rows.data_ptr() + 4), dict(xc=xcur.data_ptr() + 1), dict(w=worst.data_ptr() + 2), dict(a=active.data_ptr() + 2),
               dict(xc=x.data_ptr()), dict(xc=cand.data_ptr())):
        assert select(**kw) == -1, kw
        assert lib.ttnet_last_error()
    small = ttnet._Plan(spec_and_state("small")[0], args_for("small"), 0, 4)
    try:
        assert propose(h=small.handle) == -4 and "affine head" in lib.ttnet_last_error().decode()
        assert select(h=small.handle) == -4
    finally:
        small.close()
    raw = ttnet._Plan(spec_and_state("valexnet")[0], args_for("valexnet"), 0, 4)
    try:
        assert propose(h=raw.handle) == -2 and "ttnet_attack_propose_u8 before ttnet_plan_finalize" in lib.ttnet_last_error().decode()
        assert select(h=raw.handle) == -2 and "ttnet_attack_select_u8 before ttnet_plan_finalize" in lib.ttnet_last_error().decode()
    finally:
        raw.close()
    torch.cuda.synchronize()
    for t, k in zip((cand, gains, rows, xcur, worst, active), keep):     # nothing was launched in any error case
        assert torch.equal(t, k)
    assert select() == 0


# ---- 7. the command -----------------------------------------------------------------------------------------------------------------------

def test_command_prints_robust_lines(dev, tmp_path):
    model = new_model(dev, max_batch=128)                               # the command's plan: chunks of --eval_batch_size candidates
    n = 300
    u8 = synth.synth_images_u8(n, hw=(32, 32))
    labels = (np.arange(n) % 10).astype(np.int64)
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    np.concatenate([labels[:, None].astype(np.uint8), u8.reshape(n, 3072)], axis=1).tofile(str(d / "test_batch.bin"))
    x = np.ascontiguousarray(u8.transpose(0, 2, 3, 1))
    batches = list(cifar.device_batches(x, labels, 128, dev))
    certs = CF.certify_batches(model, batches, [0.5, 1.0, 2.5])
    found = AT.attack_batches(model, batches, [1.0, 2.5], 2, 1e-6, keep_witnesses=True)
    assert [a["images"] for a in found] == [n, n] and [a["levels"] for a in found] == [1, 2]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    rows_file, wit_file = tmp_path / "a.csv", tmp_path / "w.npz"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "scale_imagenet_amd.cifar", "--data_dir", str(tmp_path),
                        "--synthetic-ckpt", "--eval_batch_size", "128", "--certify", "0.5,1,2.5", "--attack", "--attack_rounds", "2",
                        "--attack_rows", str(rows_file), "--attack_witnesses", str(wit_file)],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == 7 and re.fullmatch(r"Acc\.\. (\S+) (\S+)", out[0])
    assert [out[1], out[3], out[5]] == [CF.verified_line(s) for s in certs]
    assert out[2].startswith("Robust.. eps=0.5 not searched")
    assert out[4] == AT.robust_line(1.0, certs[1]["rows"], found[0]["rows"])
    assert out[6] == AT.robust_line(2.5, certs[2]["rows"], found[1]["rows"]) + " [searched at floor(eps) = 2 byte levels]"
    assert re.fullmatch(r"Robust\.\. eps=1 certified \d+/300 <= robust <= \d+/300 \(falsified \d+: wrong at x0 \d+, by search \d+; open \d+\)", out[4])
    with open(rows_file, newline="") as f:
        got = list(csv.DictReader(f))
    assert len(got) == 2 * n
    for a, part in zip(found, (got[:n], got[n:])):
        assert [int(g["status"]) for g in part] == a["rows"]["status"].tolist() and [int(g["class"]) for g in part] == labels.tolist()
        assert np.array_equal(np.array([float(g["best"]) for g in part], dtype=np.float32), a["rows"]["best"])
    with np.load(wit_file) as z:
        assert sorted(z.files) == ["eps_1", "eps_2.5", "status_1", "status_2.5"]
        assert np.array_equal(z["eps_1"], found[0]["witnesses"]) and np.array_equal(z["status_2.5"], found[1]["rows"]["status"])
    assert sorted(os.listdir(tmp_path)) == ["a.csv", "cifar-10-batches-bin", "w.npz"]
    # without --attack the command prints what it printed
    r2 = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "scale_imagenet_amd.cifar", "--data_dir", str(tmp_path),
                         "--synthetic-ckpt", "--eval_batch_size", "128", "--certify", "0.5,1,2.5"], capture_output=True, text=True, env=env,
                        cwd=str(tmp_path))
    assert r2.returncode == 0 and r2.stdout.splitlines() == [out[0], out[1], out[3], out[5]]
