"""Falsified L-infinity robustness of ``TT_FHE_XSMALL_vAlexnet``: a search for uint8 witnesses.  (include/ttnet.h:
ttnet_attack_propose_u8, ttnet_attack_select_u8; DESIGN.md: falsified robustness.)

``certify`` bounds the robust accuracy from below.  This module bounds it from above: an image is *falsified* when the
device holds a concrete uint8 image inside the integer box ``[max(0, b - e), min(255, b + e)]`` (``e = floor(eps)`` byte
levels, a subset of the certificate's real box) on which ``forward_u8`` no longer gives the class.  A witness is checked by
the forward itself, so a falsified image is never wrong; a search is not a decision, so an open image stays open.

    certified / N  <=  robust accuracy  <=  (N - falsified) / N

One round, per open image: the flip gain of every stem bit that the box can move (the certificate's stem planes), from the
truth tables and the effective head; a push per stem bit; a score per input byte through the summed stem kernels; eight
candidates (two modes, four thresholds) whose forwards a select step compares.  ``attack_u8`` / ``attack_batches`` run on
the device (csrc/attack.hip); ``gains_cpu``, ``scores_cpu``, ``candidates_cpu``, ``select_cpu`` and ``attack_cpu`` are
the numpy float64 twin: the same sums in the same order, the same record.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import certify as CF
from .cifar import CIFAR_MEAN, CIFAR_STD
from .valexnet_block import FEAT_CH, N_REACH, POOL, SIDE, STEM_CH, f64, fold_bn, reached, table_words, window_indices  # noqa: F401
from .valexnet_block import block_words as _words

RECORD = np.dtype([("margin0", "<f4"), ("best", "<f4"), ("worst", "<i4"), ("status", "<i4"), ("round", "<i4"),
                   ("changed", "<i4"), ("linf", "<i4"), ("tried", "<i4")])     # the 32-byte record of ttnet_attack_select_u8
OPEN, WRONG, FALSIFIED = 0, 1, 2
TAUS = (0.0, 0.125, 0.25, 0.5)
N_CAND = 2 * len(TAUS)
EPS_LEVELS_MAX, ROUNDS_MAX = 64, 8
# A margin is a difference of forward_u8 logits, and lin1's split-K count -- with it the last bits of a float32 logit --
# depends on the number of images in a forward (csrc/head.hip: gemm_f16x2_splits).  Up to 256 images the count is the same, so
# the search never forwards more at a time: the record of an image then does not depend on the batch it came in
# (tests/test_gpu_attack.py checks the forward for this).
FORWARD_ROWS = 256
ROWS_HEADER = ["index", "class", "status", "falsified", "margin0", "best", "worst", "round", "changed", "linf", "tried"]


def eps_levels(eps: float) -> int:
    """``floor(eps)``: the byte levels of the integer box inside the certificate's real box at ``eps``."""
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    e = int(math.floor(eps))
    if e > EPS_LEVELS_MAX:
        raise ValueError(f"eps must be at most {EPS_LEVELS_MAX} byte levels, got {eps}")
    return e


# ---- the device path ---------------------------------------------------------------------------------------------------

class AttackResult:
    """What ``attack_u8`` leaves on the device: ``rows`` int32 ``[n, 8]`` holding the n 32-byte records (``numpy()`` gives
    them as dtype ``RECORD``), ``witnesses`` uint8 ``[n, 32, 32, 3]`` (the image of the smallest margin found: inside the box
    for every image, a counter-example where ``falsified``), and ``falsified`` (bool ``[n]``: status 1 or 2)."""

    def __init__(self, rows, witnesses):
        self.rows = rows
        self.witnesses = witnesses
        self.status = rows[:, 3]

    def __len__(self):
        return self.rows.shape[0]

    @property
    def falsified(self):
        return self.status > 0

    def numpy(self) -> np.ndarray:
        """The records as a structured array of dtype ``RECORD`` (synchronises)."""
        return self.rows.cpu().numpy().view(RECORD).reshape(-1)


def _forward_into(plan, lane: int, x, out, stream):
    from . import _lib
    _lib.check(plan.lib.ttnet_forward_u8(plan.handle, int(lane), C.c_void_p(x.data_ptr()), x.shape[0], C.c_void_p(out.data_ptr()),
                                         C.c_void_p(stream)))


def propose_u8(model, x0, xcur, classes, worst, stem_planes, levels: int, active, lane: int = 0, return_gains: bool = False):
    """One ``ttnet_attack_propose_u8`` call on the stage buffers of the forward last issued on ``lane`` (which must have
    been the forward of ``xcur``).  ``stem_planes``: int64 ``[2, n, 64, 10]`` (lo, hi).  Returns the candidates uint8
    ``[n, 8, 32, 32, 3]`` and, with ``return_gains``, the flip gains float64 ``[n, 64, 10, 10]``."""
    import torch

    from . import _lib
    n = x0.shape[0]
    plan = model._plan_for(x0.device, n)
    cand = torch.empty((n, N_CAND, 32, 32, 3), dtype=torch.uint8, device=x0.device)
    gains = torch.empty((n, 64, 10, 10), dtype=torch.float64, device=x0.device) if return_gains else None
    stream = torch.cuda.current_stream(x0.device).cuda_stream
    _lib.check(plan.lib.ttnet_attack_propose_u8(plan.handle, int(lane), C.c_void_p(x0.data_ptr()), C.c_void_p(xcur.data_ptr()), n,
                                                C.c_void_p(classes.data_ptr()), C.c_void_p(worst.data_ptr()),
                                                C.c_void_p(stem_planes.data_ptr()), int(levels), C.c_void_p(active.data_ptr()),
                                                C.c_void_p(cand.data_ptr()), C.c_void_p(gains.data_ptr() if return_gains else None),
                                                C.c_void_p(stream)))
    return (cand, gains) if return_gains else cand


def select_u8(model, cand, logits, n: int, n_cand: int, classes, min_margin: float, x0, xcur, rows, worst, active, rnd: int):
    """One ``ttnet_attack_select_u8`` call: updates ``xcur``, ``rows``, ``worst`` and ``active`` in place."""
    import torch

    from . import _lib
    plan = model._plan_for(x0.device, n)
    stream = torch.cuda.current_stream(x0.device).cuda_stream
    _lib.check(plan.lib.ttnet_attack_select_u8(plan.handle, C.c_void_p(cand.data_ptr()), C.c_void_p(logits.data_ptr()), n, int(n_cand),
                                               C.c_void_p(classes.data_ptr()), float(min_margin), C.c_void_p(x0.data_ptr()),
                                               C.c_void_p(xcur.data_ptr()), C.c_void_p(rows.data_ptr()), C.c_void_p(worst.data_ptr()),
                                               C.c_void_p(active.data_ptr()), int(rnd), C.c_void_p(stream)))


def attack_u8(model, x_u8, classes, eps: float, rounds: int = 3, min_margin: float = 0.0, lane: int = 0, planes=None) -> AttackResult:
    """Search the integer box of ``floor(eps)`` byte levels around every image of ``x_u8`` (uint8 HIP tensor
    ``[N, 32, 32, 3]``) for an image on which ``forward_u8`` does not give ``classes[i]`` by more than ``min_margin``.
    ``planes``: the certificate's stem planes at this eps, int64 ``(lo, hi)`` each ``[N, 64, 10]`` (``certify_u8(..,
    return_planes=True).planes``); without them the certificate is run first.  Each round costs one forward of the
    current images and eight of the candidates, all on ``lane``.  More than ``FORWARD_ROWS`` images are searched in parts of
    that size and no forward is larger, so an image's record and witness do not depend on the batch it came in.
    Asynchronous on the current stream; nothing is read back."""
    import torch
    x0, classes = CF.checked_inputs(model, x_u8, classes, "attack_u8", "the search needs the certificate's stem planes,")
    n, dev = x0.shape[0], x0.device
    levels = eps_levels(eps)
    if not 0 <= int(rounds) <= ROUNDS_MAX:
        raise ValueError(f"rounds must be in [0, {ROUNDS_MAX}], got {rounds}")
    if math.isnan(min_margin):
        raise ValueError("min_margin is NaN")
    if planes is not None:
        planes = tuple(torch.as_tensor(p).reshape(n, 64, 10).to(device=dev, dtype=torch.int64) for p in planes)
    rows = torch.empty((n, 8), dtype=torch.int32, device=dev)
    xcur = torch.empty_like(x0)
    for a in range(0, n, FORWARD_ROWS):                  # parts of at most FORWARD_ROWS images, each searched on its own
        b = min(n, a + FORWARD_ROWS)
        part = None if planes is None else (planes[0][a:b], planes[1][a:b])
        _attack_part(model, x0[a:b], classes[a:b], eps, levels, int(rounds), min_margin, lane, part, rows[a:b], xcur[a:b])
    return AttackResult(rows, xcur)


def _attack_part(model, x0, classes, eps, levels, rounds, min_margin, lane, planes, rows, xcur):
    """The rounds of ``attack_u8`` for at most ``FORWARD_ROWS`` images; ``rows`` and ``xcur`` are written in place."""
    import torch
    n, dev = x0.shape[0], x0.device
    if planes is None and rounds > 0:
        p = CF.certify_u8(model, x0, classes, eps, 0, max(min_margin, 0.0), lane, return_planes=True).planes
        planes = (p["stem_lo"], p["stem_hi"])
    plan = model._plan_for(dev, n)
    chunk = min(plan.max_batch, FORWARD_ROWS)
    stream = torch.cuda.current_stream(dev).cuda_stream
    worst = torch.empty(n, dtype=torch.int32, device=dev)
    active = torch.empty(n, dtype=torch.int32, device=dev)
    logits = torch.empty((n * N_CAND, 10), dtype=torch.float32, device=dev)
    _forward_into(plan, lane, x0, logits[:n], stream)
    select_u8(model, x0, logits, n, 1, classes, min_margin, x0, xcur, rows, worst, active, 0)
    if rounds > 0:
        stem = torch.stack([planes[0].reshape(n, 64, 10), planes[1].reshape(n, 64, 10)]).contiguous()
    for r in range(1, rounds + 1):
        if r > 1:                                        # (in round 1 the lane still holds the forward of x0 = xcur)
            _forward_into(plan, lane, xcur, logits[:n], stream)
        cand = propose_u8(model, x0, xcur, classes, worst, stem, levels, active, lane)
        flat = cand.view(n * N_CAND, 32, 32, 3)
        for a in range(0, n * N_CAND, chunk):
            _forward_into(plan, lane, flat[a:a + chunk], logits[a:a + chunk], stream)
        select_u8(model, cand, logits, n, N_CAND, classes, min_margin, x0, xcur, rows, worst, active, r)


def summarise(eps: float, rows: np.ndarray, rounds: int) -> dict:
    """What ``attack_batches`` reports per eps, from the records of all images."""
    by_round = [int(((rows["status"] == FALSIFIED) & (rows["round"] == r)).sum()) for r in range(1, rounds + 1)]
    return {"eps": float(eps), "levels": int(math.floor(eps)), "images": int(rows.size), "wrong": int((rows["status"] == WRONG).sum()),
            "search": int((rows["status"] == FALSIFIED).sum()), "falsified": int((rows["status"] > 0).sum()), "by_round": by_round,
            "rows": rows}


def attack_batches(model, batches: Iterable, eps_list: Sequence[float], rounds: int = 3, min_margin: float = 0.0, lane: int = 0,
                   keep_witnesses: bool = False) -> List[dict]:
    """``attack_u8`` on the targets of ``batches`` (pairs ``(uint8 images, int64 targets)`` on the device) at every eps of
    ``eps_list``.  One dict per eps: ``eps, levels, images, wrong, search, falsified, by_round`` and ``rows`` (dtype
    ``RECORD``, dataset order); with ``keep_witnesses`` also ``witnesses`` (uint8 numpy ``[N, 32, 32, 3]``).  The records
    stay on the device until the last batch."""
    import torch
    eps_list = [float(e) for e in eps_list]
    parts: List[List] = [[] for _ in eps_list]
    wits: List[List] = [[] for _ in eps_list]
    for x, t in batches:
        for i, eps in enumerate(eps_list):
            res = attack_u8(model, x, t, eps, rounds, min_margin, lane)
            parts[i].append(res.rows)
            if keep_witnesses:
                wits[i].append(res.witnesses)
    out = []
    for i, eps in enumerate(eps_list):
        rows = torch.cat(parts[i]).cpu().numpy().view(RECORD).reshape(-1) if parts[i] else np.zeros(0, dtype=RECORD)
        s = summarise(eps, rows, rounds)
        if keep_witnesses:
            s["witnesses"] = torch.cat(wits[i]).cpu().numpy() if wits[i] else np.zeros((0, 32, 32, 3), np.uint8)
        out.append(s)
    return out


def robust_bounds(certify_rows: np.ndarray, attack_rows: np.ndarray) -> Tuple[int, int, int]:
    """``(certified, falsified, open)`` of the same images from the records of the certificate and of the search.  An image
    in both is a bug in one of the two: ``ValueError`` names the first."""
    cert = np.asarray(certify_rows["stage"]) > 0
    fals = np.asarray(attack_rows["status"]) > 0
    if cert.shape != fals.shape:
        raise ValueError(f"{cert.size} certificates for {fals.size} attack records")
    both = np.flatnonzero(cert & fals)
    if both.size:
        raise ValueError(f"image {int(both[0])} is both certified and falsified ({both.size} such images): a bug in the "
                         "certificate or in the search")
    return int(cert.sum()), int(fals.sum()), int(cert.size - cert.sum() - fals.sum())


def robust_line(eps: float, certify_rows: np.ndarray, attack_rows: np.ndarray) -> str:
    """``Robust.. eps=E certified a/N <= robust <= b/N (falsified f: wrong at x0 w, by search s; open o)``"""
    a, f, o = robust_bounds(certify_rows, attack_rows)
    n = int(np.asarray(attack_rows).size)
    w = int((attack_rows["status"] == WRONG).sum())
    return (f"Robust.. eps={eps:g} certified {a}/{n} <= robust <= {n - f}/{n} (falsified {f}: wrong at x0 {w}, by search {f - w}; "
            f"open {o})")


def rows_csv_rows(summaries: Sequence[dict], classes: Sequence[int]) -> List[list]:
    """Header first, then one row per (eps, image): eps, then the columns of ``ROWS_HEADER``; floats with ``repr``."""
    out = [["eps"] + ROWS_HEADER]
    for s in summaries:
        if len(classes) != s["rows"].size:
            raise ValueError(f"{len(classes)} classes for {s['rows'].size} records")
        for i, (r, c) in enumerate(zip(s["rows"], classes)):
            out.append([repr(float(s["eps"])), i, int(c), int(r["status"]), int(r["status"] > 0), repr(float(r["margin0"])),
                        repr(float(r["best"])), int(r["worst"]), int(r["round"]), int(r["changed"]), int(r["linf"]), int(r["tried"])])
    return out


def write_rows_csv(path: Optional[str], summaries: Sequence[dict], classes: Sequence[int]):
    """The records of ``attack_batches`` as CSV (``path`` None: standard output); written to a temporary name and renamed."""
    from .report import write_csv
    write_csv(path, rows_csv_rows(summaries, classes))


# ---- the numpy float64 twin ----------------------------------------------------------------------------------------------

def wsum_cpu(state) -> np.ndarray:
    """``Wsum[ch][k][5][5]``: the nine 3 x 3 stem kernels of channel ch, input channel k, shifted to the nine positions
    (dy, dx ascending) of the MaxPool(3) window and summed, float64 from the float32 weights.  Entry [r][q] weighs the pixel
    in row ``3 py - 1 + r``, column ``3 px - 1 + q`` of the 5 x 5 field of pooled cell (py, px)."""
    w = f64(state["features.0.weight"])
    out = np.zeros((64, 3, 5, 5))
    for dy in range(3):
        for dx in range(3):
            out[:, :, dy:dy + 3, dx:dx + 3] = out[:, :, dy:dy + 3, dx:dx + 3] + w
    return out


def head_cpu(state) -> np.ndarray:
    """The effective head ``A = lin2 diag(bn_scale) lin1`` float64 ``[10, 30976]`` summed the way the device sums it (the
    hidden unit i ascending, every product and every sum rounded on its own), so that ``D_f`` has the device's bytes;
    ``certify.effective_head`` leaves the order to the BLAS and agrees to rounding."""
    s, _ = fold_bn(state, "features.7.BN2")
    m = f64(state["features.7.lin2.weight"]) * s[None, :]
    lin1 = f64(state["features.7.lin1.weight"])
    A = np.zeros((m.shape[0], lin1.shape[1]))
    for i in range(m.shape[1]):
        A = A + m[:, i, None] * lin1[i][None, :]
    return A


def reached_features() -> np.ndarray:
    """int64 ``[21, 64, 10, 10]``: the flat index (``channel * 121 + oy * 11 + ox`` of the 256 x 11 x 11 features) of the
    features whose windows hold stem bit (ch, py, px), in the order of the gain's sum (``valexnet_block.reach``); -1 where a
    window would lie outside the plane."""
    valid, fc, oy, ox, _ = reached()
    return np.where(valid != 0, (fc * SIDE + oy) * SIDE + ox, -1)


def gains_cpu(A: np.ndarray, words, stem_bits: np.ndarray, feat_bits: np.ndarray, unknown: np.ndarray, classes, worst,
              return_changed: bool = False):
    """Flip gains float64 ``[n, 64, 10, 10]``: for every stem bit s marked in ``unknown`` the change of ``logit_c -
    logit_j`` (c = ``classes[i]``, j = ``worst[i]``, through ``A`` ``[10, 30976]``) when s alone flips, zero elsewhere and
    for an image whose c or j is no class.  ``stem_bits`` ``[n, 64, 10, 10]``, ``feat_bits`` ``[n, 256, 11, 11]`` (what the
    forward produced: y before the flip), ``words = [table_words(conv1), (conv2), (conv3)]``.  The sum runs over the at most
    21 features whose windows hold s, in the order of ``valexnet_block.reach``: the feature's table read at its index with
    input p flipped, and every term is +D_f, -D_f or nothing.  ``return_changed``: also bool ``[n, 21, 64, 10, 10]``, which of
    the 21 features change."""
    stem_bits = np.asarray(stem_bits).astype(np.int64)
    feat = np.asarray(feat_bits).astype(np.int64)
    n = stem_bits.shape[0]
    classes, worst = np.asarray(classes).astype(np.int64), np.asarray(worst).astype(np.int64)
    ok = (classes >= 0) & (classes < 10) & (worst >= 0) & (worst < 10)
    c, j = np.where(ok, classes, 0), np.where(ok, worst, 0)
    D = (A[c] - A[j]).reshape(n, FEAT_CH, SIDE, SIDE)
    idx = window_indices(stem_bits)                                        # [n, 64, 10, 11], [n, 64, 11, 10], [n, 8, 10, 10]
    T1, T2, T3 = words[0][:, 0, 0], words[1][:, 0, 0], words[2]              # [64], [64], [8, 8, 4]
    ch, py, px = np.meshgrid(np.arange(STEM_CH), np.arange(POOL), np.arange(POOL), indexing="ij")
    g = np.zeros((n, STEM_CH, POOL, POOL))
    changed = np.zeros((n, N_REACH, STEM_CH, POOL, POOL), dtype=bool)

    def bit(T, i):
        return ((T >> i.astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    for t, (valid, fc, oy, ox, p) in enumerate(zip(*reached())):
        valid = valid != 0
        oy, ox = np.where(valid, oy, 0), np.where(valid, ox, 0)            # (a window outside the plane: any entry, masked below)
        kind, old = int(fc[0, 0, 0]) // 64, feat[:, fc, oy, ox]
        if kind < 2:                                                       # conv1 / conv2: the channel's 64-entry table
            new = bit((T1, T2)[kind][ch], idx[kind][:, ch, oy, ox] ^ (1 << p))
        elif kind == 2:                                                    # conv3: output fc of the group, four words
            i3 = idx[2][:, ch // 8, py, px] ^ (1 << p)
            w = np.broadcast_to(T3[(fc - 128) // 8, fc % 8], i3.shape + (4,))
            new = bit(np.take_along_axis(w, (i3 >> 6)[..., None], axis=-1)[..., 0], i3 & 63)
        else:                                                              # out4 carries the bit itself
            new, old = 1 - stem_bits, stem_bits
        d = np.where(valid, new - old, 0)
        Df = D[:, fc, oy, ox]
        g = g + np.where(d == 1, Df, np.where(d == -1, -Df, 0.0))
        changed[:, t] = d != 0
    keep = np.asarray(unknown).astype(bool) & ok[:, None, None, None]
    g = np.where(keep, g, 0.0)
    return (g, changed & keep[:, None]) if return_changed else g


def scores_cpu(gains: np.ndarray, stem_bits: np.ndarray, unknown: np.ndarray, bn_scale: np.ndarray, Wsum: np.ndarray) -> np.ndarray:
    """Pixel scores float64 ``[n, 2 modes, 32, 32, 3]``.  The push of stem bit s is ``wt_s = -g_s (bit_s == 0 ? +1 : -1)
    sign(bn_scale[ch])``: in mode 0 for the unknown bits with ``g_s < 0`` (zero elsewhere), in mode 1 for every unknown bit.
    ``score[y][x][k] = sum_s wt_s Wsum[ch_s][k][y - 3 py_s + 1][x - 3 px_s + 1]`` over the bits whose 5 x 5 field holds the
    pixel, ch ascending, then py, then px; products and sums rounded one by one."""
    unknown = np.asarray(unknown).astype(bool)
    sgn = np.where(np.asarray(stem_bits) == 0, 1.0, -1.0) * np.where(bn_scale >= 0, 1.0, -1.0)[None, :, None, None]
    wt1 = np.where(unknown, -gains * sgn, 0.0)
    wt = (np.where(gains < 0, wt1, 0.0), wt1)
    n = gains.shape[0]
    y = np.arange(32)
    hi = (y + 1) // 3                                                      # the later cell whose field holds row / column y ..
    cells = np.stack([hi - 1, hi], axis=1)                                 # .. and the one before it, ascending
    offs = y[:, None] - 3 * cells + 1
    valid = (cells >= 0) & (cells <= 9) & (offs >= 0) & (offs <= 4)
    cells, offs = np.clip(cells, 0, 9), np.clip(offs, 0, 4)
    # per (a, b): the pushes and the kernels gathered to the pixels.  A cell that does not hold the pixel gets the weight
    # zero; its term is then +-0, which changes no sum (the sums start at +0 and never become -0).
    ab = [(a, b) for a in range(2) for b in range(2)]
    W = [np.where((valid[:, a][:, None] & valid[:, b][None, :])[None, :, :, None],
                  Wsum[:, :, offs[:, a]][:, :, :, offs[:, b]].transpose(0, 2, 3, 1), 0.0) for a, b in ab]      # [64, 32, 32, 3]
    G = [[w[:, :, cells[:, a]][:, :, :, cells[:, b]] for a, b in ab] for w in wt]                              # [n, 64, 32, 32]
    out = np.zeros((2, n, 32, 32, 3))
    for ch in range(64):
        for q in range(4):
            for m in range(2):
                out[m] += G[m][q][:, ch, :, :, None] * W[q][ch][None]
    return np.ascontiguousarray(out.transpose(1, 0, 2, 3, 4))


def candidates_cpu(scores: np.ndarray, x0: np.ndarray, xcur: np.ndarray, levels: int, active=None) -> np.ndarray:
    """The eight candidates uint8 ``[n, 8, 32, 32, 3]``, index ``4 mode + tau index``: with ``M = max |score|`` of the image
    and mode, a byte is selected when ``score != 0 and |score| > tau M``; selected bytes take the upper (score > 0) or lower
    end of the clipped box of ``x0``, every other byte keeps ``xcur``.  An image with ``active[i] == 0`` gets eight copies of
    ``xcur``."""
    x0, xcur = np.asarray(x0), np.asarray(xcur)
    n = x0.shape[0]
    up = np.minimum(255, x0.astype(np.int64) + levels).astype(np.uint8)
    dn = np.maximum(0, x0.astype(np.int64) - levels).astype(np.uint8)
    act = np.ones(n, bool) if active is None else np.asarray(active).astype(bool)
    out = np.empty((n, N_CAND, 32, 32, 3), dtype=np.uint8)
    for m in range(2):
        s = scores[:, m]
        mag = np.abs(s)
        M = mag.reshape(n, -1).max(axis=1)[:, None, None, None]
        for t, tau in enumerate(TAUS):
            sel = (s != 0) & (mag > tau * M) & act[:, None, None, None]
            out[:, 4 * m + t] = np.where(sel, np.where(s > 0, up, dn), xcur)
    return out


def new_state(n: int):
    """``(rows, xcur, worst, active)`` for ``select_cpu`` to initialise in round 0."""
    return np.zeros(n, dtype=RECORD), np.zeros((n, 32, 32, 3), np.uint8), np.full(n, -1, np.int32), np.zeros(n, np.int32)


def select_cpu(cand: np.ndarray, logits: np.ndarray, n_cand: int, classes, min_margin: float, x0: np.ndarray, xcur: np.ndarray,
               rows: np.ndarray, worst: np.ndarray, active: np.ndarray, rnd: int):
    """The twin of ``ttnet_attack_select_u8``; ``xcur``, ``rows``, ``worst``, ``active`` are updated in place.  ``cand``
    ``[n, n_cand, 32, 32, 3]``, ``logits`` float32 ``[n * n_cand, 10]``."""
    n = x0.shape[0]
    cand = np.asarray(cand).reshape(n, n_cand, 32, 32, 3)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1, 10)[:n * n_cand].reshape(n, n_cand, 10)
    classes = np.asarray(classes).astype(np.int64)
    thr = np.float32(-np.float32(min_margin))
    for i in range(n):
        c = int(classes[i])
        if rnd == 0:
            rows[i] = (np.nan, np.inf, -1, OPEN, 0, 0, 0, 0)
            xcur[i] = x0[i]
            worst[i] = -1
            active[i] = 1 if 0 <= c < 10 else 0
            if not active[i]:
                rows[i]["margin0"] = rows[i]["best"] = -np.inf
        if not active[i]:
            continue
        best_m, best_k, best_j = np.float32(np.inf), -1, -1
        for k in range(n_cand):
            l = logits[i, k]
            if np.isnan(l).any():
                continue
            j = max((q for q in range(10) if q != c), key=lambda q: l[q])   # (the first of equal maxima)
            with np.errstate(invalid="ignore"):                             # (inf - inf: a NaN margin, below nothing)
                m = np.float32(l[c] - l[j])
            if rnd == 0 and k == 0:
                rows[i]["margin0"] = m
            if m < best_m:
                best_m, best_k, best_j = m, k, j
        rows[i]["tried"] += n_cand
        if best_k < 0 or not best_m < rows[i]["best"]:
            continue
        xcur[i] = cand[i, best_k]
        d = np.abs(xcur[i].astype(np.int64) - x0[i].astype(np.int64))
        rows[i]["best"], rows[i]["worst"], rows[i]["round"] = best_m, best_j, rnd
        rows[i]["changed"], rows[i]["linf"] = int((d != 0).sum()), int(d.max())
        worst[i] = best_j
        if best_m < thr:
            rows[i]["status"] = WRONG if rnd == 0 else FALSIFIED
            active[i] = 0


def attack_cpu(state, tables, x_u8, classes, eps: float, rounds: int = 3, min_margin: float = 0.0, *, forward: Callable,
               mean=CIFAR_MEAN, std=CIFAR_STD, planes=None):
    """The numpy float64 twin of ``attack_u8``.  ``forward(x_u8) -> (stem bits [n, 64, 10, 10], feature bits [n, 256, 11, 11],
    logits [n, 10])`` stands in for ``forward_u8`` and its stage buffers; ``planes``: ``(lo_bit, hi_bit)`` uint8
    ``[n, 64, 10, 10]`` instead of the twin's own stage 0 at ``eps``.  Returns ``(rows, witnesses)``."""
    x0 = np.asarray(x_u8)
    n = x0.shape[0]
    classes = np.asarray(classes).astype(np.int64).reshape(-1)
    if x0.dtype != np.uint8 or x0.shape[1:] != (32, 32, 3) or classes.size != n:
        raise ValueError(f"expected uint8 images [n, 32, 32, 3] and n classes, got {x0.dtype} {x0.shape}, {classes.size}")
    levels = eps_levels(eps)
    if not 0 <= int(rounds) <= ROUNDS_MAX:
        raise ValueError(f"rounds must be in [0, {ROUNDS_MAX}], got {rounds}")
    rows, xcur, worst, active = new_state(n)
    stem, feat, logits = forward(x0)
    select_cpu(x0[:, None], logits, 1, classes, min_margin, x0, xcur, rows, worst, active, 0)
    if rounds > 0:
        lo, hi = planes if planes is not None else CF.stem_planes_cpu(state, x0, eps, mean, std)
        unknown = np.asarray(lo) != np.asarray(hi)
        A = head_cpu(state)
        words, Wsum, scale = _words(tables), wsum_cpu(state), fold_bn(state, "features.2")[0]
    for r in range(1, int(rounds) + 1):
        if r > 1:
            stem, feat, _ = forward(xcur)
        g = gains_cpu(A, words, stem, feat, unknown, classes, worst)
        cand = candidates_cpu(scores_cpu(g, stem, unknown, scale, Wsum), x0, xcur, levels, active)
        _, _, logits = forward(cand.reshape(-1, 32, 32, 3))
        select_cpu(cand, logits, N_CAND, classes, min_margin, x0, xcur, rows, worst, active, r)
    return rows, xcur
