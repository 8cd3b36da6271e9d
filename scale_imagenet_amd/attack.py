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
from .valexnet_block import FEAT_CH, N_REACH, POOL, SIDE, STEM_CH, f64, fold_bn, reach, reached, table_words, window_indices  # noqa: F401
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


def _table_rows(words):
    """``(T1 [64], T2 [64], T3 [64, 4])`` of ``words = [table_words(conv1), (conv2), (conv3)]``: a table per output channel."""
    return words[0][:, 0, 0], words[1][:, 0, 0], words[2].reshape(STEM_CH, 4)


def gains_listed(A: np.ndarray, T, pad: np.ndarray, pi, ch, y, x, c, j, feat=None):
    """Flip gains float64 ``[B]`` of the listed stem bits ``(pi, ch, y, x)`` -- ``pi``: the plane of ``pad`` each lives in; ``pad``:
    int64 ``[n, 64, 12, 12]``, the stem bits with the zero padding around them -- and bool ``[B, 21]``, which of the 21 features
    change: for bit s the change of ``logit_c - logit_j`` (``c``, ``j`` per listed bit or scalars, through ``A`` ``[10, 30976]``) when
    s alone flips.  The sum runs over the at most 21 features whose windows hold s, in the order of ``valexnet_block.reach``: the
    feature's table (``T = _table_rows(words)``) read at its index with input p flipped against the feature before the flip --
    ``feat`` ``[n, 256, 11, 11]`` where given (what a forward produced), else the table at the unflipped index -- and every
    term is +D_f, -D_f or nothing."""
    def bit(T, i):
        return ((T >> i.astype(np.uint64)) & np.uint64(1)).astype(np.int64)
    g = np.zeros(pi.size)
    changed = np.zeros((pi.size, N_REACH), dtype=bool)
    for t in range(N_REACH):
        valid, fc, oy, ox, p = reach(ch, y, x, t)
        valid = np.broadcast_to(np.asarray(valid, dtype=bool), pi.shape)
        oy, ox = np.where(valid, oy, 0), np.where(valid, ox, 0)            # (a window outside the plane: any entry, masked below)
        kind = 0 if t < 6 else 1 if t < 12 else 2 if t < 20 else 3
        if kind < 2:                                                       # conv1 / conv2: the channel's 64-entry table
            kw = (2, 3)[kind]
            idx = sum(pad[pi, ch, oy + q // kw, ox + q % kw] << q for q in range(6))
            new, old = bit(T[kind][ch], idx ^ (1 << p)), bit(T[kind][ch], idx)
        elif kind == 2:                                                    # conv3: output fc of the group, four words
            idx = sum(pad[pi, ch // 8 * 8 + q, y + 1, x + 1] << q for q in range(8))
            i3 = idx ^ (1 << p)
            new, old = bit(T[2][fc - 128, i3 >> 6], i3 & 63), bit(T[2][fc - 128, idx >> 6], idx & 63)
        else:                                                              # out4 carries the bit itself
            old = pad[pi, ch, y + 1, x + 1]
            new = 1 - old
        if feat is not None and kind < 3:
            old = feat[pi, fc, oy, ox]
        d = np.where(valid, new - old, 0)
        f = (fc * SIDE + oy) * SIDE + ox
        Df = A[c, f] - A[j, f]
        g = g + np.where(d == 1, Df, np.where(d == -1, -Df, 0.0))
        changed[:, t] = d != 0
    return g, changed


def gains_cpu(A: np.ndarray, words, stem_bits: np.ndarray, feat_bits: np.ndarray, unknown: np.ndarray, classes, worst,
              return_changed: bool = False):
    """Flip gains float64 ``[n, 64, 10, 10]``: ``gains_listed`` on every stem bit marked in ``unknown`` (c = ``classes[i]``, j =
    ``worst[i]``), zero elsewhere and for an image whose c or j is no class.  ``stem_bits`` ``[n, 64, 10, 10]``, ``feat_bits``
    ``[n, 256, 11, 11]`` (what the forward produced: y before the flip), ``words = [table_words(conv1), (conv2), (conv3)]``.
    ``return_changed``: also bool ``[n, 21, 64, 10, 10]``, which of the 21 features change."""
    stem_bits = np.asarray(stem_bits).astype(np.int64)
    n = stem_bits.shape[0]
    classes, worst = np.asarray(classes).astype(np.int64), np.asarray(worst).astype(np.int64)
    ok = (classes >= 0) & (classes < 10) & (worst >= 0) & (worst < 10)
    pi, ch, y, x = np.nonzero(np.asarray(unknown).astype(bool) & ok[:, None, None, None])
    g = np.zeros((n, STEM_CH, POOL, POOL))
    changed = np.zeros((n, N_REACH, STEM_CH, POOL, POOL), dtype=bool)
    g[pi, ch, y, x], changed[pi, :, ch, y, x] = gains_listed(A, _table_rows(words), np.pad(stem_bits, ((0, 0), (0, 0), (1, 1), (1, 1))), pi, ch,
                                                             y, x, classes[pi], worst[pi], np.asarray(feat_bits).astype(np.int64))
    return (g, changed) if return_changed else g


def _cells_of(v: np.ndarray):
    """The two cells whose 5-wide field may hold row / column v (ascending), v's offset in each, and whether it does."""
    hi = (v + 1) // 3
    cells = np.stack([hi - 1, hi], axis=-1)
    offs = v[..., None] - 3 * cells + 1
    valid = (cells >= 0) & (cells <= 9) & (offs >= 0) & (offs <= 4)
    return np.clip(cells, 0, 9), np.clip(offs, 0, 4), valid


def scores_rect(wt, Wsum: np.ndarray, y0, x0, h: int, w: int) -> np.ndarray:
    """Scores float64 ``[2 modes, B, h, w, 3]`` of the bytes of the h x w rectangle at ``(y0[i], x0[i])`` of image i from the pushes
    ``wt[m]`` ``[B, 64, 10, 10]`` of mode m: ``score[y][x][k] = sum_s wt_s Wsum[ch_s][k][y - 3 py_s + 1][x - 3 px_s + 1]`` over the stem
    bits whose 5 x 5 field holds the pixel, ch ascending, then py, then px; products and sums rounded one by one.  A cell that does
    not hold the pixel gets the weight zero; its term is then +-0, which changes no sum (the sums start at +0 and never become
    -0), and a channel without a push is skipped for the same reason."""
    B = y0.size
    cy, oy, vy = _cells_of(y0[:, None] + np.arange(h)[None, :])            # [B, h, 2]
    cx, ox, vx = _cells_of(x0[:, None] + np.arange(w)[None, :])
    out = np.zeros((2, B, h, w, 3))
    b = np.arange(B)[:, None, None]
    for ch in np.flatnonzero((wt[1] != 0).reshape(B, STEM_CH, -1).any(axis=(0, 2))):
        for a_ in range(2):
            for b_ in range(2):
                v = vy[:, :, a_][:, :, None] & vx[:, :, b_][:, None, :]
                W = np.where(v[..., None], Wsum[ch][:, oy[:, :, a_][:, :, None], ox[:, :, b_][:, None, :]].transpose(1, 2, 3, 0), 0.0)
                for m in range(2):
                    out[m] += wt[m][b, ch, cy[:, :, a_][:, :, None], cx[:, :, b_][:, None, :]][..., None] * W
    return out


def scores_cpu(gains: np.ndarray, stem_bits: np.ndarray, unknown: np.ndarray, bn_scale: np.ndarray, Wsum: np.ndarray) -> np.ndarray:
    """Pixel scores float64 ``[n, 2 modes, 32, 32, 3]``.  The push of stem bit s is ``wt_s = -g_s (bit_s == 0 ? +1 : -1)
    sign(bn_scale[ch])``: in mode 0 for the unknown bits with ``g_s < 0`` (zero elsewhere), in mode 1 for every unknown bit.
    The scores are ``scores_rect`` of the whole image."""
    sgn = np.where(np.asarray(stem_bits) == 0, 1.0, -1.0) * np.where(bn_scale >= 0, 1.0, -1.0)[None, :, None, None]
    wt1 = np.where(np.asarray(unknown).astype(bool), -gains * sgn, 0.0)
    zero = np.zeros(gains.shape[0], dtype=np.int64)
    return np.ascontiguousarray(scores_rect((np.where(gains < 0, wt1, 0.0), wt1), Wsum, zero, zero, 32, 32).transpose(1, 0, 2, 3, 4))


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


# ---- patches: the falsifying side of certify.certify_patch_u8 (include/ttnet.h: ttnet_attack_patch_u8) ------------------------------

PATCH_RECORD = np.dtype([("m_pred", "<f8"), ("worst", "<i4"), ("round", "<u2"), ("unknown", "<u2")])   # 16 bytes: the entry's map
PATCH_MAP = np.dtype([("m_pred", "<f8"), ("worst", "<i4"), ("round", "<u2"), ("unknown", "<u2"), ("status", "<i4"), ("margin", "<f4")])
PATCH_ROW = np.dtype([("positions", "<i4"), ("falsified", "<i4"), ("predicted", "<i4"), ("pos_first", "<i4"), ("status", "<i4")])
FILL_BYTES = 3 * CF.PATCH_MAX * CF.PATCH_MAX             # a fill record: the patch row-major (y, x, channel), zeros behind it
PATCH_ROUNDS_MAX = 4
PREDICTED = 3                                            # a position's status: the search predicts a witness that no forward judged
CONFIRM = ("all", "best", "none")


def check_patch_attack(patch, stride, amp, rounds, min_margin, confirm="all"):
    """``(h, w, stride, amp, Py, Px, rounds)`` of a patch search, or ValueError."""
    h, w, stride, amp, py, px = CF.check_patch(patch, stride, amp)
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= rounds <= PATCH_ROUNDS_MAX:
        raise ValueError(f"rounds must be an integer in [1, {PATCH_ROUNDS_MAX}], got {rounds!r}")
    if math.isnan(min_margin):
        raise ValueError("min_margin is NaN")
    if confirm not in CONFIRM:
        raise ValueError(f"confirm must be one of {CONFIRM}, got {confirm!r}")
    return h, w, stride, amp, py, px, int(rounds)


def paste_cpu(x_u8: np.ndarray, patch, stride: int, fills: np.ndarray, tasks) -> np.ndarray:
    """What ``ttnet_patch_paste_u8`` writes: image ``tasks[k] // P`` of ``x_u8`` with fill ``tasks[k]`` of ``fills``
    (``[n, P, 192]``) pasted at position ``tasks[k] % P``; all zero for a task outside ``[0, n P)``."""
    h, w, stride, _, py, px = CF.check_patch(patch, stride, 1)
    x_u8, tasks = np.asarray(x_u8), np.asarray(tasks).astype(np.int64).reshape(-1)
    P, n = py * px, x_u8.shape[0]
    flat = np.asarray(fills).reshape(n * P, FILL_BYTES)
    out = np.zeros((tasks.size, 32, 32, 3), np.uint8)
    for k, t in enumerate(tasks):
        if 0 <= t < n * P:
            y0, x0 = (t % P) // px * stride, (t % P) % px * stride
            out[k] = x_u8[t // P]
            out[k, y0:y0 + h, x0:x0 + w] = flat[t, :3 * h * w].reshape(h, w, 3)
    return out


class PatchAttackResult:
    """What ``attack_patch_u8`` (or the twin) found.  ``map``: structured ``[n, Py, Px]`` of dtype ``PATCH_MAP`` -- ``m_pred``,
    ``worst``, ``round``, ``unknown`` as the entry wrote them, ``status`` (0 open, 2 falsified: a forward judged the witness,
    3 predicted but not forwarded) and ``margin`` (the confirmed float32 margin, NaN where no forward ran); ``rows``: ``PATCH_ROW``
    per image -- ``positions``, ``falsified``, ``predicted`` (positions of status 2 or 3), ``pos_first`` (the first falsified
    position, -1: none) and ``status`` (0 open, 1 wrong at x0, 2 falsified at some position); ``fills`` uint8 ``[n, P, 192]``
    (numpy, or the device tensor); ``near`` (the twin only): bool ``[n, P]``, positions where the best and the second-best distinct prediction
    of some round lay within the summation tolerance ``1e-9 sum|A|`` of each other."""

    def __init__(self, x0, patch, stride, amp, map_, rows, fills, near=None):
        self.x0, self.patch, self.stride, self.amp = x0, tuple(patch), int(stride), int(amp)
        self.map, self.rows, self.fills, self.near = map_, rows, fills, near

    def __len__(self):
        return self.rows.shape[0]

    def fills_numpy(self) -> np.ndarray:
        return self.fills if isinstance(self.fills, np.ndarray) else self.fills.cpu().numpy()

    def witness(self, i: int, p: int) -> np.ndarray:
        """Image i with the kept fill of position p pasted: uint8 numpy ``[32, 32, 3]``."""
        P = self.map.shape[1] * self.map.shape[2]
        if not (0 <= i < len(self) and 0 <= p < P):
            raise IndexError(f"image {i}, position {p} of {len(self)} x {P}")
        x = self.x0[i:i + 1]
        x = x if isinstance(x, np.ndarray) else x.cpu().numpy()
        f = self.fills[i:i + 1]
        f = f if isinstance(f, np.ndarray) else f.cpu().numpy()
        return paste_cpu(x, self.patch, self.stride, f, [p])[0]


def patch_rows_from_map(maps: np.ndarray, wrong: np.ndarray) -> np.ndarray:
    """The image records (``PATCH_ROW``) of position records ``[n, Py, Px]``; ``wrong``: bool ``[n]``, wrong at x0."""
    n = maps.shape[0]
    flat = maps.reshape(n, -1)
    rows = np.zeros(n, dtype=PATCH_ROW)
    rows["positions"] = flat.shape[1]
    fals = flat["status"] == FALSIFIED
    rows["falsified"] = fals.sum(axis=1)
    rows["predicted"] = (fals | (flat["status"] == PREDICTED)).sum(axis=1)
    rows["pos_first"] = np.where(fals.any(axis=1), fals.argmax(axis=1), -1)
    rows["status"] = np.where(np.asarray(wrong).astype(bool), WRONG, np.where(fals.any(axis=1), FALSIFIED, OPEN))
    return rows


def confirm_tasks(rec: np.ndarray, confirm: str, confirm_slack: float) -> np.ndarray:
    """The tasks (``image * P + position``) whose witness goes through the forward, from the entry's records ``[n, P]``: the kept
    fill differs from the clean bytes (``round > 0``: a kept candidate lowered the prediction, so it is no copy) and ``m_pred <
    confirm_slack``; ``"best"``: of those only each image's position of smallest ``m_pred`` (the first one)."""
    n, P = rec.shape
    want = (rec["round"] > 0) & (rec["m_pred"] < confirm_slack)
    if confirm == "none":
        want[:] = False
    elif confirm == "best":
        best = rec["m_pred"].argmin(axis=1)
        only = np.zeros_like(want)
        only[np.arange(n), best] = True
        want &= only
    return np.flatnonzero(want.reshape(-1))


HASH_SLOTS, HASH_STREAM = (3, 7), 11                     # the candidates of tau = 1/2 give their slots away; slot k hashes stream 11 + k


def hash_corner(pos, rnd: int, slot: int, byte) -> np.ndarray:
    """bool per byte ``byte`` of the patch at position ``pos``, round ``rnd`` and stream ``slot``: bit 16 of a 32-bit integer
    mix, the same on the device (csrc/attack.hip: hash_corner)."""
    m = np.uint64(0xFFFFFFFF)
    v = (np.asarray(pos).astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64((rnd * 8 + slot) * 0x85EBCA6B)
         + np.asarray(byte).astype(np.uint64) * np.uint64(0xC2B2AE35)) & m
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & m
    v ^= v >> np.uint64(12)
    v = (v * np.uint64(0x297A2D39)) & m
    v ^= v >> np.uint64(15)
    return ((v >> np.uint64(16)) & np.uint64(1)).astype(bool)


def _reached_rect(kind: int, r0, rn, q0, qn):
    """``reached_rect`` of csrc/certify_lookup.h on arrays: first row, rows, first column, columns of branch ``kind``."""
    r1, q1 = r0 + rn - 1, q0 + qn - 1
    if kind == 0:
        r0, r1, q1 = np.maximum(r0 - 1, 0), np.minimum(r1 + 1, POOL - 1), q1 + 1
    elif kind == 1:
        r1, q0, q1 = r1 + 1, np.maximum(q0 - 1, 0), np.minimum(q1 + 1, POOL - 1)
    return r0, r1 - r0 + 1, q0, q1 - q0 + 1


class _PatchTwin:
    """What the patch twin derives once per call: the head in the device's bytes, the tables as words, the summed kernels."""

    def __init__(self, state, tables, mean, std):
        self.state, self.tables, self.mean, self.std = state, tables, mean, std
        self.A = head_cpu(state)                                           # [10, F]: D_f in the device's bytes
        self.c0 = CF.effective_head(state)[1]
        self.words = _words(tables)
        self.T = _table_rows(self.words)
        self.Wsum = wsum_cpu(state)
        self.scale = fold_bn(state, "features.2")[0]
        self.slack = CF.stem_slack(state, mean, std)[None, :, None, None]
        self.a, self.off = CF._norm(mean, std)
        self.tol = 1e-9 * float(np.abs(self.A).sum())

    def gains(self, pad, pi, ch, y, x, c, j):
        """``gains_listed`` on the twin's head and tables, the old feature bits from the tables: float64 ``[B]``."""
        return gains_listed(self.A, self.T, pad, pi, ch, y, x, c, j)[0]

    def scores(self, wt, y0, x0, h, w):
        """``scores_rect`` on the twin's summed kernels: ``[2, B, h, w, 3]``."""
        return scores_rect(wt, self.Wsum, y0, x0, h, w)


def _patch_image_cpu(tw: _PatchTwin, x: np.ndarray, c: int, h, w, stride, amp, rounds, min_margin, chunk: int = 128):
    """The search of every position of one image: ``(records [P] PATCH_RECORD, fills [P, 192], near [P])``."""
    org = CF.patch_origins((h, w), stride)
    P = len(org)
    y0, x0 = org[:, 0].astype(np.int64), org[:, 1].astype(np.int64)
    rec = np.zeros(P, dtype=PATCH_RECORD)
    near = np.zeros(P, dtype=bool)
    clean_fill = np.stack([x[a:a + h, b:b + w] for a, b in org])            # [P, h, w, 3]
    fills = np.zeros((P, FILL_BYTES), np.uint8)
    fills[:, :3 * h * w] = clean_fill.reshape(P, -1)
    if not 0 <= c < 10:
        rec["m_pred"], rec["worst"] = -np.inf, -1
        return rec, fills, near
    st, tables = tw.state, tw.tables
    clean_lo, clean_hi = (v[0] for v in CF.stem_planes_cpu(st, x[None], 0.0, tw.mean, tw.std))
    ylo_c, yhi_c = (v[0].reshape(-1).astype(np.int64) for v in CF.block_planes_cpu(tables, clean_lo[None], clean_hi[None]))
    unk_c = (ylo_c != yhi_c).astype(np.int64)
    D = tw.A[c][None, :] - tw.A
    Dm = np.minimum(D, 0.0)
    S, U = D @ ylo_c.astype(np.float64), Dm @ unk_c.astype(np.float64)
    lb0 = tw.c0[c] - tw.c0 + (S + U)
    lb0[c] = np.inf
    m_clean, j_clean = float(lb0.min()), int(lb0.argmin())
    rec["m_pred"], rec["worst"] = m_clean, j_clean
    spans = np.array([(*CF.field_span(int(a), h), *CF.field_span(int(b), w)) for a, b in org]).reshape(P, 4)   # first row, rows, first column, columns
    in_span = np.zeros((P, POOL, POOL), dtype=bool)
    for p, (r0, rn, q0, qn) in enumerate(spans):
        in_span[p, r0:r0 + rn, q0:q0 + qn] = rn > 0 and qn > 0
    blo, bhi = CF._patch_stem_planes(st, x, clean_lo, clean_hi, h, w, stride, amp, tw.mean, tw.std)
    movable = (blo != bhi) & in_span[:, None]                                # [P, 64, 10, 10]
    del blo, bhi
    rec["unknown"] = ((clean_lo != clean_hi)[None] & in_span[:, None]).reshape(P, -1).sum(axis=1)   # round 0: the clean cells of the span
    active = movable.reshape(P, -1).any(axis=1) & (not m_clean < -min_margin)
    cur_lo = np.broadcast_to(clean_lo, (P,) + clean_lo.shape).copy()
    cur_un = np.broadcast_to((clean_lo != clean_hi).astype(np.uint8), (P,) + clean_lo.shape).copy()
    fill = clean_fill.copy()
    m_cur, j_cur = np.full(P, m_clean), np.full(P, j_clean)
    b0 = clean_fill.astype(np.int64)
    up, dn = np.minimum(255, b0 + amp).astype(np.uint8), np.maximum(0, b0 - amp).astype(np.uint8)
    bpad = np.zeros((33, 33, 3))                                             # row / column 0: the padding
    bpad[1:, 1:] = x.astype(np.float64)
    for r in range(1, rounds + 1):
        corners = h == 1 and w == 1 and r == 1
        for a0 in range(0, P, chunk):
            sel = a0 + np.flatnonzero(active[a0:a0 + chunk])
            if not sel.size:
                continue
            B = sel.size
            # ---- the eight candidates -----------------------------------------------------------------------------------------------
            cand = np.empty((B, N_CAND, h, w, 3), np.uint8)
            if corners:
                for k in range(N_CAND):
                    for ch in range(3):
                        cand[:, k, 0, 0, ch] = (up if (k >> ch) & 1 else dn)[sel, 0, 0, ch]
            else:
                bits = (cur_lo[sel] & (1 - cur_un[sel])).astype(np.int64)
                pad = np.pad(bits, ((0, 0), (0, 0), (1, 1), (1, 1)))
                pi, ch, yy, xx = np.nonzero(movable[sel])
                g = tw.gains(pad, pi, ch, yy, xx, c, j_cur[sel][pi])
                sgn = np.where(bits[pi, ch, yy, xx] == 0, 1.0, -1.0) * np.where(tw.scale[ch] >= 0, 1.0, -1.0)
                wt1 = -g * sgn
                wt = np.zeros((2, B, STEM_CH, POOL, POOL))
                wt[1][pi, ch, yy, xx] = wt1
                wt[0][pi, ch, yy, xx] = np.where(g < 0, wt1, 0.0)
                sc = tw.scores(wt, y0[sel], x0[sel], h, w)
                # the six score slots are candidates_cpu's: the scores masked to the patch, every other byte scores 0 and keeps x_cur
                full = np.zeros((B, 2, 32, 32, 3))
                xc = np.broadcast_to(x, (B, 32, 32, 3)).copy()
                for i, p in enumerate(sel):
                    full[i, :, y0[p]:y0[p] + h, x0[p]:x0[p] + w] = sc[:, i]
                    xc[i, y0[p]:y0[p] + h, x0[p]:x0[p] + w] = fill[p]
                whole = candidates_cpu(full, np.broadcast_to(x, xc.shape), xc, amp)
                for i, p in enumerate(sel):
                    cand[i] = whole[i, :, y0[p]:y0[p] + h, x0[p]:x0[p] + w]
                # Two slots (the tau = 1/2 ones) go to another proposal: the sign corner of mode 1 -- upper end where the score is
                # positive, lower end where it is negative, the current byte where it is zero -- with a hashed half of its bytes at
                # the opposite end.  It looks around the first-order optimum where no single flip is rewarded.
                s = sc[1]
                base = np.where(s > 0, up[sel], np.where(s < 0, dn[sel], fill[sel]))
                other = np.where(s > 0, dn[sel], np.where(s < 0, up[sel], fill[sel]))
                for k in HASH_SLOTS:
                    inv = hash_corner(sel[:, None], r, HASH_STREAM + k, np.arange(3 * h * w)[None, :]).reshape(B, h, w, 3)
                    cand[:, k] = np.where(inv, other, base)
            # ---- their predictions --------------------------------------------------------------------------------------------------
            sp = spans[sel]
            nr, nc = int(sp[:, 1].max()), int(sp[:, 3].max())
            fr, fq = np.minimum(sp[:, 0], POOL - nr), np.minimum(sp[:, 2], POOL - nc)
            rr = 3 * fr[:, None] + np.arange(3 * nr + 2)[None, :]           # padded rows of the window
            qq = 3 * fq[:, None] + np.arange(3 * nc + 2)[None, :]
            win = bpad[rr[:, :, None], qq[:, None, :]]                       # [B, wr, wq, 3]
            iy, ix = rr - 1 - y0[sel][:, None], qq - 1 - x0[sel][:, None]
            inside = ((iy >= 0) & (iy < h))[:, :, None] & ((ix >= 0) & (ix < w))[:, None, :]
            cw = cand[np.arange(B)[:, None, None, None], np.arange(N_CAND)[None, :, None, None],
                      np.clip(iy, 0, h - 1)[:, None, :, None], np.clip(ix, 0, w - 1)[:, None, None, :]]     # [B, 8, wr, wq, 3]
            v = np.where(inside[:, None, :, :, None], cw.astype(np.float64), win[:, None])
            padding = ((rr == 0)[:, :, None] | (qq == 0)[:, None, :])[:, None, :, :, None]
            xn = np.where(padding, 0.0, (v - tw.off) * tw.a).reshape((B * N_CAND,) + v.shape[2:]).transpose(0, 3, 1, 2)
            lo, hi = CF._stem_bounds_norm(st, xn, xn, 0)                     # [B * 8, 64, nr, nc]
            wlo = (lo - tw.slack >= 0).astype(np.uint8).reshape(B, N_CAND, STEM_CH, nr, nc)
            whi = (hi + tw.slack >= 0).astype(np.uint8).reshape(B, N_CAND, STEM_CH, nr, nc) | wlo
            c_lo = np.repeat(cur_lo[sel][:, None], N_CAND, axis=1)           # [B, 8, 64, 10, 10]
            c_un = np.repeat(cur_un[sel][:, None], N_CAND, axis=1)
            unknown = np.zeros((B, N_CAND), np.int64)
            for i, (r0, rn, q0, qn) in enumerate(sp):
                a_, b_ = r0 - fr[i], q0 - fq[i]
                l_, h_ = wlo[i, :, :, a_:a_ + rn, b_:b_ + qn], whi[i, :, :, a_:a_ + rn, b_:b_ + qn]
                c_lo[i, :, :, r0:r0 + rn, q0:q0 + qn] = l_
                c_un[i, :, :, r0:r0 + rn, q0:q0 + qn] = l_ != h_
                unknown[i] = (l_ != h_).reshape(N_CAND, -1).sum(axis=1)
            Lp = np.pad(c_lo, ((0, 0), (0, 0), (0, 0), (1, 1), (1, 1)))
            Up = np.pad(c_un, ((0, 0), (0, 0), (0, 0), (1, 1), (1, 1)))
            bi = np.arange(B)[:, None, None, None, None]
            ki = np.arange(N_CAND)[None, :, None, None, None]
            chi = np.arange(STEM_CH)[None, None, :, None, None]
            dS, dU = np.zeros((B * N_CAND, 10)), np.zeros((B * N_CAND, 10))
            for kind in range(4):
                R0, NR, Q0, NQ = _reached_rect(kind, sp[:, 0], sp[:, 1], sp[:, 2], sp[:, 3])
                mr, mq = int(NR.max()), int(NQ.max())
                oy = np.minimum(R0[:, None] + np.arange(mr)[None, :], 10 if kind == 1 else 9)
                ox = np.minimum(Q0[:, None] + np.arange(mq)[None, :], 10 if kind == 0 else 9)
                ok = ((np.arange(mr)[None, :] < NR[:, None])[:, :, None] & (np.arange(mq)[None, :] < NQ[:, None])[:, None, :])[:, None, None]
                oy5, ox5 = oy[:, None, None, :, None], ox[:, None, None, None, :]
                if kind < 2:
                    kw = (2, 3)[kind]
                    l_ = np.stack([Lp[bi, ki, chi, oy5 + q // kw, ox5 + q % kw] for q in range(6)], axis=-1)
                    u_ = np.stack([Up[bi, ki, chi, oy5 + q // kw, ox5 + q % kw] for q in range(6)], axis=-1)
                    ylo, yhi = CF.lookup3(tw.T[kind].reshape(1, 1, STEM_CH, 1, 1, 1), l_ & (1 - u_), l_ | u_)
                elif kind == 2:
                    grp = (np.arange(STEM_CH) // 8 * 8)[None, None, :, None, None]
                    l_ = np.stack([Lp[bi, ki, grp + q, oy5 + 1, ox5 + 1] for q in range(8)], axis=-1)
                    u_ = np.stack([Up[bi, ki, grp + q, oy5 + 1, ox5 + 1] for q in range(8)], axis=-1)
                    ylo, yhi = CF.lookup3(tw.T[2].reshape(1, 1, STEM_CH, 1, 1, 4), l_ & (1 - u_), l_ | u_)
                else:
                    l_, u_ = Lp[bi, ki, chi, oy5 + 1, ox5 + 1], Up[bi, ki, chi, oy5 + 1, ox5 + 1]
                    ylo, yhi = l_ & (1 - u_), l_ | u_
                f = np.broadcast_to(((kind * 64 + chi) * SIDE + oy5) * SIDE + ox5, ylo.shape)
                dl = np.where(ok, ylo.astype(np.int64) - ylo_c[f], 0)
                du = np.where(ok, (ylo != yhi).astype(np.int64) - unk_c[f], 0)
                b_, k_, *_ = nz = np.nonzero((dl != 0) | (du != 0))
                row, fz = b_ * N_CAND + k_, f[nz]
                for j in range(10):
                    dS[:, j] += np.bincount(row, weights=D[j, fz] * dl[nz], minlength=B * N_CAND)
                    dU[:, j] += np.bincount(row, weights=Dm[j, fz] * du[nz], minlength=B * N_CAND)
            lb = tw.c0[c] - tw.c0 + ((S + dS) + (U + dU))
            lb[:, c] = np.inf
            m = lb.min(axis=1).reshape(B, N_CAND)
            jw = lb.argmin(axis=1).reshape(B, N_CAND)
            # ---- the smallest prediction wins (ties: the lowest index) and replaces the state if strictly below it --------------------
            kb = m.argmin(axis=1)
            mb = m[np.arange(B), kb]
            for i in range(B):
                u_ = np.unique(m[i])                                         # the best and the second-best distinct prediction
                if u_.size > 1 and u_[1] - u_[0] <= tw.tol:
                    near[sel[i]] = True
            better = mb < m_cur[sel]
            ps, ib = sel[better], np.flatnonzero(better)
            cur_lo[ps], cur_un[ps] = c_lo[ib, kb[ib]], c_un[ib, kb[ib]]
            fill[ps] = cand[ib, kb[ib]]
            m_cur[ps], j_cur[ps] = mb[ib], jw[ib, kb[ib]]
            rec["round"][ps], rec["unknown"][ps] = r, unknown[ib, kb[ib]]
            active[sel] = ~(m_cur[sel] < -min_margin)                        # (a round that kept its state still gets new hashed corners)
    rec["m_pred"], rec["worst"] = m_cur, j_cur
    fills[:, :3 * h * w] = fill.reshape(P, -1)
    return rec, fills, near


def attack_patch_cpu(state, tables, x_u8, classes, patch=(1, 1), stride: int = 1, amp: int = 255, rounds: int = 2,
                     min_margin: float = 0.0, *, forward: Callable, mean=CIFAR_MEAN, std=CIFAR_STD, confirm: str = "all",
                     confirm_slack: float = 1e-5) -> PatchAttackResult:
    """The numpy float64 twin of ``attack_patch_u8``: the gains, scores and candidates in the device's order and bytes (the sums of
    ``gains_cpu`` / ``scores_cpu`` / ``candidates_cpu`` with ``unknown`` := the position's box planes and the scores kept for the
    bytes of the patch only), ``m_pred`` as ``certify_box_cpu`` defines ``lb_interval`` for the degenerate box of the pasted image,
    summed in numpy's order.  ``forward(x_u8) -> (stem bits, feature bits, logits)`` judges the witnesses, as in ``attack_cpu``."""
    h, w, stride, amp, py, px, rounds = check_patch_attack(patch, stride, amp, rounds, min_margin, confirm)
    x0 = np.asarray(x_u8)
    n = x0.shape[0] if x0.ndim else 0
    classes = np.asarray(classes).astype(np.int64).reshape(-1)
    if x0.dtype != np.uint8 or x0.shape[1:] != (32, 32, 3) or classes.size != n:
        raise ValueError(f"expected uint8 images [n, 32, 32, 3] and n classes, got {x0.dtype} {x0.shape}, {classes.size}")
    tw = _PatchTwin(state, tables, mean, std)
    P = py * px
    rec, fills, near = np.zeros((n, P), PATCH_RECORD), np.zeros((n, P, FILL_BYTES), np.uint8), np.zeros((n, P), bool)
    for i in range(n):
        rec[i], fills[i], near[i] = _patch_image_cpu(tw, x0[i], int(classes[i]), h, w, stride, amp, rounds, min_margin)

    def judge(images, cls):
        rows, xcur, worst, active = new_state(len(images))
        select_cpu(images[:, None], forward(images)[2], 1, cls, min_margin, images, xcur, rows, worst, active, 0)
        return rows
    wrong = judge(x0, classes)["status"] == WRONG if n else np.zeros(0, bool)
    return _patch_result(x0, (h, w), stride, amp, rec.reshape(n, py, px), fills, wrong, confirm, confirm_slack,
                         lambda tasks: judge(paste_cpu(x0, (h, w), stride, fills, tasks), classes[tasks // P]), near)


def _patch_result(x0, patch, stride, amp, rec, fills, wrong, confirm, confirm_slack, judge, near=None) -> PatchAttackResult:
    """The entry's records ``[n, Py, Px]`` and the forward's verdicts (``judge(tasks)`` -> select records) as a result."""
    n, py, px = rec.shape
    maps = np.zeros((n, py * px), dtype=PATCH_MAP)
    for k in PATCH_RECORD.names:
        maps[k] = rec.reshape(n, -1)[k]
    maps["margin"] = np.nan
    flat = maps.reshape(-1)
    pred = (flat["round"] > 0) & (flat["m_pred"] < confirm_slack)
    flat["status"][pred] = PREDICTED
    tasks = confirm_tasks(rec.reshape(n, -1), confirm, confirm_slack)
    if tasks.size:
        rows = judge(tasks)
        flat["margin"][tasks] = rows["margin0"]
        flat["status"][tasks] = np.where(rows["status"] == WRONG, FALSIFIED, OPEN)
    maps = maps.reshape(n, py, px)
    return PatchAttackResult(x0, patch, stride, amp, maps, patch_rows_from_map(maps, wrong), fills, near)


# ---- patches on the device ---------------------------------------------------------------------------------------------------

def patch_search_u8(model, x_u8, classes, patch=(1, 1), stride: int = 1, amp: int = 255, rounds: int = 2, min_margin: float = 0.0,
                    lane: int = 0):
    """One ``ttnet_attack_patch_u8`` call on at most ``max_batch`` images: ``(records, fills)`` on the device -- float64
    ``[n, P, 2]`` holding the 16-byte records (``.cpu().numpy().view(PATCH_RECORD)``) and uint8 ``[n, P, 192]``.  Predictions
    only: no forward has judged them.  Asynchronous on the current stream."""
    import torch

    from . import _lib
    x_u8, classes = CF.checked_inputs(model, x_u8, classes, "attack_patch_u8", "the search needs the certificate's stem planes,")
    h, w, stride, amp, py, px, rounds = check_patch_attack(patch, stride, amp, rounds, min_margin)
    n = x_u8.shape[0]
    plan = model._plan_for(x_u8.device, n)
    rec = torch.empty((n, py * px, 2), dtype=torch.float64, device=x_u8.device)
    fills = torch.empty((n, py * px, FILL_BYTES), dtype=torch.uint8, device=x_u8.device)
    stream = torch.cuda.current_stream(x_u8.device).cuda_stream
    _lib.check(plan.lib.ttnet_attack_patch_u8(plan.handle, int(lane), C.c_void_p(x_u8.data_ptr()), n, C.c_void_p(classes.data_ptr()), h, w,
                                              stride, amp, rounds, float(min_margin), C.c_void_p(rec.data_ptr()),
                                              C.c_void_p(fills.data_ptr()), C.c_void_p(stream)))
    return rec, fills


def paste_u8(model, x_u8, patch, stride: int, fills, tasks):
    """``ttnet_patch_paste_u8``: uint8 ``[m, 32, 32, 3]``, image ``tasks[k] // P`` of ``x_u8`` with fill ``tasks[k]`` pasted."""
    import torch

    from . import _lib
    h, w, stride, _, py, px = CF.check_patch(patch, stride, 1)
    n, m = x_u8.shape[0], int(tasks.shape[0])
    tasks = tasks.to(device=x_u8.device, dtype=torch.int64).contiguous()
    plan = model._plan_for(x_u8.device, n)
    out = torch.empty((m, 32, 32, 3), dtype=torch.uint8, device=x_u8.device)
    stream = torch.cuda.current_stream(x_u8.device).cuda_stream
    _lib.check(plan.lib.ttnet_patch_paste_u8(plan.handle, C.c_void_p(x_u8.data_ptr()), n, h, w, stride, C.c_void_p(fills.data_ptr()),
                                             C.c_void_p(tasks.data_ptr()), m, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out


def _judge_u8(model, images, classes, min_margin: float, lane: int) -> np.ndarray:
    """The select records (``RECORD``) of round 0 for ``images`` (at most ``FORWARD_ROWS``) through one ``forward_u8``: ``status == 1``
    means ``margin0 < -min_margin``."""
    import torch
    m, dev = images.shape[0], images.device
    plan = model._plan_for(dev, m)
    stream = torch.cuda.current_stream(dev).cuda_stream
    logits = torch.empty((m, 10), dtype=torch.float32, device=dev)
    rows = torch.empty((m, 8), dtype=torch.int32, device=dev)
    xcur = torch.empty_like(images)
    worst = torch.empty(m, dtype=torch.int32, device=dev)
    active = torch.empty(m, dtype=torch.int32, device=dev)
    _forward_into(plan, lane, images, logits, stream)
    select_u8(model, images, logits, m, 1, classes, min_margin, images, xcur, rows, worst, active, 0)
    return rows.cpu().numpy().view(RECORD).reshape(-1)


def attack_patch_u8(model, x_u8, classes, patch=(1, 1), stride: int = 1, amp: int = 255, rounds: int = 2, min_margin: float = 0.0,
                    confirm: str = "all", confirm_slack: float = 1e-5, lane: int = 0) -> PatchAttackResult:
    """For every position of ``certify_patch_u8`` (the same positions, ``stride`` and ``amp``) search a uint8 fill of the patch on
    which image i of ``x_u8`` (uint8 HIP tensor ``[N, 32, 32, 3]``) loses ``classes[i]``.  The device predicts (``m_pred``), the
    forward alone confirms: the positions whose kept fill differs from the clean bytes and whose ``m_pred < confirm_slack`` (the
    default is the logit tolerance, so near ties get their forward) are pasted, forwarded in chunks of at most ``FORWARD_ROWS``
    and judged by ``ttnet_attack_select_u8``; ``status == 2`` there means ``margin < -min_margin``.  ``confirm="best"`` forwards
    only each image's position of smallest ``m_pred`` (enough for the accuracy bracket), ``"none"`` nothing.  More than
    ``FORWARD_ROWS`` images are searched in parts of that size.  Synchronises: the records come back to choose the forwards."""
    import torch
    x0, classes = CF.checked_inputs(model, x_u8, classes, "attack_patch_u8", "the search needs the certificate's stem planes,")
    h, w, stride, amp, py, px, rounds = check_patch_attack(patch, stride, amp, rounds, min_margin, confirm)
    n, P = x0.shape[0], py * px
    parts = [(a, min(n, a + FORWARD_ROWS)) for a in range(0, n, FORWARD_ROWS)]
    found = [patch_search_u8(model, x0[a:b], classes[a:b], (h, w), stride, amp, rounds, min_margin, lane) for a, b in parts]
    rec = (np.concatenate([r.cpu().numpy().view(PATCH_RECORD).reshape(-1, P) for r, _ in found]) if found
           else np.zeros((0, P), PATCH_RECORD))
    fills = torch.cat([f for _, f in found]) if found else torch.empty((0, P, FILL_BYTES), dtype=torch.uint8, device=x0.device)
    wrong = np.concatenate([_judge_u8(model, x0[a:b], classes[a:b], min_margin, lane)["status"] == WRONG for a, b in parts] or
                           [np.zeros(0, bool)])

    def judge(tasks: np.ndarray) -> np.ndarray:
        out = []
        for a, b in parts:                                              # (tasks ascend: the parts' answers follow each other)
            local = tasks[(tasks >= a * P) & (tasks < b * P)] - a * P
            chunk = min(model._plan_for(x0.device, b - a).max_batch, FORWARD_ROWS)
            for k in range(0, local.size, chunk):
                t = torch.from_numpy(local[k:k + chunk]).to(x0.device)
                images = paste_u8(model, x0[a:b], (h, w), stride, fills[a:b], t)
                out.append(_judge_u8(model, images, classes[a:b][t // P], min_margin, lane))
        return np.concatenate(out)
    return _patch_result(x0, (h, w), stride, amp, rec.reshape(n, py, px), fills, wrong, confirm, confirm_slack, judge)


def kept_fills(res: PatchAttackResult) -> Tuple[np.ndarray, np.ndarray]:
    """``(tasks, fills)`` of the positions a result would ever write out -- status falsified or predicted --: int64 ``[k]``
    (``image * P + position``) and uint8 ``[k, 3 h w]``, the meaningful bytes of their fill records."""
    h, w = res.patch
    tasks = np.flatnonzero(res.map.reshape(-1)["status"] > 0)
    flat = res.fills.reshape(-1, FILL_BYTES)
    if isinstance(flat, np.ndarray):
        return tasks, flat[tasks, :3 * h * w].copy()
    import torch
    return tasks, flat[torch.from_numpy(tasks).to(flat.device)][:, :3 * h * w].cpu().numpy()


def _summary(patch, stride, amp, rounds, m, rows, tasks, fills) -> dict:
    return {"patch": tuple(patch), "stride": int(stride), "amp": int(amp), "images": int(rows.size), "wrong": int((rows["status"] == WRONG).sum()),
            "search": int((rows["status"] == FALSIFIED).sum()), "falsified": int((rows["status"] > 0).sum()),
            "positions": int(m.size), "positions_falsified": int((m["status"] == FALSIFIED).sum()),
            "positions_predicted": int((m["status"] == PREDICTED).sum()), "rounds": int(rounds), "rows": rows, "map": m,
            "fill_tasks": tasks, "fills": fills}


def summarise_patch(res: PatchAttackResult, rounds: int) -> dict:
    """What ``attack_patch_batches`` reports per patch size: counts, ``rows``, ``map``, and the fills of the falsified and predicted
    positions alone (``fill_tasks``, ``fills``: ``kept_fills``)."""
    return _summary(res.patch, res.stride, res.amp, rounds, res.map, res.rows, *kept_fills(res))


def attack_patch_batches(model, batches: Iterable, patches: Sequence, stride: int = 1, amp: int = 255, rounds: int = 2,
                         min_margin: float = 0.0, confirm: str = "all", confirm_slack: float = 1e-5, lane: int = 0) -> List[dict]:
    """``attack_patch_u8`` on the targets of ``batches`` (``cifar.device_batches``) for every patch size of ``patches``: one dict
    per size (``summarise_patch``) with ``rows`` and ``map`` in dataset order.  Of a batch's fill records only the bytes of the
    falsified and predicted positions are kept; the records themselves go with the batch."""
    patches = [tuple(p) for p in patches]
    parts: List[List[tuple]] = [[] for _ in patches]
    seen = 0
    for x, t in batches:
        for i, p in enumerate(patches):
            res = attack_patch_u8(model, x, t, p, stride, amp, rounds, min_margin, confirm, confirm_slack, lane)
            tasks, fills = kept_fills(res)
            parts[i].append((res.map, res.rows, tasks + seen * res.map.shape[1] * res.map.shape[2], fills))
        seen += int(x.shape[0])
    out = []
    for p, res in zip(patches, parts):
        h, w, _, _, py, px = CF.check_patch(p, stride, amp)
        cat = lambda k, empty: np.concatenate([r[k] for r in res]) if res else empty  # noqa: E731
        out.append(_summary((h, w), stride, amp, rounds, cat(0, np.zeros((0, py, px), PATCH_MAP)), cat(1, np.zeros(0, PATCH_ROW)),
                            cat(2, np.zeros(0, np.int64)), cat(3, np.zeros((0, 3 * h * w), np.uint8))))
    return out


def patch_robust_bounds(certify_summary: dict, attack_summary: dict) -> dict:
    """The patch bracket of the same images from ``certify.certify_patch_batches``' and ``attack_patch_batches``' summaries of one
    size: ``certified, falsified, open`` images and ``positions_certified, positions_falsified, positions_open``.  A position that
    is both certified (stage > 0) and falsified, or an image that is both, is a bug in one of the two: ``ValueError`` names the
    first."""
    cm, am = np.asarray(certify_summary["map"]), np.asarray(attack_summary["map"])
    if cm.shape != am.shape:
        raise ValueError(f"certificates {cm.shape} for attack records {am.shape}")
    cert, fals = cm["stage"] > 0, am["status"] == FALSIFIED
    both = np.argwhere(cert & fals)
    if both.size:
        raise ValueError(f"image {int(both[0][0])}, position {tuple(int(v) for v in both[0][1:])} is both certified and falsified "
                         f"({len(both)} such positions): a bug in the certificate or in the search")
    crow, arow = certify_summary["rows"], attack_summary["rows"]
    icert, ifals = np.asarray(crow["certified"] == crow["positions"]), np.asarray(arow["status"]) > 0
    ib = np.flatnonzero(icert & ifals)
    if ib.size:
        raise ValueError(f"image {int(ib[0])} is both patch-certified and falsified ({ib.size} such images): a bug in the certificate "
                         "or in the search")
    return {"images": int(icert.size), "certified": int(icert.sum()), "falsified": int(ifals.sum()),
            "open": int(icert.size - icert.sum() - ifals.sum()), "wrong": int((arow["status"] == WRONG).sum()),
            "positions_certified": int(cert.sum()), "positions_falsified": int(fals.sum()),
            "positions_open": int(cert.size - cert.sum() - fals.sum())}


def patch_robust_line(certify_summary: dict, attack_summary: dict) -> str:
    """``PatchRobust.. size=HxW amp=A stride=S certified a/N <= robust <= b/N (falsified f: wrong at x0 w, by search s; open o;
    positions certified p, falsified q, open r)``"""
    b, s = patch_robust_bounds(certify_summary, attack_summary), attack_summary
    n, f = b["images"], b["falsified"]
    return (f"PatchRobust.. size={s['patch'][0]}x{s['patch'][1]} amp={s['amp']} stride={s['stride']} certified {b['certified']}/{n} <= robust "
            f"<= {n - f}/{n} (falsified {f}: wrong at x0 {b['wrong']}, by search {f - b['wrong']}; open {b['open']}; positions certified "
            f"{b['positions_certified']}, falsified {b['positions_falsified']}, open {b['positions_open']})")


def write_patch_witnesses_npz(path: str, summaries: Sequence[dict]):
    """The falsified positions as .npz: per size ``tasks_HxW`` int64 (``image * P + position``), ``fills_HxW`` uint8 ``[k, 3 h w]``,
    ``margin_HxW`` float32 (the forward's), ``m_pred_HxW`` float64 and ``geometry_HxW`` int64 ``(h, w, stride, amp, Py, Px)``; a
    witness is image ``task // P`` with the fill pasted at position ``task % P`` (``paste_cpu``).  Written to a temporary name and
    renamed."""
    from .report import replacing
    arrays = {}
    for s in summaries:
        h, w = s["patch"]
        key = f"{h}x{w}"
        m = s["map"]
        flat = m.reshape(-1)
        tasks = np.flatnonzero(flat["status"] == FALSIFIED)
        arrays.update({f"tasks_{key}": tasks.astype(np.int64),
                       f"fills_{key}": s["fills"][np.searchsorted(s["fill_tasks"], tasks)],
                       f"margin_{key}": flat["margin"][tasks], f"m_pred_{key}": flat["m_pred"][tasks],
                       f"geometry_{key}": np.array([h, w, s["stride"], s["amp"], m.shape[1], m.shape[2]], dtype=np.int64)})
    with replacing(path, "wb") as f:
        np.savez(f, **arrays)
