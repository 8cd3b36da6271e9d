"""Certified L-infinity robustness of ``TT_FHE_XSMALL_vAlexnet``: does an image keep its class when every input byte may
move by up to ``eps`` byte levels?  (include/ttnet.h: ttnet_certify_u8; DESIGN.md: certified robustness.)

The network makes the question cheap to answer soundly: the stem (conv + bias, ReLU, BatchNorm, MaxPool, ``x >= 0``) is
monotone, so a box of inputs becomes three-valued stem bits by interval arithmetic (stage 0); the block is three small
truth tables, through which unknown bits go exactly per lookup; and the head ``lin2(BN(lin1(.)))`` is affine in the
feature bits, so a lower bound on every logit difference is a signed sum (stage 1).  Images left open with few unknown
stem bits are settled by enumerating the completions of those bits (stage 2).  Sound, not complete.

``certify_u8`` / ``certify_batches`` run on the device (csrc/certify.hip).  ``certify_cpu`` is the numpy float64 twin of all
three stages: the same slack, the same definitions, the same record.  It takes the truth tables as an argument
(``model.get_table``, canonical order), since the package builds tables on the device only.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .cifar import CIFAR_MEAN, CIFAR_STD
from .valexnet_block import (FEAT_ROWS, N_CLASSES, N_FEAT, N_REACH, PADS, STEM_ROWS, WINDOW_SIZE, block_windows,  # noqa: F401
                             block_words, f64, fold_bn, reach, table_words, window_input, zpad)   # (some only re-exported)

RECORD = np.dtype([("lb_interval", "<f8"), ("lb", "<f8"), ("worst", "<i4"), ("stage", "<i4"), ("unknown_stem", "<i4"),
                   ("unknown_feat", "<i4")])                # the 32-byte record of ttnet_certify_u8
ENUM_BITS_MAX = 12
ROWS_HEADER = ["index", "class", "stage", "certified", "lb", "lb_interval", "worst", "unknown_stem", "unknown_feat"]


# ---- the device path ---------------------------------------------------------------------------------------------------

class CertifyResult:
    """The records of one ``certify_u8`` call, on the device: ``rows`` is float64 ``[n, 4]`` holding the n 32-byte records;
    ``lb_interval``, ``lb`` (float64) and ``worst``, ``stage``, ``unknown_stem``, ``unknown_feat`` (int32) are views of it.
    ``planes`` (``return_planes=True``): ``{"stem_lo", "stem_hi"}`` int64 ``[n, 64, 10]`` and ``{"feat_lo", "feat_hi"}``
    int64 ``[n, 256, 11]`` row-packed words (the layouts of ``read_stage("features.4")`` / ``("features.5")``)."""

    def __init__(self, rows, planes=None):
        import torch
        self.rows = rows
        self.planes = planes
        ints = rows.view(torch.int32)
        self.lb_interval, self.lb = rows[:, 0], rows[:, 1]
        self.worst, self.stage, self.unknown_stem, self.unknown_feat = (ints[:, 4 + k] for k in range(4))

    def __len__(self):
        return self.rows.shape[0]

    @property
    def certified(self):
        return self.stage > 0

    def numpy(self) -> np.ndarray:
        """The records as a structured array of dtype ``RECORD`` (synchronises)."""
        return self.rows.cpu().numpy().view(RECORD).reshape(-1)

    def planes_numpy(self) -> Dict[str, np.ndarray]:
        return {k: v.cpu().numpy().view(np.uint64) for k, v in (self.planes or {}).items()}


def checked_inputs(model, x_u8, classes, who: str, needs: str):
    """What ``certify_u8`` and ``attack_u8`` check first: the variant, eval mode, the image tensor and the classes.  Returns
    the images contiguous and 4-byte aligned and the classes as an int32 tensor on their device."""
    import torch
    if getattr(model, "VARIANT", None) != "valexnet":
        raise RuntimeError(f"{who} serves TT_FHE_XSMALL_vAlexnet only: {needs} an affine head and truth tables of at most 8 inputs")
    if model.training:
        raise RuntimeError("the HIP path implements eval-mode inference only: call model.eval()")
    if (not x_u8.is_cuda) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or tuple(x_u8.shape[1:]) != (32, 32, 3):
        raise RuntimeError(f"expected a uint8 HIP tensor [N,32,32,3], got {x_u8.dtype} {tuple(x_u8.shape)} on {x_u8.device}")
    n = x_u8.shape[0]
    classes = torch.as_tensor(classes)
    if classes.dim() != 1 or classes.shape[0] != n or classes.dtype.is_floating_point or classes.dtype == torch.bool:
        raise RuntimeError(f"expected {n} integer classes, got {classes.dtype} {tuple(classes.shape)}")
    x_u8 = x_u8.contiguous()
    if x_u8.data_ptr() % 4:
        x_u8 = x_u8.clone()
    return x_u8, classes.to(device=x_u8.device, dtype=torch.int32).contiguous()


def certify_u8(model, x_u8, classes, eps: float, enum_bits: int = 10, min_margin: float = 1e-6, lane: int = 0,
               return_planes: bool = False) -> CertifyResult:
    """Certify that image i of ``x_u8`` (uint8 HIP tensor ``[N, 32, 32, 3]``, what ``forward_u8`` takes) keeps the class
    ``classes[i]`` when every byte moves by up to ``eps`` byte levels (``eps=2`` is 2/255).  ``classes``: an integer tensor
    ``[N]``; a class outside 0..9 is not an error, that image's record says stage 0 and ``lb = -inf`` (nothing is read back
    from the device to check it).  Asynchronous on the current stream.  No graph capture."""
    import torch

    from . import _lib
    x_u8, classes = checked_inputs(model, x_u8, classes, "certify_u8", "the certificate needs")
    n = x_u8.shape[0]
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    if not 0 <= int(enum_bits) <= ENUM_BITS_MAX:
        raise ValueError(f"enum_bits must be in [0, {ENUM_BITS_MAX}], got {enum_bits}")
    plan = model._plan_for(x_u8.device, n)
    rows = torch.empty((n, 4), dtype=torch.float64, device=x_u8.device)
    words = torch.empty(n * 2 * (STEM_ROWS + FEAT_ROWS) if return_planes else 0, dtype=torch.int64, device=x_u8.device)
    stream = torch.cuda.current_stream(x_u8.device).cuda_stream
    _lib.check(plan.lib.ttnet_certify_u8(plan.handle, int(lane), C.c_void_p(x_u8.data_ptr()), n, C.c_void_p(classes.data_ptr()),
                                         float(eps), int(enum_bits), float(min_margin), C.c_void_p(rows.data_ptr()),
                                         C.c_void_p(words.data_ptr() if return_planes else None), C.c_void_p(stream)))
    planes = None
    if return_planes:
        a, b = n * STEM_ROWS, n * FEAT_ROWS
        planes = {"stem_lo": words[:a].view(n, 64, 10), "stem_hi": words[a:2 * a].view(n, 64, 10),
                  "feat_lo": words[2 * a:2 * a + b].view(n, 256, 11), "feat_hi": words[2 * a + b:].view(n, 256, 11)}
    return CertifyResult(rows, planes)


def summarise(eps: float, rows: np.ndarray) -> dict:
    """What ``certify_batches`` reports per eps, from the records of all images."""
    k = rows["unknown_stem"]
    return {"eps": float(eps), "images": int(rows.size), "certified": int((rows["stage"] > 0).sum()),
            "interval": int((rows["stage"] == 1).sum()), "enumeration": int((rows["stage"] == 2).sum()),
            "unknown_stem_median": float(np.median(k)) if rows.size else 0.0, "unknown_stem_max": int(k.max()) if rows.size else 0,
            "rows": rows}


def certify_batches(model, batches: Iterable, eps_list: Sequence[float], enum_bits: int = 10, min_margin: float = 1e-6,
                    lane: int = 0) -> List[dict]:
    """Certify the targets of ``batches`` (pairs ``(uint8 images, int64 targets)`` on the device: ``cifar.device_batches``)
    at every eps of ``eps_list``.  One dict per eps: ``eps, images, certified, interval, enumeration`` (counts by stage),
    ``unknown_stem_median, unknown_stem_max`` and ``rows``, the records in dataset order (dtype ``RECORD``).  Certifying the
    labels makes ``certified / images`` the verified accuracy.  The records stay on the device until the last batch."""
    import torch
    eps_list = [float(e) for e in eps_list]
    parts: List[List] = [[] for _ in eps_list]
    for x, t in batches:
        for i, eps in enumerate(eps_list):
            parts[i].append(certify_u8(model, x, t, eps, enum_bits, min_margin, lane).rows)
    out = []
    for eps, p in zip(eps_list, parts):
        rows = torch.cat(p).cpu().numpy().view(RECORD).reshape(-1) if p else np.zeros(0, dtype=RECORD)
        out.append(summarise(eps, rows))
    return out


def verified_line(s: dict) -> str:
    """``Verified.. eps=E certified/N pct (interval a, enumeration b; unknown stem bits median u max v)``"""
    pct = 100.0 * s["certified"] / max(1, s["images"])
    return (f"Verified.. eps={s['eps']:g} {s['certified']}/{s['images']} {pct:.2f} (interval {s['interval']}, enumeration "
            f"{s['enumeration']}; unknown stem bits median {s['unknown_stem_median']:g} max {s['unknown_stem_max']})")


def rows_csv_rows(summaries: Sequence[dict], classes: Sequence[int]) -> List[list]:
    """Header first, then one row per (eps, image): eps, then the columns of ``ROWS_HEADER``.  Floats are written with
    ``repr`` (round-trip exact)."""
    out = [["eps"] + ROWS_HEADER]
    for s in summaries:
        if len(classes) != s["rows"].size:
            raise ValueError(f"{len(classes)} classes for {s['rows'].size} records")
        for i, (r, c) in enumerate(zip(s["rows"], classes)):
            out.append([repr(float(s["eps"])), i, int(c), int(r["stage"]), int(r["stage"] > 0), repr(float(r["lb"])),
                        repr(float(r["lb_interval"])), int(r["worst"]), int(r["unknown_stem"]), int(r["unknown_feat"])])
    return out


def write_rows_csv(path: Optional[str], summaries: Sequence[dict], classes: Sequence[int]):
    """The records of ``certify_batches`` as CSV (``path`` None: standard output); written to a temporary name and renamed."""
    from .report import write_csv
    write_csv(path, rows_csv_rows(summaries, classes))


# ---- the numpy float64 twin ----------------------------------------------------------------------------------------------

def _norm(mean, std) -> Tuple[np.ndarray, np.ndarray]:
    """(a, off): the normalised value of byte level v of channel c is (v - off[c]) * a[c]; the constants are float32, as the
    plan holds them."""
    mean, std = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (mean, std))
    return 1.0 / (255.0 * std), 255.0 * mean


def stem_slack(state, mean=CIFAR_MEAN, std=CIFAR_STD) -> np.ndarray:
    """The outward widening of the stem bounds, per channel (include/ttnet.h)."""
    a, off = _norm(mean, std)
    X = max(np.abs((0.0 - off) * a).max(), np.abs((255.0 - off) * a).max())
    scale, shift = fold_bn(state, "features.2")
    l1 = np.abs(f64(state["features.0.weight"])).reshape(64, -1).sum(axis=1)
    return np.ldexp((l1 * X + np.abs(f64(state["features.0.bias"]))) * np.abs(scale) + np.abs(shift), -40)


def stem_bounds_cpu(state, x_u8: np.ndarray, eps: float, mean=CIFAR_MEAN, std=CIFAR_STD) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 0 without the slack: float64 ``(lo, hi)`` ``[n, 64, 10, 10]`` of the pooled pre-activation over the box."""
    import torch
    import torch.nn.functional as F
    a, off = _norm(mean, std)
    b = np.asarray(x_u8).astype(np.float64).transpose(0, 3, 1, 2)                      # [n, 3, 32, 32]
    x_lo = (np.maximum(0.0, b - eps) - off[None, :, None, None]) * a[None, :, None, None]
    x_hi = (np.minimum(255.0, b + eps) - off[None, :, None, None]) * a[None, :, None, None]
    w = f64(state["features.0.weight"])
    wp, wn = torch.from_numpy(np.maximum(w, 0.0)), torch.from_numpy(np.minimum(w, 0.0))
    bias = torch.from_numpy(f64(state["features.0.bias"]))
    tl, th = torch.from_numpy(np.ascontiguousarray(x_lo)), torch.from_numpy(np.ascontiguousarray(x_hi))
    lo = F.relu(F.conv2d(tl, wp, bias, 1, 1) + F.conv2d(th, wn, None, 1, 1))          # zero padding: zero in normalised space
    hi = F.relu(F.conv2d(th, wp, bias, 1, 1) + F.conv2d(tl, wn, None, 1, 1))
    scale, shift = (torch.from_numpy(v)[None, :, None, None] for v in fold_bn(state, "features.2"))
    pos = scale >= 0
    ylo = torch.where(pos, lo, hi) * scale + shift                                     # a negative scale swaps the bounds
    yhi = torch.where(pos, hi, lo) * scale + shift
    return F.max_pool2d(ylo, 3).numpy(), F.max_pool2d(yhi, 3).numpy()


def stem_planes_cpu(state, x_u8, eps: float, mean=CIFAR_MEAN, std=CIFAR_STD) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 0: uint8 ``(lo_bit, hi_bit)`` ``[n, 64, 10, 10]``; unknown where they differ."""
    lo, hi = stem_bounds_cpu(state, x_u8, eps, mean, std)
    sl = stem_slack(state, mean, std)[None, :, None, None]
    lo_bit = (lo - sl >= 0).astype(np.uint8)
    return lo_bit, (hi + sl >= 0).astype(np.uint8) | lo_bit


_IDX_MASK = np.array([0xAAAAAAAAAAAAAAAA, 0xCCCCCCCCCCCCCCCC, 0xF0F0F0F0F0F0F0F0, 0xFF00FF00FF00FF00, 0xFFFF0000FFFF0000,
                      0xFFFFFFFF00000000], dtype=np.uint64)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def lookup3(words: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Three-valued lookup by selector words.  ``words`` ``[..., W]`` (W = 1 for n <= 6, 4 for n = 8), ``lo`` / ``hi``
    ``[..., n]`` bits (unknown where they differ).  Returns ``(ylo, yhi)``: certainly 1, possibly 1."""
    n = lo.shape[-1]
    lo, un = lo.astype(bool), lo != hi
    S = np.full(lo.shape[:-1], _ALL, dtype=np.uint64)
    for p in range(min(n, 6)):
        S &= np.where(un[..., p], _ALL, np.where(lo[..., p], _IDX_MASK[p], ~_IDX_MASK[p]))
    shape = np.broadcast_shapes(S.shape, words.shape[:-1])
    can0 = np.zeros(shape, dtype=bool)
    can1 = np.zeros(shape, dtype=bool)
    for w in range(words.shape[-1]):
        ok = np.ones(S.shape, dtype=bool)
        for p in range(6, n):                                                          # inputs 6, 7 pick the word
            ok &= un[..., p] | (lo[..., p] == bool((w >> (p - 6)) & 1))
        can1 |= ok & ((words[..., w] & S) != 0)
        can0 |= ok & ((~words[..., w] & S) != 0)
    return (~can0).astype(np.uint8), can1.astype(np.uint8)


def block_planes_cpu(tables, lo_bit: np.ndarray, hi_bit: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 1, the block: ``(ylo, yhi)`` uint8 ``[n, 256, 11, 11]`` from the stem planes; paddings are known zeros."""
    w1, w2, w3 = block_words(tables)                                                   # [64, 1, 1], [64, 1, 1], [8, 8, 4]
    wl, wh = block_windows(lo_bit), block_windows(hi_bit)
    outs = [lookup3(w[None, :, 0, None, None, :], wl[k], wh[k]) for k, w in enumerate((w1, w2))]
    l3, h3 = lookup3(w3[None, :, :, None, None, :], wl[2][:, :, None], wh[2][:, :, None])   # [n, g, o, y, x]
    outs.append((l3.reshape(lo_bit.shape), h3.reshape(lo_bit.shape)))
    outs.append((lo_bit, hi_bit))
    pads = (PADS[0], PADS[1], PADS[2], PADS[2])
    return tuple(np.concatenate([zpad(o[k], p) for o, p in zip(outs, pads)], axis=1) for k in (0, 1))


def effective_head(state) -> Tuple[np.ndarray, np.ndarray]:
    """``A = lin2 diag(bn_scale) lin1`` float64 ``[10, 30976]`` and ``c0 = lin2 bn_shift + bias``."""
    s, t = fold_bn(state, "features.7.BN2")
    l2 = f64(state["features.7.lin2.weight"])
    return (l2 * s[None, :]) @ f64(state["features.7.lin1.weight"]), l2 @ t + f64(state["features.7.lin2.bias"])


def margins_cpu(A, c0, ylo: np.ndarray, yhi: np.ndarray, c: int) -> np.ndarray:
    """``lb_j`` of one image (flattened feature planes) for every j; ``+inf`` at j = c."""
    D = A[c][None, :] - A
    lb = c0[c] - c0 + D @ ylo.astype(np.float64) + np.minimum(D, 0.0) @ (ylo != yhi).astype(np.float64)
    lb[c] = np.inf
    return lb


def _affected(lo_bit: np.ndarray, hi_bit: np.ndarray):
    """The unknown stem bits of one image in (channel, row, column) order and the features whose windows hold one, in the
    order the device lists them: per unknown bit conv1, conv2, conv3, out4, first mention wins.  A feature is
    ``(channel of the 256, oy, ox, [(input p, stem channel, y, x)])``; inputs that fall into the padding are left out."""
    unk = [tuple(int(v) for v in u) for u in np.argwhere(lo_bit != hi_bit)]
    seen, feats = set(), []
    for ch, y, x in unk:
        for t in range(N_REACH):
            valid, fc, oy, ox, _ = reach(ch, y, x, t)
            if not valid or (fc, oy, ox) in seen:
                continue
            seen.add((fc, oy, ox))
            inputs = [(p, window_input(fc // 64, fc % 64, oy, ox, p)) for p in range(WINDOW_SIZE[fc // 64])]
            feats.append((fc, oy, ox, [(p, *s) for p, s in inputs if s is not None]))
    return unk, feats


def enumerate_margins_cpu(A, c0, words, lo_bit: np.ndarray, hi_bit: np.ndarray, ylo: np.ndarray, c: int) -> np.ndarray:
    """Stage 2 for one image, per class: the minimum over all completions of the unknown stem bits of ``logit_c - logit_j``
    for every j (``+inf`` at j = c).  ``words`` = ``[table_words(conv1), (conv2), (conv3)]``; ``ylo`` ``[256, 11, 11]``."""
    unk, feats = _affected(lo_bit, hi_bit)
    k, ne = len(unk), len(feats)
    which = {u: i for i, u in enumerate(unk)}
    D = A[c][None, :] - A                                                              # [10, F]
    T = np.zeros((ne, 4), dtype=np.uint64)
    base = np.zeros(ne, dtype=np.int64)
    src = np.full((ne, 8), -1, dtype=np.int64)                                         # unknown index feeding input p
    f_idx = np.empty(ne, dtype=np.int64)
    for e, (fc, oy, ox, inputs) in enumerate(feats):
        kind, ch = fc // 64, fc % 64
        T[e, :1 if kind != 2 else 4] = (words[kind][ch, 0] if kind < 2 else words[2][ch // 8, ch % 8] if kind == 2
                                        else np.array([2], dtype=np.uint64))
        for p, sc, y, x in inputs:
            if (sc, y, x) in which:
                src[e, p] = which[(sc, y, x)]
            elif lo_bit[sc, y, x]:
                base[e] |= 1 << p
        f_idx[e] = fc * 121 + oy * 11 + ox
    keep = ylo.reshape(-1).astype(np.float64)
    keep[f_idx] = 0.0                                                                  # the re-evaluated features leave the base sum
    m0 = c0[c] - c0 + D @ keep
    a = np.arange(1 << k, dtype=np.int64)
    idx = np.broadcast_to(base[None, :], (a.size, ne)).copy()
    for p in range(8):
        sel = src[:, p] >= 0
        idx[:, sel] |= ((a[:, None] >> src[sel, p][None, :]) & 1) << p
    out = (T[np.arange(ne)[None, :], idx >> 6] >> (idx & 63).astype(np.uint64)) & np.uint64(1)
    m = m0[None, :] + out.astype(np.float64) @ D[:, f_idx].T                           # [2^k, 10]
    m[:, c] = np.inf
    return m.min(axis=0)


def enumerate_cpu(A, c0, words, lo_bit: np.ndarray, hi_bit: np.ndarray, ylo: np.ndarray, c: int) -> Tuple[float, int]:
    """Stage 2 for one image: the smallest of ``enumerate_margins_cpu`` and the j that attains it (ties: the smaller j)."""
    per_j = enumerate_margins_cpu(A, c0, words, lo_bit, hi_bit, ylo, c)
    j = int(np.argmin(per_j))                                                          # (the first of equal minima)
    return float(per_j[j]), j


def certify_cpu(state, tables, x_u8, classes, eps: float, enum_bits: int = 10, min_margin: float = 1e-6, mean=CIFAR_MEAN,
                std=CIFAR_STD, stem_planes=None, return_planes: bool = False, return_bounds: bool = False):
    """The numpy float64 twin of ``ttnet_certify_u8``: records (dtype ``RECORD``) for uint8 HWC images ``[n, 32, 32, 3]``.
    ``state``: the state dict as numpy arrays; ``tables``: ``{Block_TT name: canonical table}`` (``model.get_table``);
    ``stem_planes``: ``(lo_bit, hi_bit)`` uint8 ``[n, 64, 10, 10]`` to use instead of stage 0 (the device's, for a comparison
    of the later stages that a bound within the slack of zero cannot disturb).  ``return_planes``: also a dict of the four
    planes as uint8 bit arrays.  ``return_bounds``: also float64 ``[n, 10]``, the bound of every class j (``+inf`` at j = c and
    for an invalid class) from the stage that gave the record its ``lb`` and ``worst``: what decides between two candidates
    for ``worst``.  The extras follow the records in that order."""
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    if not 0 <= int(enum_bits) <= ENUM_BITS_MAX:
        raise ValueError(f"enum_bits must be in [0, {ENUM_BITS_MAX}], got {enum_bits}")
    x_u8 = np.asarray(x_u8)
    n = x_u8.shape[0]
    classes = np.asarray(classes).astype(np.int64).reshape(-1)
    if x_u8.dtype != np.uint8 or x_u8.shape[1:] != (32, 32, 3) or classes.size != n:
        raise ValueError(f"expected uint8 images [n, 32, 32, 3] and n classes, got {x_u8.dtype} {x_u8.shape}, {classes.size}")
    lo_bit, hi_bit = stem_planes if stem_planes is not None else stem_planes_cpu(state, x_u8, eps, mean, std)
    lo_bit, hi_bit = np.asarray(lo_bit, dtype=np.uint8), np.asarray(hi_bit, dtype=np.uint8)
    ylo, yhi = block_planes_cpu(tables, lo_bit, hi_bit)
    A, c0 = effective_head(state)
    words = block_words(tables)
    rows = np.zeros(n, dtype=RECORD)
    bounds = np.full((n, N_CLASSES), np.inf)
    rows["unknown_stem"] = (lo_bit != hi_bit).reshape(n, -1).sum(axis=1)
    rows["unknown_feat"] = (ylo != yhi).reshape(n, -1).sum(axis=1)
    for i in range(n):
        c = int(classes[i])
        if not 0 <= c < N_CLASSES:
            rows[i]["lb_interval"] = rows[i]["lb"] = -np.inf
            rows[i]["worst"] = -1
            continue
        lb = margins_cpu(A, c0, ylo[i].reshape(-1), yhi[i].reshape(-1), c)
        j = int(np.argmin(lb))
        bounds[i] = lb
        rows[i]["lb_interval"] = rows[i]["lb"] = lb[j]
        rows[i]["worst"] = j
        rows[i]["stage"] = 1 if lb[j] > min_margin else 0
        if rows[i]["stage"] == 0 and 1 <= rows[i]["unknown_stem"] <= enum_bits:
            bounds[i] = enumerate_margins_cpu(A, c0, words, lo_bit[i], hi_bit[i], ylo[i], c)
            j2 = int(np.argmin(bounds[i]))                                              # (the first of equal minima)
            rows[i]["lb"], rows[i]["worst"] = bounds[i][j2], j2
            rows[i]["stage"] = 2 if bounds[i][j2] > min_margin else 0
    extras = ([{"stem_lo": lo_bit, "stem_hi": hi_bit, "feat_lo": ylo, "feat_hi": yhi}] if return_planes else []) + \
             ([bounds] if return_bounds else [])
    return (rows, *extras) if extras else rows
