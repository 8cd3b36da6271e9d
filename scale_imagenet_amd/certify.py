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
from .valexnet_block import (FEAT_ROWS, N_CLASSES, N_FEAT, N_REACH, PADS, PATCH_MAX, STEM_ROWS, WINDOW_SIZE,  # noqa: F401
                             block_windows, block_words, f64, field_span, fold_bn, patch_positions, reach, table_words,
                             window_input, zpad)                                        # (some only re-exported)

RECORD = np.dtype([("lb_interval", "<f8"), ("lb", "<f8"), ("worst", "<i4"), ("stage", "<i4"), ("unknown_stem", "<i4"),
                   ("unknown_feat", "<i4")])                # the 32-byte record of ttnet_certify_u8
MAP_RECORD = np.dtype([("lb", "<f8"), ("worst", "<i4"), ("stage", "<u2"), ("unknown_stem", "<u2")])   # 16 bytes: ttnet_certify_patch_u8's map
PATCH_ROW = np.dtype([("lb_min", "<f8"), ("pos_min", "<i4"), ("worst", "<i4"), ("certified", "<i4"), ("interval", "<i4"),
                      ("enumeration", "<i4"), ("positions", "<i4")])               # 32 bytes: its record per image
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
    return _planes_result(rows, words, n, return_planes)


def _planes_result(rows, words, n: int, return_planes: bool) -> CertifyResult:
    planes = None
    if return_planes:
        a, b = n * STEM_ROWS, n * FEAT_ROWS
        planes = {"stem_lo": words[:a].view(n, 64, 10), "stem_hi": words[a:2 * a].view(n, 64, 10),
                  "feat_lo": words[2 * a:2 * a + b].view(n, 256, 11), "feat_hi": words[2 * a + b:].view(n, 256, 11)}
    return CertifyResult(rows, planes)


def certify_box_u8(model, lo_u8, hi_u8, classes, enum_bits: int = 10, min_margin: float = 1e-6, lane: int = 0,
                   return_planes: bool = False, check_order: bool = True) -> CertifyResult:
    """``certify_u8`` for a box given per byte: byte k of image i may take any real value in ``[lo_u8, hi_u8]`` (two uint8 HIP
    tensors ``[N, 32, 32, 3]``).  ``lo_u8 > hi_u8`` anywhere raises ValueError (``check_order``: one synchronising comparison;
    without it the device takes such a byte as the degenerate box ``lo``).  The records and planes are ``certify_u8``'s."""
    import torch

    from . import _lib
    lo_u8, classes = checked_inputs(model, lo_u8, classes, "certify_box_u8", "the certificate needs")
    hi_u8, _ = checked_inputs(model, hi_u8, classes, "certify_box_u8", "the certificate needs")
    if hi_u8.shape != lo_u8.shape or hi_u8.device != lo_u8.device:
        raise RuntimeError(f"lo and hi differ: {tuple(lo_u8.shape)} on {lo_u8.device}, {tuple(hi_u8.shape)} on {hi_u8.device}")
    if check_order and bool((lo_u8 > hi_u8).any()):
        raise ValueError("certify_box_u8: lo > hi somewhere")
    if not 0 <= int(enum_bits) <= ENUM_BITS_MAX:
        raise ValueError(f"enum_bits must be in [0, {ENUM_BITS_MAX}], got {enum_bits}")
    n = lo_u8.shape[0]
    plan = model._plan_for(lo_u8.device, n)
    rows = torch.empty((n, 4), dtype=torch.float64, device=lo_u8.device)
    words = torch.empty(n * 2 * (STEM_ROWS + FEAT_ROWS) if return_planes else 0, dtype=torch.int64, device=lo_u8.device)
    stream = torch.cuda.current_stream(lo_u8.device).cuda_stream
    _lib.check(plan.lib.ttnet_certify_box_u8(plan.handle, int(lane), C.c_void_p(lo_u8.data_ptr()), C.c_void_p(hi_u8.data_ptr()), n,
                                             C.c_void_p(classes.data_ptr()), int(enum_bits), float(min_margin),
                                             C.c_void_p(rows.data_ptr()), C.c_void_p(words.data_ptr() if return_planes else None),
                                             C.c_void_p(stream)))
    return _planes_result(rows, words, n, return_planes)


class PatchResult:
    """What one ``certify_patch_u8`` call left on the device: ``rows`` float64 ``[n, 4]`` holding the n 32-byte records of the
    images, ``map`` float64 ``[n, Py, Px, 2]`` holding the 16-byte records of the positions.  ``numpy()`` gives both as
    structured arrays (``PATCH_ROW`` ``[n]``, ``MAP_RECORD`` ``[n, Py, Px]``) and synchronises."""

    def __init__(self, rows, map_, patch, stride, amp):
        self.rows, self.map, self.patch, self.stride, self.amp = rows, map_, tuple(patch), int(stride), int(amp)

    def __len__(self):
        return self.rows.shape[0]

    def numpy(self) -> Tuple[np.ndarray, np.ndarray]:
        return (self.rows.cpu().numpy().view(PATCH_ROW).reshape(-1),
                self.map.cpu().numpy().view(MAP_RECORD).reshape(self.map.shape[:3]))


def check_patch(patch, stride, amp) -> Tuple[int, int, int, int, int, int]:
    """``(h, w, stride, amp, Py, Px)`` of a patch sweep, or ValueError."""
    try:
        h, w = (int(v) for v in patch)
    except (TypeError, ValueError):
        raise ValueError(f"patch must be a pair (h, w), got {patch!r}") from None
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (*patch, stride, amp))
    if not ok or not (1 <= h <= PATCH_MAX and 1 <= w <= PATCH_MAX and 1 <= stride <= 32 and 1 <= amp <= 255):
        raise ValueError(f"patch {patch!r} (1..{PATCH_MAX} each), stride {stride!r} (1..32), amp {amp!r} (1..255): integers in range")
    return h, w, int(stride), int(amp), patch_positions(h, int(stride)), patch_positions(w, int(stride))


def certify_patch_u8(model, x_u8, classes, patch=(1, 1), stride: int = 1, amp: int = 255, enum_bits: int = 10,
                     min_margin: float = 1e-6, lane: int = 0) -> PatchResult:
    """Certify image i of ``x_u8`` against a patch of ``patch = (h, w)`` pixels at every position ``(a * stride, b * stride)``
    that keeps it inside the image: the patch's bytes move by up to ``amp`` byte levels (255: any value), every other byte is
    exact.  One record per (image, position), equal to what ``certify_box_u8`` gives for that box, and one per image; an image
    is patch-certified when ``certified == positions`` (a statement about every placement only at ``stride=1``).
    Asynchronous on the current stream.  No graph capture."""
    import torch

    from . import _lib
    x_u8, classes = checked_inputs(model, x_u8, classes, "certify_patch_u8", "the certificate needs")
    h, w, stride, amp, py, px = check_patch(patch, stride, amp)
    if not 0 <= int(enum_bits) <= ENUM_BITS_MAX:
        raise ValueError(f"enum_bits must be in [0, {ENUM_BITS_MAX}], got {enum_bits}")
    n = x_u8.shape[0]
    plan = model._plan_for(x_u8.device, n)
    rows = torch.empty((n, 4), dtype=torch.float64, device=x_u8.device)
    map_ = torch.empty((n, py, px, 2), dtype=torch.float64, device=x_u8.device)
    stream = torch.cuda.current_stream(x_u8.device).cuda_stream
    _lib.check(plan.lib.ttnet_certify_patch_u8(plan.handle, int(lane), C.c_void_p(x_u8.data_ptr()), n, C.c_void_p(classes.data_ptr()),
                                               h, w, stride, amp, int(enum_bits), float(min_margin), C.c_void_p(rows.data_ptr()),
                                               C.c_void_p(map_.data_ptr()), C.c_void_p(stream)))
    return PatchResult(rows, map_, (h, w), stride, amp)


def summarise_patch(patch, stride: int, amp: int, rows: np.ndarray, maps: np.ndarray) -> dict:
    """What ``certify_patch_batches`` reports per patch size, from the records of all images and positions."""
    k = maps["unknown_stem"].reshape(-1)
    return {"patch": tuple(patch), "stride": int(stride), "amp": int(amp), "images": int(rows.size),
            "certified": int((rows["certified"] == rows["positions"]).sum()) if rows.size else 0,
            "positions": int(rows["positions"].sum()), "positions_certified": int(rows["certified"].sum()),
            "interval": int(rows["interval"].sum()), "enumeration": int(rows["enumeration"].sum()),
            "unknown_stem_median": float(np.median(k)) if k.size else 0.0, "unknown_stem_max": int(k.max()) if k.size else 0,
            "rows": rows, "map": maps}


def certify_patch_batches(model, batches: Iterable, patches: Sequence, stride: int = 1, amp: int = 255, enum_bits: int = 10,
                          min_margin: float = 1e-6, lane: int = 0) -> List[dict]:
    """``certify_patch_u8`` of the targets of ``batches`` (``cifar.device_batches``) for every patch size of ``patches``.  One
    dict per size (``summarise_patch``); ``rows`` and ``map`` in dataset order.  The records stay on the device until the last
    batch."""
    import torch
    patches = [tuple(p) for p in patches]
    parts: List[List] = [[] for _ in patches]
    for x, t in batches:
        for i, p in enumerate(patches):
            parts[i].append(certify_patch_u8(model, x, t, p, stride, amp, enum_bits, min_margin, lane))
    out = []
    for p, res in zip(patches, parts):
        h, w, _, _, py, px = check_patch(p, stride, amp)
        rows = torch.cat([r.rows for r in res]).cpu().numpy().view(PATCH_ROW).reshape(-1) if res else np.zeros(0, dtype=PATCH_ROW)
        maps = (torch.cat([r.map for r in res]).cpu().numpy().view(MAP_RECORD).reshape(-1, py, px) if res
                else np.zeros((0, py, px), dtype=MAP_RECORD))
        out.append(summarise_patch((h, w), stride, amp, rows, maps))
    return out


def patch_line(s: dict) -> str:
    """``Patch.. size=HxW amp=A stride=S [sampled ]certified/N pct (positions p/P certified: interval a, enumeration b; unknown
    stem bits median u max v)``; ``sampled`` when the stride is above 1, since only stride 1 covers every placement."""
    pct = 100.0 * s["certified"] / max(1, s["images"])
    return (f"Patch.. size={s['patch'][0]}x{s['patch'][1]} amp={s['amp']} stride={s['stride']} {'sampled ' if s['stride'] > 1 else ''}"
            f"{s['certified']}/{s['images']} {pct:.2f} (positions {s['positions_certified']}/{s['positions']} certified: interval "
            f"{s['interval']}, enumeration {s['enumeration']}; unknown stem bits median {s['unknown_stem_median']:g} max "
            f"{s['unknown_stem_max']})")


PATCH_ROWS_HEADER = ["size", "amp", "stride", "index", "class", "patch_certified", "certified", "positions", "interval",
                     "enumeration", "lb_min", "pos_min", "worst"]


def write_patch_rows_csv(path: Optional[str], summaries: Sequence[dict], classes: Sequence[int]):
    """The image records of ``certify_patch_batches`` as CSV (``PATCH_ROWS_HEADER``; floats by ``repr``)."""
    from .report import write_csv
    out = [list(PATCH_ROWS_HEADER)]
    for s in summaries:
        if len(classes) != s["rows"].size:
            raise ValueError(f"{len(classes)} classes for {s['rows'].size} records")
        for i, (r, c) in enumerate(zip(s["rows"], classes)):
            out.append([f"{s['patch'][0]}x{s['patch'][1]}", s["amp"], s["stride"], i, int(c), int(r["certified"] == r["positions"]),
                        int(r["certified"]), int(r["positions"]), int(r["interval"]), int(r["enumeration"]), repr(float(r["lb_min"])),
                        int(r["pos_min"]), int(r["worst"])])
    write_csv(path, out)


def write_patch_map_npz(path: str, summaries: Sequence[dict]):
    """The position records as .npz: per size ``lb_HxW`` float64, ``stage_HxW`` uint8, ``worst_HxW`` int8 and
    ``unknown_stem_HxW`` uint16, each ``[N, Py, Px]``; written to a temporary name and renamed."""
    from .report import replacing
    arrays = {}
    for s in summaries:
        key = f"{s['patch'][0]}x{s['patch'][1]}"
        m = s["map"]
        arrays.update({f"lb_{key}": m["lb"], f"stage_{key}": m["stage"].astype(np.uint8), f"worst_{key}": m["worst"].astype(np.int8),
                       f"unknown_stem_{key}": m["unknown_stem"]})
    with replacing(path, "wb") as f:
        np.savez(f, **arrays)


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


def eps_box(x_u8, eps: float) -> Tuple[np.ndarray, np.ndarray]:
    """The box of ``certify_cpu``: float64 byte levels ``(max(0, b - eps), min(255, b + eps))``."""
    b = np.asarray(x_u8).astype(np.float64)
    return np.maximum(0.0, b - eps), np.minimum(255.0, b + eps)


def stem_bounds_cpu(state, x_u8: np.ndarray, eps: float, mean=CIFAR_MEAN, std=CIFAR_STD) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 0 without the slack: float64 ``(lo, hi)`` ``[n, 64, 10, 10]`` of the pooled pre-activation over the box."""
    return stem_bounds_box_cpu(state, *eps_box(x_u8, eps), mean, std)


def stem_bounds_box_cpu(state, lo, hi, mean=CIFAR_MEAN, std=CIFAR_STD) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 0 without the slack for byte levels in ``[lo, hi]`` (HWC ``[n, 32, 32, 3]``, any real values): float64 ``(lo, hi)``
    ``[n, 64, 10, 10]`` of the pooled pre-activation."""
    a, off = _norm(mean, std)
    x_lo = (f64(lo).transpose(0, 3, 1, 2) - off[None, :, None, None]) * a[None, :, None, None]
    x_hi = (f64(hi).transpose(0, 3, 1, 2) - off[None, :, None, None]) * a[None, :, None, None]
    return _stem_bounds_norm(state, x_lo, x_hi, 1)


def _stem_bounds_norm(state, x_lo: np.ndarray, x_hi: np.ndarray, pad: int) -> Tuple[np.ndarray, np.ndarray]:
    """... from normalised CHW bounds ``[n, 3, H, W]``; ``pad`` 1: zero padding around them (zero in normalised space), 0: the
    arrays carry what surrounds them (the pixel windows of ``_patch_stem_planes``)."""
    import torch
    import torch.nn.functional as F
    w = f64(state["features.0.weight"])
    wp, wn = torch.from_numpy(np.maximum(w, 0.0)), torch.from_numpy(np.minimum(w, 0.0))
    bias = torch.from_numpy(f64(state["features.0.bias"]))
    tl, th = torch.from_numpy(np.ascontiguousarray(x_lo)), torch.from_numpy(np.ascontiguousarray(x_hi))
    lo = F.relu(F.conv2d(tl, wp, bias, 1, pad) + F.conv2d(th, wn, None, 1, pad))      # zero padding: zero in normalised space
    hi = F.relu(F.conv2d(th, wp, bias, 1, pad) + F.conv2d(tl, wn, None, 1, pad))
    scale, shift = (torch.from_numpy(v)[None, :, None, None] for v in fold_bn(state, "features.2"))
    pos = scale >= 0
    ylo = torch.where(pos, lo, hi) * scale + shift                                     # a negative scale swaps the bounds
    yhi = torch.where(pos, hi, lo) * scale + shift
    return F.max_pool2d(ylo, 3).numpy(), F.max_pool2d(yhi, 3).numpy()


def stem_planes_cpu(state, x_u8, eps: float, mean=CIFAR_MEAN, std=CIFAR_STD) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 0: uint8 ``(lo_bit, hi_bit)`` ``[n, 64, 10, 10]``; unknown where they differ."""
    return stem_planes_box_cpu(state, *eps_box(x_u8, eps), mean, std)


def stem_planes_box_cpu(state, lo, hi, mean=CIFAR_MEAN, std=CIFAR_STD) -> Tuple[np.ndarray, np.ndarray]:
    """Stage 0 for byte levels in ``[lo, hi]``."""
    lo, hi = stem_bounds_box_cpu(state, lo, hi, mean, std)
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
    x_u8 = np.asarray(x_u8)
    if x_u8.dtype != np.uint8:
        raise ValueError(f"expected uint8 images [n, 32, 32, 3], got {x_u8.dtype} {x_u8.shape}")
    return certify_box_cpu(state, tables, *eps_box(x_u8, eps), classes, enum_bits, min_margin, mean, std, stem_planes, return_planes,
                           return_bounds)


def certify_box_cpu(state, tables, lo, hi, classes, enum_bits: int = 10, min_margin: float = 1e-6, mean=CIFAR_MEAN, std=CIFAR_STD,
                    stem_planes=None, return_planes: bool = False, return_bounds: bool = False):
    """The numpy float64 twin of ``ttnet_certify_box_u8``: byte k of image i may take any real value in ``[lo, hi]`` (HWC
    ``[n, 32, 32, 3]``: uint8 as the device takes them, or any real byte levels, which is how ``certify_cpu`` states its eps
    box).  ``lo > hi`` anywhere raises ValueError.  Everything else as ``certify_cpu``."""
    if not 0 <= int(enum_bits) <= ENUM_BITS_MAX:
        raise ValueError(f"enum_bits must be in [0, {ENUM_BITS_MAX}], got {enum_bits}")
    lo, hi = np.asarray(lo), np.asarray(hi)
    n = lo.shape[0] if lo.ndim else 0
    classes = np.asarray(classes).astype(np.int64).reshape(-1)
    if lo.shape != hi.shape or lo.shape[1:] != (32, 32, 3) or classes.size != n:
        raise ValueError(f"expected boxes [n, 32, 32, 3] and n classes, got {lo.shape}, {hi.shape}, {classes.size}")
    if (lo > hi).any() or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("certify_box_cpu: lo > hi somewhere, or a bound that is not finite")
    lo_bit, hi_bit = stem_planes if stem_planes is not None else stem_planes_box_cpu(state, lo, hi, mean, std)
    return _certify_planes_cpu(state, tables, lo_bit, hi_bit, classes, enum_bits, min_margin, return_planes, return_bounds)


def _certify_planes_cpu(state, tables, lo_bit, hi_bit, classes, enum_bits, min_margin, return_planes, return_bounds):
    """Stages 1 and 2 of the twin from the stem planes."""
    n = classes.size
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


# ---- all positions of a patch: the twin of ttnet_certify_patch_u8 -------------------------------------------------------------

def patch_origins(patch, stride: int) -> np.ndarray:
    """``[P, 2]`` int: ``(y0, x0)`` of every position, row-major."""
    h, w, stride, _, py, px = check_patch(patch, stride, 1)
    return np.stack(np.meshgrid(np.arange(py) * stride, np.arange(px) * stride, indexing="ij"), axis=-1).reshape(-1, 2)


def patch_boxes(x_u8: np.ndarray, patch, stride: int = 1, amp: int = 255) -> Tuple[np.ndarray, np.ndarray]:
    """The boxes of one image ``[32, 32, 3]`` materialised: uint8 ``(lo, hi)`` ``[P, 32, 32, 3]``, what ``certify_box_u8`` /
    ``certify_box_cpu`` take (the non-incremental way, for tests and measurements)."""
    h, w, stride, amp, _, _ = check_patch(patch, stride, amp)
    org = patch_origins((h, w), stride)
    x = np.asarray(x_u8)
    lo, hi = (np.broadcast_to(x, (len(org),) + x.shape).copy() for _ in range(2))
    b = x.astype(np.int64)
    for p, (y0, x0) in enumerate(org):
        lo[p, y0:y0 + h, x0:x0 + w] = np.maximum(0, b[y0:y0 + h, x0:x0 + w] - amp)
        hi[p, y0:y0 + h, x0:x0 + w] = np.minimum(255, b[y0:y0 + h, x0:x0 + w] + amp)
    return lo, hi


def _patch_stem_planes(state, x: np.ndarray, clean_lo, clean_hi, h, w, stride, amp, mean, std):
    """Stage 0 of every position of one image, incrementally: only the pooled cells whose field meets the patch are bounded
    again, from the pixels of those fields (at most 14 x 14).  Returns ``(lo_bit, hi_bit)`` uint8 ``[P, 64, 10, 10]``."""
    org = patch_origins((h, w), stride)
    P = len(org)
    spans = [(field_span(int(y0), h), field_span(int(x0), w)) for y0, x0 in org]
    nr, nc = max(s[0][1] for s in spans), max(s[1][1] for s in spans)
    lo_bit, hi_bit = (np.broadcast_to(v, (P,) + v.shape).copy() for v in (clean_lo, clean_hi))
    if nr == 0 or nc == 0:
        return lo_bit, hi_bit
    a, off = _norm(mean, std)
    b = np.zeros((33, 33, 3))                                                          # row / column 0: the padding (set to zero below)
    b[1:, 1:] = x.astype(np.float64)
    # a window of nr x nc cells from cell (fr, fc): padded pixel rows 3 fr .. 3 fr + 3 nr + 1.  Positions with fewer cells get
    # neighbours that the patch cannot reach; only the cells of the true span are taken over.
    fr = np.array([min(s[0][0], 10 - nr) for s in spans])
    fc = np.array([min(s[1][0], 10 - nc) for s in spans])
    rr = 3 * fr[:, None] + np.arange(3 * nr + 2)[None, :]                               # [P, wr] padded rows
    qq = 3 * fc[:, None] + np.arange(3 * nc + 2)[None, :]
    win = b[rr[:, :, None], qq[:, None, :]]                                            # [P, wr, wq, 3]
    inside = (((rr - 1 >= org[:, :1]) & (rr - 1 < org[:, :1] + h))[:, :, None] & ((qq - 1 >= org[:, 1:]) & (qq - 1 < org[:, 1:] + w))[:, None, :])
    bl = np.where(inside[..., None], np.maximum(0.0, win - amp), win)
    bh = np.where(inside[..., None], np.minimum(255.0, win + amp), win)
    padding = ((rr == 0)[:, :, None] | (qq == 0)[:, None, :])[..., None]
    x_lo = np.where(padding, 0.0, (bl - off) * a).transpose(0, 3, 1, 2)                # the padding is zero in normalised space
    x_hi = np.where(padding, 0.0, (bh - off) * a).transpose(0, 3, 1, 2)
    lo, hi = _stem_bounds_norm(state, x_lo, x_hi, 0)                                   # [P, 64, nr, nc]
    sl = stem_slack(state, mean, std)[None, :, None, None]
    wlo = (lo - sl >= 0).astype(np.uint8)
    whi = (hi + sl >= 0).astype(np.uint8) | wlo
    for p, ((r0, cr), (q0, cq)) in enumerate(spans):
        if cr and cq:
            lo_bit[p, :, r0:r0 + cr, q0:q0 + cq] = wlo[p, :, r0 - fr[p]:r0 - fr[p] + cr, q0 - fc[p]:q0 - fc[p] + cq]
            hi_bit[p, :, r0:r0 + cr, q0:q0 + cq] = whi[p, :, r0 - fr[p]:r0 - fr[p] + cr, q0 - fc[p]:q0 - fc[p] + cq]
    return lo_bit, hi_bit


def patch_rows_from_map(maps: np.ndarray) -> np.ndarray:
    """The image records (``PATCH_ROW``) that belong to position records ``[n, Py, Px]``, as the device folds them."""
    n = maps.shape[0]
    flat = maps.reshape(n, -1)
    rows = np.zeros(n, dtype=PATCH_ROW)
    for i in range(n):
        p = int(np.argmin(flat[i]["lb"]))                                              # (the first of equal minima)
        rows[i] = (flat[i]["lb"][p], p, flat[i]["worst"][p], int((flat[i]["stage"] > 0).sum()), int((flat[i]["stage"] == 1).sum()),
                   int((flat[i]["stage"] == 2).sum()), flat.shape[1])
    return rows


def certify_patch_cpu(state, tables, x_u8, classes, patch=(1, 1), stride: int = 1, amp: int = 255, enum_bits: int = 10,
                      min_margin: float = 1e-6, mean=CIFAR_MEAN, std=CIFAR_STD, return_planes: bool = False, chunk: int = 128):
    """The numpy float64 twin of ``ttnet_certify_patch_u8``: ``(rows, map)`` of dtypes ``PATCH_ROW`` ``[n]`` and ``MAP_RECORD``
    ``[n, Py, Px]``.  Incremental as the device is: per image the clean planes and the sums ``S_j``, ``U_j`` once; per position
    stage 0 for the cells whose field meets the patch, and ``lb_j = c0_c - c0_j + ((S_j + dS_j) + (U_j + dU_j))`` with the
    differences summed over the features whose three-valued value left the clean one (numpy sums them in its own order, the
    device in the order include/ttnet.h states: the same real number).  The lookups of a position whose stem planes changed are
    taken on whole planes, batched over positions; a position whose stem planes did not change takes the clean sums as they are.
    ``return_planes``: also a list of n dicts of uint8 bit arrays ``stem_lo, stem_hi`` ``[P, 64, 10, 10]`` and ``feat_lo, feat_hi``
    ``[P, 256, 11, 11]``."""
    h, w, stride, amp, py, px = check_patch(patch, stride, amp)
    if not 0 <= int(enum_bits) <= ENUM_BITS_MAX:
        raise ValueError(f"enum_bits must be in [0, {ENUM_BITS_MAX}], got {enum_bits}")
    x_u8 = np.asarray(x_u8)
    n = x_u8.shape[0] if x_u8.ndim else 0
    classes = np.asarray(classes).astype(np.int64).reshape(-1)
    if x_u8.dtype != np.uint8 or x_u8.shape[1:] != (32, 32, 3) or classes.size != n:
        raise ValueError(f"expected uint8 images [n, 32, 32, 3] and n classes, got {x_u8.dtype} {x_u8.shape}, {classes.size}")
    A, c0 = effective_head(state)
    words = block_words(tables)
    P = py * px
    maps = np.zeros((n, P), dtype=MAP_RECORD)
    all_planes = []
    for i in range(n):
        c = int(classes[i])
        valid = 0 <= c < N_CLASSES
        clean_lo, clean_hi = (v[0] for v in stem_planes_cpu(state, x_u8[i:i + 1], 0.0, mean, std))
        ylo_c, yhi_c = (v[0].reshape(-1) for v in block_planes_cpu(tables, clean_lo[None], clean_hi[None]))
        unk_c = (ylo_c != yhi_c)
        lo_bit, hi_bit = _patch_stem_planes(state, x_u8[i], clean_lo, clean_hi, h, w, stride, amp, mean, std)
        maps[i]["unknown_stem"] = (lo_bit != hi_bit).reshape(P, -1).sum(axis=1)
        changed = np.flatnonzero(((lo_bit != clean_lo[None]) | (hi_bit != clean_hi[None])).reshape(P, -1).any(axis=1))
        if return_planes:
            fl, fh = (np.broadcast_to(v.reshape(256, 11, 11), (P, 256, 11, 11)).copy() for v in (ylo_c, yhi_c))
            all_planes.append({"stem_lo": lo_bit, "stem_hi": hi_bit, "feat_lo": fl, "feat_hi": fh})
        if not valid:
            maps[i]["lb"], maps[i]["worst"] = -np.inf, -1
            if return_planes:
                for a0 in range(0, changed.size, chunk):
                    sel = changed[a0:a0 + chunk]
                    fl[sel], fh[sel] = block_planes_cpu(tables, lo_bit[sel], hi_bit[sel])
            continue
        D = A[c][None, :] - A
        Dm = np.minimum(D, 0.0)
        S, U = D @ ylo_c.astype(np.float64), Dm @ unk_c.astype(np.float64)
        lbs = np.broadcast_to(c0[c] - c0 + (S + U), (P, N_CLASSES)).copy()
        dS = np.zeros((P, N_CLASSES))
        ylo_of = {}
        for a0 in range(0, changed.size, chunk):
            sel = changed[a0:a0 + chunk]
            ylo, yhi = (v.reshape(sel.size, -1) for v in block_planes_cpu(tables, lo_bit[sel], hi_bit[sel]))
            if return_planes:
                fl[sel], fh[sel] = ylo.reshape(-1, 256, 11, 11), yhi.reshape(-1, 256, 11, 11)
            for k, p in enumerate(sel):
                f = np.flatnonzero((ylo[k] != ylo_c) | (yhi[k] != yhi_c))
                dS[p] = D[:, f] @ (ylo[k, f].astype(np.float64) - ylo_c[f])
                dU = Dm[:, f] @ ((ylo[k, f] != yhi[k, f]).astype(np.float64) - unk_c[f])
                lbs[p] = c0[c] - c0 + ((S + dS[p]) + (U + dU))
                ylo_of[int(p)] = ylo[k]
        lbs[:, c] = np.inf
        for p in range(P):
            j = int(np.argmin(lbs[p]))
            lb, stage = lbs[p, j], 1 if lbs[p, j] > min_margin else 0
            if stage == 0 and 1 <= maps[i, p]["unknown_stem"] <= enum_bits:
                per_j = enumerate_margins_cpu(A, c0, words, lo_bit[p], hi_bit[p], ylo_of.get(p, ylo_c).reshape(256, 11, 11), c)
                j = int(np.argmin(per_j))                                              # (the first of equal minima)
                lb, stage = per_j[j], 2 if per_j[j] > min_margin else 0
            maps[i, p]["lb"], maps[i, p]["worst"], maps[i, p]["stage"] = lb, j, stage
    maps = maps.reshape(n, py, px)
    out = (patch_rows_from_map(maps), maps)
    return (*out, all_planes) if return_planes else out
