"""The geometry of ``TT_FHE_XSMALL_vAlexnet``'s block, once, for the numpy twins of the certificate (certify.py) and of
the witness search (attack.py); csrc/va_block.h holds the same for the device and describes the layout.  numpy only.
The order of ``reach``'s t is the order in which a flip gain sums its terms and stage 2 lists its entries."""
from __future__ import annotations

from functools import lru_cache
from typing import Tuple

import numpy as np

from .spec import VAlexSpec

STEM_CH, POOL, FEAT_CH, SIDE, N_CLASSES = 64, 10, 256, 11, 10
STEM_ROWS, FEAT_ROWS, N_FEAT = STEM_CH * POOL, FEAT_CH * SIDE, FEAT_CH * SIDE * SIDE
N_REACH = 21                                             # a stem bit sits in the windows of at most 21 features
WINDOW_SIZE = (6, 6, 8, 1)                               # inputs of a feature of kind (feature channel // 64)
BN_EPS = 1e-5
BLOCKS = ("features.5.Block_conv1", "features.5.Block_conv2", "features.5.Block_conv3")
PADS = VAlexSpec().pads                                  # zero padding of (out1, out2, out3 / out4) as (left, right, top, bottom)


def f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


def fold_bn(state, prefix: str) -> Tuple[np.ndarray, np.ndarray]:
    """Eval-mode BatchNorm as ``y = x * scale + shift`` in float64."""
    scale = f64(state[f"{prefix}.weight"]) / np.sqrt(f64(state[f"{prefix}.running_var"]) + BN_EPS)
    return scale, f64(state[f"{prefix}.bias"]) - f64(state[f"{prefix}.running_mean"]) * scale


def table_words(table: np.ndarray, n: int) -> np.ndarray:
    """A truth table in the canonical order (``[G, 2^n, cout]`` bits, index = inputs MSB first) as uint64 words
    ``[G, cout, max(1, 2^n / 64)]`` indexed by the window itself: bit ``i % 64`` of word ``i / 64``, input p in bit p of i."""
    table = np.asarray(table)
    g, size, cout = table.shape
    assert size == 1 << n
    i = np.arange(size)
    canon = np.zeros(size, dtype=np.int64)
    for p in range(n):
        canon |= ((i >> p) & 1) << (n - 1 - p)
    bits = table[:, canon, :].astype(np.uint64).transpose(0, 2, 1)                     # [G, cout, 2^n], window order
    nw = max(1, size // 64)
    bits = bits.reshape(g, cout, nw, -1)
    return (bits << np.arange(bits.shape[-1], dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def block_words(tables):
    """``[table_words(conv1), (conv2), (conv3)]`` from ``{Block_TT name: canonical table}``."""
    return [table_words(tables[b], 6 if i < 2 else 8) for i, b in enumerate(BLOCKS)]


def zpad(x: np.ndarray, p) -> np.ndarray:
    l, r, t, b = p
    return np.pad(x, ((0, 0), (0, 0), (t, b), (l, r)))


def windows(bits: np.ndarray, kh: int, kw: int, pad: int) -> np.ndarray:
    """[n, C, H, W] -> [n, C, Ho, Wo, kh * kw] (input p = kh index * kw + kw index); the padding is known zeros."""
    x = np.pad(bits, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    ho, wo = x.shape[2] - kh + 1, x.shape[3] - kw + 1
    return np.stack([x[:, :, a:a + ho, b:b + wo] for a in range(kh) for b in range(kw)], axis=-1)


def block_windows(bits: np.ndarray):
    """The window inputs of conv1 ``[n, 64, 10, 11, 6]``, conv2 ``[n, 64, 11, 10, 6]`` and conv3 ``[n, 8 groups, 10, 10, 8]``."""
    n = bits.shape[0]
    return (windows(bits, 3, 2, 1), windows(bits, 2, 3, 1), bits.reshape(n, 8, 8, POOL, POOL).transpose(0, 1, 3, 4, 2))


def window_indices(bits: np.ndarray):
    """The table indices of ``block_windows``: int64, input p in bit p."""
    return tuple((w.astype(np.int64) << np.arange(w.shape[-1])).sum(axis=-1) for w in block_windows(bits))


def reach(ch, y, x, t: int):
    """Feature t (0..20) of those whose windows hold stem bit (ch, y, x), integers or arrays: ``(valid, fc, oy, ox, p)`` --
    whether the window lies in the plane, the feature's channel of the 256 (``fc // 64``: conv1, conv2, conv3, out4), row
    and column, and which input p of that window the stem bit is.  conv1 with doy = -1, 0, 1 outer and dox = 0, 1 inner, conv2
    with doy = 0, 1 outer and dox = -1, 0, 1 inner, the eight conv3 outputs of the group, out4."""
    if t < 6:
        doy, dox = t // 2 - 1, t % 2
        return (y + doy >= 0) & (y + doy < POOL), ch, y + doy, x + dox, (1 - doy) * 2 + (1 - dox)
    if t < 12:
        doy, dox = (t - 6) // 3, (t - 6) % 3 - 1
        return (x + dox >= 0) & (x + dox < POOL), 64 + ch, y + doy, x + dox, (1 - doy) * 3 + (1 - dox)
    if t < 20:
        return True, 128 + ch // 8 * 8 + (t - 12), y, x, ch % 8
    return True, 192 + ch, y, x, 0


def window_input(kind: int, ch: int, oy: int, ox: int, p: int):
    """The inverse: input p of the window of feature (kind, ch, oy, ox) is stem bit ``(channel, y, x)``; None: padding."""
    kw = (2, 3)[kind] if kind < 2 else 1
    y, x = (oy - 1 + p // kw, ox - 1 + p % kw) if kind < 2 else (oy, ox)
    return (ch // 8 * 8 + p if kind == 2 else ch, y, x) if 0 <= y < POOL and 0 <= x < POOL else None


PATCH_MAX = 8                                            # a patch side at most


def field_span(y0: int, h: int) -> Tuple[int, int]:
    """``(first, count)``: the pooled cells whose 5 x 5 pixel field (pixel rows ``3 py - 1 .. 3 py + 3``; likewise columns)
    meets the pixel rows ``[y0, y0 + h)``.  At most 4 for h <= 8; none for row 31 alone, which lies in no field."""
    first, last = (0 if y0 < 3 else (y0 - 1) // 3), min((y0 + h) // 3, POOL - 1)
    return first, max(0, last - first + 1)


def patch_positions(patch: int, stride: int) -> int:
    """Positions of a patch along one side of the 32-pixel image."""
    return (32 - patch) // stride + 1


@lru_cache(maxsize=None)
def reached():
    """``reach`` for every stem bit: five int64 arrays ``[21, 64, 10, 10]`` (valid, fc, oy, ox, p), read-only."""
    ch, y, x = np.meshgrid(np.arange(STEM_CH), np.arange(POOL), np.arange(POOL), indexing="ij")
    out = tuple(np.stack([np.broadcast_to(np.asarray(v, dtype=np.int64), ch.shape) for v in col])
                for col in zip(*(reach(ch, y, x, t) for t in range(N_REACH))))
    for a in out:
        a.setflags(write=False)
    return out
