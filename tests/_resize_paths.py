"""Which code of scale_imagenet_amd/csrc/preproc.hip a resize geometry reaches, and the geometries the path tests run
(test infrastructure).

Plain-integer twins of the two launchers' sizing: ``uniform_plan`` restates ttnet_resize_center_crop_u8 (the resized
size, the crop offsets, the tap counts of the two tables, the staged columns and rows, the LDS bytes, the template
instantiation the dispatch picks, and whether a staged 16-byte piece is the buffer's last, partial one);
``ragged_plan`` restates launch_ragged (rows per tile, dword columns per thread, WIDE, the tap stride, the staging area,
the LDS bytes, accept / refuse).  The coefficient windows come from oracle/pil_resize.py (``_coeffs``), which
tests/test_pil_resize_oracle.py pins to Pillow.

WHICH INSTANTIATION ACTUALLY RAN on an accepted geometry is inferred from these twins, not observed: the library does
not say which kernel it launched.  The one place where the restated arithmetic is tied to the launcher's own is the
refusal text of the uniform entry point, whose LDS byte count tests/test_gpu_resize_paths.py compares with
``uniform_plan(..).lds`` (the sum of every term restated here).  tests/test_resize_paths_cpu.py asserts without a GPU that
the case lists below reach every path; tools/gen_resize_paths_fixture.py writes Pillow's own hashes of every case to
tests/golden/ref_resize_paths.json.
"""
from __future__ import annotations

import json
import math
import os
from functools import lru_cache
from typing import List, NamedTuple, Tuple

import numpy as np

from _util import GOLD, resize_test_images
from oracle import pil_resize as PR

LDS_LIMIT = 160 * 1024
RS_TY, RS_CHUNK, RS_THREADS, RS_STAGE_LOADS = 16, 16, 256, 6
RG_TY, RG_THREADS, RG_ITEMS, RG_CHUNK, RG_STAGE_Q = 16, 256, 16, 16, 6 * 256
UNROLLED = (1, 3, 5, 7, 9)


# ---------------------------------------------------------------------------------------------------------------------
# the single-size entry point

class UniformPlan(NamedTuple):
    nh: int
    nw: int
    y0: int
    x0: int
    ksh: int
    ksv: int
    c0: int
    cw: int
    rmax: int
    row_q: int
    chunk: int
    lds: int
    accepted: bool
    inst: int                 # K of resize_crop_kernel<K, K>; 0: the run-time loops
    tiles: int
    last_tile_rows: int
    partial_piece: bool       # some staged piece index equals total >> 4 with total % 16 != 0

    @property
    def name(self) -> str:
        return f"resize_crop_kernel<{self.inst},{self.inst}> ({self.ksh} / {self.ksv} taps, chunk {self.chunk})"


@lru_cache(maxsize=None)
def _bounds(in_size: int, out_size: int):
    """(first input index, tap count) per output index and the table's tap count; a pass Pillow skips is the identity."""
    if in_size == out_size:
        return np.stack([np.arange(in_size), np.ones(in_size, dtype=np.int64)], axis=1), 1
    bounds, kk = PR._coeffs(in_size, out_size)
    return bounds, kk.shape[1]


@lru_cache(maxsize=None)
def uniform_plan(h: int, w: int, resize: int, crop: int, n: int = 1) -> UniformPlan:
    nh, nw = PR.resized_size(h, w, resize)
    assert nh >= crop and nw >= crop and (crop * 3) % 4 == 0
    y0, x0 = int(round((nh - crop) / 2.0)), int(round((nw - crop) / 2.0))
    bh, ksh = _bounds(w, nw)
    bv, ksv = _bounds(h, nh)
    c0 = int(bh[x0, 0])
    cw = int(bh[x0 + crop - 1, 0] + bh[x0 + crop - 1, 1]) - c0
    tiles = []                                              # (first, end) intermediate row of every tile
    for t0 in range(0, crop, RS_TY):
        last = y0 + min(crop, t0 + RS_TY) - 1
        tiles.append((int(bv[y0 + t0, 0]), int(bv[last, 0] + bv[last, 1])))
    rmax = max(e - s for s, e in tiles)
    row_q = (cw * 3 + 15 + 15) // 16
    chunk = min(RS_CHUNK, (RS_STAGE_LOADS * RS_THREADS) // row_q)
    lds = chunk * row_q * 16 + rmax * crop * 3 + (crop + crop * ksh + RS_TY + RS_TY * ksv) * 4
    accepted = lds <= LDS_LIMIT and chunk >= 1
    inst = ksh if (ksh == ksv and ksh in UNROLLED) else 0
    total = n * h * w * 3
    partial = False
    if accepted and total % 16:
        rows = sorted({r for s, e in tiles for r in range(s, e)})
        for im in range(n):
            for r in rows:
                first = ((im * h + r) * w + c0) * 3
                if (first >> 4) <= (total >> 4) < (first >> 4) + row_q:
                    partial = True
    return UniformPlan(nh, nw, y0, x0, ksh, ksv, c0, cw, rmax, row_q, chunk, lds, accepted, inst, len(tiles),
                       crop - RS_TY * (len(tiles) - 1), partial)


class UniformCase(NamedTuple):
    case: str
    h: int
    w: int
    resize: int
    crop: int
    n: int

    @property
    def seed(self) -> int:
        return self.h * 1000 + self.w + 7 * self.resize

    @property
    def key(self) -> str:
        return f"{self.case}-{self.h}x{self.w}-{self.resize}-{self.crop}-n{self.n}"

    def plan(self) -> UniformPlan:
        return uniform_plan(self.h, self.w, self.resize, self.crop, self.n)

    def images(self) -> np.ndarray:
        return _uniform_images(self)


# case, h, w, resize, crop, images                       what it reaches
UNIFORM_CASES = [UniformCase(*c) for c in [
    ("u1", 40, 50, 40, 32, 2),                           # <1,1>: no resampling
    ("u7", 100, 130, 40, 32, 3),                         # <7,7>
    ("u7", 130, 100, 40, 32, 2),
    ("u9", 140, 150, 40, 32, 2),                         # <9,9>
    ("u11", 200, 170, 40, 32, 2),                        # <0,0> by 11 / 11 taps
    ("u11", 170, 200, 40, 32, 3),
    ("u17", 300, 300, 40, 40, 2),                        # <0,0>, 17 taps, last tile of 8 rows
    ("umix", 64, 97, 32, 32, 3),                         # <0,0> by unequal counts: 7 / 5
    ("umix", 97, 64, 32, 32, 2),                         # 5 / 7
    ("umix", 512, 769, 256, 224, 2),                     # 7 / 5
    ("utail", 50, 50, 32, 32, 1),                        # resize = crop: the crop keeps the buffer's last bytes, total % 16 = 12
    ("utail", 45, 45, 36, 36, 1),                        # total % 16 = 11; a 4-row last tile
    ("utail", 50, 50, 32, 32, 3),                        # the same behind two other images, total % 16 = 4
    ("urows", 90, 70, 24, 20, 3),                        # <7,7> with a 4-row last tile
    ("ubig", 2592, 3888, 256, 224, 1),                   # accepted at 159,216 B of LDS, chunk 3, 23 taps
    ("uwide", 600, 800, 438, 384, 2),                    # another resize / crop: <5,5>
    ("uwide", 500, 375, 438, 384, 2),                    # <3,3>, upscaling
]]
# refused: TTNET_E_UNSUPPORTED, nothing launched (the ragged entry point serves them)
UNIFORM_REFUSED = [UniformCase(*c) for c in [
    ("urefuse", 2700, 4050, 256, 224, 1),                # 165,456 B
    ("urefuse", 2848, 4288, 256, 224, 1),                # 175,248 B
]]


@lru_cache(maxsize=4)
def _uniform_images(c: UniformCase) -> np.ndarray:
    x = resize_test_images(c.n, c.h, c.w, seed=c.seed)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def uniform_oracle(c: UniformCase) -> Tuple[np.ndarray, ...]:
    """The numpy oracle's crops of a case's images (computed once per process, read-only)."""
    out = tuple(PR.resize_center_crop(x, c.resize, c.crop) for x in c.images())
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the ragged entry points

class RaggedPlan(NamedTuple):
    smax: float
    owq: int
    ncol: int
    ty: int
    wide: bool
    kmax: int
    row_q_max: int
    stage_q: int
    lds: int
    accepted: bool
    tiles: int
    last_tile_rows: int
    last_col_threads: int     # live threads of the last dword column
    items: int                # ncol * ty of the RG_ITEMS sums a thread holds


def eval_max_scale(max_h: int, max_w: int, resize: int) -> float:
    """ttnet_eval_views_max_scale"""
    return max(1.0, min(max_h, max_w) / (resize - 1.0 if resize > 1 else 1.0))


def ragged_plan(crop: int, smax: float) -> RaggedPlan:
    """launch_ragged for axis scales up to ``smax`` (``eval_max_scale`` for the centre-crop entry, ``max_scale`` for views)."""
    assert (crop * 3) % 4 == 0
    ow = crop * 3
    owq = ow // 4
    ncol = (owq + RG_THREADS - 1) // RG_THREADS
    ty = min(RG_TY, RG_ITEMS // ncol)
    kmax = 2 * int(math.ceil(smax)) + 3
    cw_max = int(math.ceil((crop + 1) * smax)) + 4
    row_q_max = (cw_max * 3 + 30) // 16
    stage_q = min(RG_CHUNK * row_q_max, RG_STAGE_Q)
    lds = stage_q * 16 + RG_CHUNK * ow + ((3 * kmax + 31) & ~15) + (crop + crop * kmax + 2 * RG_TY + RG_TY * kmax) * 4
    accepted = ty >= 1 and smax <= 1e4 and row_q_max <= RG_STAGE_Q and lds <= LDS_LIMIT
    tiles = (crop + ty - 1) // ty if ty else 0
    return RaggedPlan(smax, owq, ncol, ty, owq > RG_THREADS, kmax, row_q_max, stage_q, lds, accepted, tiles,
                      crop - ty * (tiles - 1) if ty else 0, owq - RG_THREADS * (ncol - 1), ncol * ty)


def ragged_center_plan(max_h: int, max_w: int, resize: int, crop: int) -> RaggedPlan:
    return ragged_plan(crop, eval_max_scale(max_h, max_w, resize))


def largest_accepted_side(resize: int, crop: int, limit: int = 65536) -> int:
    """The largest m with max_h = max_w = m accepted by the ragged centre-crop entry (accept is monotone in m)."""
    lo, hi = 1, limit + 1                                   # lo accepted, hi refused
    assert ragged_center_plan(lo, lo, resize, crop).accepted and not ragged_center_plan(hi, hi, resize, crop).accepted
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ragged_center_plan(mid, mid, resize, crop).accepted:
            lo = mid
        else:
            hi = mid
    return lo


def taps(h: int, w: int, resize: int) -> Tuple[int, int]:
    """(horizontal, vertical) tap counts of Resize(resize) on an h x w image; 1: the pass is skipped."""
    nh, nw = PR.resized_size(h, w, resize)
    one = lambda i, o: 1 if i == o else int(math.ceil(max(float(np.float32(i)) / o, 1.0))) * 2 + 1
    return one(w, nw), one(h, nh)


# (resize, crop) of the ragged and view batches: 340 is the last crop that is not WIDE (255 dword columns), 344 the first
# (258: two live threads in the second column); 344, 384, 448 have 2 columns and 8 rows per tile, 684 has 3 and 5 (a 4-row
# last tile, 15 of 16 items)
RAGGED_PAIRS = [(40, 20), (292, 256), (360, 340), (360, 344), (438, 384), (512, 448), (730, 684)]
VIEW_PAIRS = [(360, 344), (730, 684)]


def ragged_sizes(resize: int) -> List[Tuple[int, int]]:
    """One mixed batch per resize R: upscaled (3 / 3 taps), 5 / 5, 7 / 7, unequal counts (5 / 7), and last an image
    whose shorter side already is R (no resampling), with a width that leaves the buffer's length no multiple of 16."""
    R = resize
    sizes = [(6 * R // 10, 8 * R // 10), (3 * R // 2 + 1, 13 * R // 10), (2 * R + R // 20, 2 * R + R // 5 + 1), (2 * R + 1, 2 * R)]
    return sizes + [(R, R + R // 8 + 2)]                   # (the CPU test asserts the buffer's length % 16 != 0 for every R used)


def ragged_seed(resize: int, i: int) -> int:
    return 9000 + 10 * resize + i


@lru_cache(maxsize=2)
def ragged_images(resize: int) -> Tuple[np.ndarray, ...]:
    out = tuple(resize_test_images(1, h, w, seed=ragged_seed(resize, i))[0] for i, (h, w) in enumerate(ragged_sizes(resize)))
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def ragged_oracle(resize: int, crop: int) -> Tuple[np.ndarray, ...]:
    out = tuple(PR.resize_center_crop(x, resize, crop) for x in ragged_images(resize))
    for a in out:
        a.setflags(write=False)
    return out


def view_boxes(resize: int, crop: int) -> List[Tuple[int, ...]]:
    """Explicit views (image, flags, bx, by, bw, bh, nw, nh, x0, y0) of the batch ``ragged_sizes(resize)``."""
    s = ragged_sizes(resize)
    (h0, w0), (h1, w1), (h2, w2), (h4, w4) = s[0], s[1], s[2], s[4]
    bw2 = 2 * (crop + 25)
    return [
        # the bottom-right quarter of the last image, upscaled, mirrored, the window in its corner: ends on the buffer's last byte
        (4, 1, w4 - w4 // 2, h4 - h4 // 2, w4 // 2, h4 // 2, crop + 10, crop + 6, 10, 6),
        (2, 0, 3, 5, bw2, h2 - 5, bw2 // 2, crop, 12, 0),                  # 5 taps horizontally (scale 2), 7 vertically
        (1, 1, 7, 9, crop + 4, h1 - 9, crop + 4, crop, 4, 0),              # no horizontal pass, 5 taps vertically
        (0, 1, 0, 0, w0, h0, crop + crop // 2, crop, 3, 0),                # the whole first image, upscaled
        (2, 0, 0, 11, w2, crop, crop + 1, crop, 1, 0),                     # 7 taps horizontally, no vertical pass
    ]


@lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(GOLD, "ref_resize_paths.json")) as f:
        return json.load(f)


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    """For an assertion message: the first (y, x, c) at which two crops differ."""
    d = np.argwhere(got != want)
    if not len(d):
        return "equal"
    y, x, c = (int(v) for v in d[0])
    return f"{len(d)} bytes differ, first at (y {y}, x {x}, c {c}): got {int(got[y, x, c])}, want {int(want[y, x, c])}"
