"""Which batch sizes and which images the stem sweeps run (test infrastructure).

scale_imagenet_amd/csrc/stem.hip cuts a batch into items (one image x 8 output rows, seven per image) and gives every
persistent workgroup a run of consecutive items.  The arithmetic -- the grid, a workgroup's first item and item count,
whether an item continues the image of the one before -- stands once, in csrc/partition.h, which the launcher, the
kernel and plan.hip call; this file reads it from the library through the stateless ``ttnet_launch_partition`` (it
answers without a GPU).  G is 256, or 128 for float32 input on a plan with two or more lanes; the uint8 kernel always
gets 256.  What depends on the run: the tile double buffer (item j in buffer j & 1), the NSTAGE = 3 stage ring whose rows
are emitted two periods late, the sign word carried across the item barrier, and ``continues(j)``, which picks the halo
copy inside LDS (the item continues the image of the one before) or a whole-tile load (first item of a run, or of an
image).

The sizes of tests/test_gpu_stem_batches.py are chosen with these functions, and tests/test_stem_batch_sizes_cpu.py
asserts without a GPU that they reach every case.  Nothing of the partition is restated here: if NBLK, the grid rule or
``continues`` change in the library, the CPU test says whether SIZES still reaches every case.
"""
from __future__ import annotations

from typing import List, NamedTuple

from _gate_partition import part

NBLK, NSTAGE, _, _ = part("stem.const")     # row blocks (items) per image; stage buffers of row-word pieces
# workgroups asked for (lanes, uint8 input, full variant).  float32 input: two or more lanes, one lane
GRIDS = (part("stem.workgroups", 2, 0, 0)[0], part("stem.workgroups", 1, 0, 0)[0])
GRID_U8 = part("stem.workgroups", 2, 1, 0)[0]
# the batch sizes of the sweep (tests/test_stem_batch_sizes_cpu.py: what each one is there for)
#   n     runs on G = 128   runs on G = 256
#   1     1                 1                  7 workgroups
#   19    1, 2              1                  133 workgroups on G = 256
#   64    3, 4              1, 2               no run crosses an image boundary
#   74    4, 5              2, 3
#   150   8, 9              4, 5               42 runs on G = 128 hold a whole image
# (110 and 129 add run lengths 6, 7 on G = 128 but no case the assertions name: left out to keep the sweep short)
SIZES = [1, 19, 64, 74, 150]
N_MAX = 150


def grid(n: int, G: int) -> int:
    return part("stem.grid", n, G)[0]


def first_item(bid: int, n: int, G: int) -> int:
    return part("stem.run", bid, n, G)[0]


def my_items(bid: int, n: int, G: int) -> int:
    return part("stem.run", bid, n, G)[1]


def continues(bid: int, j: int, n: int, G: int) -> bool:
    """Item j of the workgroup continues the image of its item j - 1 (halo copy); otherwise a whole tile is loaded."""
    return bool(part("stem.continues", first_item(bid, n, G), j)[0])


class Run(NamedTuple):
    first: int                # first item
    items: int

    @property
    def starts_mid_image(self) -> bool:
        return self.first % NBLK != 0

    @property
    def crosses_boundary(self) -> bool:
        """An image boundary strictly inside the run: a whole-tile load in the middle of it."""
        return any((self.first + j) % NBLK == 0 for j in range(1, self.items))

    @property
    def holds_whole_image(self) -> bool:
        k = -(-self.first // NBLK)                          # first image that starts inside the run
        return NBLK * (k + 1) <= self.first + self.items


def runs(n: int, G: int) -> List[Run]:
    return [Run(first_item(b, n, G), my_items(b, n, G)) for b in range(grid(n, G))]


def run_lengths(n: int, G: int) -> List[int]:
    return sorted({r.items for r in runs(n, G)})


def edge_images(n: int, G: int, count: int = 4) -> List[int]:
    """``count`` distinct images of a batch of n (fewer if n is smaller) for the constant inputs of the uint8 sweep:
    the first image, the last one (it ends the last item of the last workgroup), the first image in between that a run
    of several items starts inside, the first one in between that begins in the middle of a run; filled up from the
    middle of the batch."""
    rs = runs(n, G)
    inner = lambda images: [i for i in images if 0 < i < n - 1]
    cand = [0, n - 1]
    cand += inner(r.first // NBLK for r in rs if r.starts_mid_image and r.items > 1)[:1]
    cand += [i for i in inner(-(-r.first // NBLK) for r in rs if r.crosses_boundary) if i not in cand][:1]
    out: List[int] = []
    for i in cand + list(range(n // 2, n)) + list(range(n)):
        if i not in out and len(out) < min(count, n):
            out.append(i)
    return out
