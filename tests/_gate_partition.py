"""Which batch sizes and which images the gate sweeps run (test infrastructure).

Which image a workgroup handles, in how many rounds and with which table buffer is decided by a few integer formulas
in scale_imagenet_amd/csrc/partition.h, which the launchers and kernels of gate_fused.hip, gate.hip, gate_xs.hip,
gate_va.hip, gate_full.hip and the plan's host code (plan.hip, plan_certify.hip) call.  This file reads them from the library itself, through the stateless
``ttnet_launch_partition`` (it answers without a GPU), so that the batch sizes of tests/test_gpu_gate_batches.py are
DERIVED from the launch arithmetic (first two-round batch, a last round of one image, unequal slices, ...) and
tests/test_gate_batch_sizes_cpu.py can assert, without a GPU, that the chosen sizes reach every one of those cases.
What stays here is test design: the geometries, the sizes that are always run, how sizes and constant images are picked
from the partition, and the order of a sweep.

Drift.  None of the arithmetic is restated here: a launcher that changes a target, a cap, a round length or the
placement changes what these functions return, and tests/test_gate_batch_sizes_cpu.py then says whether the sizes
still reach every case.  On the GPU the sweep still asserts that ``ttnet_plan_query("gate_grid:<block>")`` equals
``fused_grid`` / ``stage1_grid`` for every batch size it runs.  One restatement is left inside the library:
gate_block_kernel keeps the three placement branches of ``fused_owner`` as its own lines beside partition.h's
fused_owner(), which is what this file reads (called as a function the kernel compiled differently and did not pass the
timing rule of profiles/partition_refactor.txt); the comment in the kernel says so.  ``fusable`` remains a restatement
(of fused_block_supported, plan.hip's choice of path, which is no launch partition).
"""
from __future__ import annotations

import os
from functools import lru_cache
from math import gcd
from typing import List, NamedTuple, Tuple

from scale_imagenet_amd import _lib


@lru_cache(maxsize=None)
def part(what: str, *args: int) -> Tuple[int, ...]:
    """ttnet_launch_partition(what, args): the values csrc/partition.h gives, from the library itself."""
    if not os.path.exists(_lib.LIB_PATH):
        from scale_imagenet_amd.build import build_lib
        build_lib(verbose=False)
    return _lib.launch_partition(what, *args)


FT, FBUF, MAX_SCRATCH, _ = part("fused.const")
DW_TARGET, PW_TARGET, PF_TARGET = part("two_launch.const")


class Block(NamedTuple):
    """One 4-branch block as the launchers see it."""
    C: int          # input planes
    H: int          # input size
    HO: int         # branch output size after padding
    stride: int
    last: bool


def blocks_of(spec) -> List[Block]:
    return [Block(b.in_planes, b.in_hw[0], b.out_hw[0], b.stride, b.last) for b in spec.blocks]


def fusable(blocks: List[Block]) -> bool:
    """plan.hip: the fused path needs fused_block_supported() of every block (gate_fused.hip)."""
    return all(b.stride == 2 and b.C % 16 == 0 and (b.H, b.HO) in ((56, 29), (29, 15), (15, 8), (8, 5)) for b in blocks)


# ---- gate_fused.hip ---------------------------------------------------------------------------------------------
# (HO of a launch whose round length does not matter: any fused output size)
_ANY_HO = 5


def fused_round(HO: int) -> int:
    """fused_round(HO): images per round of a workgroup (8, 16, 32, 32 for HO = 29, 15, 8, 5)."""
    return part("fused.round", HO)[0]


def fused_slices(n: int, C: int) -> int:
    """fused_block_slices(): batch slices per strand; even when there are 8 strands (the pair placement)."""
    return part("fused.launch", C, _ANY_HO, n)[1]


def fused_R(n: int, C: int, HO: int) -> int:
    """launch_block_t: the images per round of a launch, fused_launch_round()."""
    return part("fused.launch", C, HO, n)[2]


def fused_grid(n: int, C: int) -> int:
    return part("fused.launch", C, _ANY_HO, n)[0]


def placement_branch(n: int, C: int) -> str:
    """fused_placement(): the branch of fused_owner() that maps blockIdx.x to (strand, slice)."""
    return ("plain", "quad", "pairs8")[part("fused.launch", C, _ANY_HO, n)[3]]


def fused_owner(b: int, n: int, C: int) -> Tuple[int, int]:
    """(strand, slice) of workgroup b, as gate_block_kernel gets st and sl."""
    return part("fused.owner", b, C, n)


def slice_bounds(sl: int, n: int, slices: int) -> Tuple[int, int]:
    """n0, n1 of a batch slice (gate_block_kernel, gate_stage1_kernel and gate_pf_kernel: slice_begin())."""
    return part("slice", sl, n, slices)


def fused_rounds(n: int, C: int, HO: int) -> List[Tuple[int, List[int]]]:
    """Per batch slice (every strand walks the same ones): (n0, [images of round 0, round 1, ...]); the round loop
    ``for (i0 = 0; i0 < total; i0 += R)`` with rn = min(R, total - i0).  A slice without images has no rounds."""
    slices, R = fused_slices(n, C), fused_R(n, C, HO)
    out = []
    for sl in range(slices):
        n0, n1 = slice_bounds(sl, n, slices)
        out.append((n0, [min(R, n1 - n0 - i0) for i0 in range(0, n1 - n0, R)]))
    return out


def fused_locate(image: int, n: int, C: int, HO: int) -> str:
    """For an assertion message: where image ``image`` of a batch of n sits in the fused kernel's walk."""
    R = fused_R(n, C, HO)
    for sl, (n0, rounds) in enumerate(fused_rounds(n, C, HO)):
        if n0 <= image < n0 + sum(rounds):
            i = image - n0
            return f"slice {sl} (images {n0}..{n0 + sum(rounds) - 1}), round {i // R} of {len(rounds)}, position {i % R} of {rounds[i // R]}"
    return "no slice"


# ---- gate.hip ---------------------------------------------------------------------------------------------------

def slices_for(n: int, units: int, target: int) -> int:
    """slices_for(): batch slices per table set so that ``units`` sets spread over at most ``target`` workgroups."""
    return part("slices_for", n, units, target)[0]


def stage1_slices(n: int, C: int) -> Tuple[int, int]:
    """launch_stage1_t: slices of the depthwise units (2 per 16 channels) and of the conv3 units (1 per 16)."""
    _, _, sl_dw, _, sl_pw = part("two_launch.stage1", C, n)
    return sl_dw, sl_pw


def stage1_grid(n: int, C: int) -> int:
    return part("two_launch.stage1", C, n)[0]


def pf_slices(n: int, C: int) -> int:
    """launch_pf_t: grid (C / 8, slices)."""
    return part("two_launch.pf", C, n)[1]


def slice_sizes(n: int, slices: int) -> List[int]:
    return [slice_bounds(sl, n, slices)[1] - slice_bounds(sl, n, slices)[0] for sl in range(slices)]


# ---- batch sizes, derived ---------------------------------------------------------------------------------------

ALWAYS = (1, 3, 63, 64, 65, 255, 256, 257)     # lin1's 256-row tiles, mid_frag's 64-row tiles, an odd n below every slice count


def fused_sizes(blocks: List[Block]) -> List[int]:
    """Batch sizes for a geometry on the fused path.  Per block, with S its largest slice count and R its round:
    S * R (the largest single-round batch), S * R + 1 (the first two-round batch: one slice gets R + 1 images, a last
    round of one, slices unequal), 2 * S * R + 1 (three rounds, the buffer flip at both parities, again a last round
    of one); 31 where a block has 8 strands (odd n, slice count forced down to 30); and the largest of these plus 13
    (many slices with three rounds at once).  The last entry is N_max."""
    sizes = set(ALWAYS)
    for b in blocks:
        S, R = fused_slices(1 << 20, b.C), fused_round(b.HO)
        sizes |= {S * R, S * R + 1, 2 * S * R + 1}
        if b.C // 8 == 8:
            sizes.add(31)
    sizes.add(max(sizes) + 13)
    return sorted(sizes)


def two_launch_sizes(blocks: List[Block], fused_too: bool = False) -> List[int]:
    """Batch sizes for the two-launch kernels: no round loop, so what varies is the slice count against n.  Per
    block and per kernel (depthwise, conv3, convf) with S its largest slice count: S and S + 1 (n == slices, and the
    first unequal partition); 2, 3 and 255..257 lie below and far above every S > 2.  ``fused_too``: the geometry also
    runs fused (the switch comparison), so the fused sizes are included."""
    sizes = set(ALWAYS) | {2}
    for b in blocks:
        for S in stage1_slices(1 << 20, b.C) + ((pf_slices(1 << 20, b.C),) if not b.last else ()):
            sizes |= {S, S + 1}
    if fused_too:
        sizes |= set(fused_sizes(blocks))
    return sorted(sizes)


# ---- gate_xs.hip, gate_va.hip: flat grids, one thread per task, ceil(n * tasks per image / threads) workgroups -------

class FlatKernel(NamedTuple):
    name: str
    per_image: int      # tasks (threads) per image
    threads: int        # workgroup size


def xs_kernels(blocks: List[Block]) -> List[FlatKernel]:
    """launch_xs_branches and, per block, launch_xs_pf or (last block) launch_xs_last."""
    out = []
    for i, b in enumerate(blocks):
        out.append(FlatKernel(f"xs_branches[{i}]", *part("flat.xs_branches", b.C, b.HO)))
        out.append(FlatKernel("xs_last", *part("flat.xs_last", b.C, b.HO, b.HO)) if b.last else FlatKernel(f"xs_pf[{i}]", *part("flat.xs_pf", b.C, b.HO)))
    return out


# launch_va_block (va_dw, va_c3) and launch_va_feat
VA_KERNELS = [FlatKernel(k, *part("flat." + k)) for k in ("va_dw", "va_c3", "va_feat")]


def flat_period(k: FlatKernel) -> int:
    """The smallest n whose tasks fill whole workgroups; every other multiple of it does too, no other n does."""
    return k.threads // gcd(k.per_image, k.threads)


def flat_last_workgroup(k: FlatKernel, n: int) -> Tuple[int, int]:
    """(workgroups, active threads of the last one) of kernel k at batch n."""
    t = n * k.per_image
    return -(-t // k.threads), (t - 1) % k.threads + 1


def flat_sizes(kernels: List[FlatKernel]) -> List[int]:
    """Batch sizes for flat grids.  Per kernel with period g (flat_period): g and g + 1 (the last workgroup full, and
    the first partial one after that), and, since g divides the workgroup size, threads - 1, threads and
    threads + 1 (the same pair far from the start, and the partial workgroup one image short of full)."""
    sizes = set(ALWAYS) | {2}
    for k in kernels:
        g = flat_period(k)
        sizes |= {g, g + 1, k.threads - 1, k.threads, k.threads + 1}
    return sorted(sizes)


def run_order(sizes: List[int]) -> List[int]:
    """Smallest, largest, then the rest from both ends towards the middle, then the largest again: up, down and up, so
    that every size but the first runs on a workspace that a larger batch has written.  (The order shows a WRONG write
    that depends on earlier contents; a MISSING write is shown by the scrub forward the sweep runs before each size.)"""
    s = sorted(sizes)
    if len(s) < 3:
        return s
    rest, out = s[1:-1], [s[0], s[-1]]
    while rest:
        out.append(rest.pop(0))
        if rest:
            out.append(rest.pop())
    return out + [s[-1]]


def edge_images(blocks: List[Block], sizes: List[int]) -> List[int]:
    """Image indices that fall first / last in a slice and first / last in a round of the fused walk, for the second
    slice and the last slice with images, at the two- and three-round sizes of every block (the constant images of
    the sweep are placed there)."""
    n_max, out = max(sizes), {0, max(sizes) - 1}
    for b in blocks:
        S, R = fused_slices(1 << 20, b.C), fused_round(b.HO)
        for n in (S * R + 1, 2 * S * R + 1, n_max):
            if n > n_max:
                continue
            rounds = [r for r in fused_rounds(n, b.C, b.HO) if r[1]]
            for n0, rn in (rounds[min(1, len(rounds) - 1)], rounds[-1], max(rounds, key=lambda r: len(r[1]))):
                i0 = n0
                for k in rn:
                    out |= {i0, i0 + k - 1}
                    i0 += k
    return sorted(out)


def slice_edge_images(blocks: List[Block], sizes: List[int]) -> List[int]:
    """The same for the two-launch kernels: first and last image of the second and of the last batch slice of every
    kernel (depthwise, conv3, convf) of every block, at n = S + 1 (the first unequal partition) and at the largest n."""
    n_max, out = max(sizes), {0, max(sizes) - 1}
    for b in blocks:
        for S in stage1_slices(1 << 20, b.C) + ((pf_slices(1 << 20, b.C),) if not b.last else ()):
            for n in (S + 1, n_max):
                if n > n_max:
                    continue
                sl_n = slices_for(n, 1, S)
                for sl in {min(1, sl_n - 1), sl_n - 1}:
                    n0, n1 = slice_bounds(sl, n, sl_n)
                    out |= {n0, n1 - 1}
    return sorted(out)


def flat_edge_images(kernels: List[FlatKernel], sizes: List[int]) -> List[int]:
    """For flat grids: the last image before and the first after a workgroup boundary that falls between two images
    (multiples of flat_period), the first such boundary and the last one below the largest n, per kernel."""
    n_max, out = max(sizes), {0, max(sizes) - 1}
    for k in kernels:
        g = flat_period(k)
        for m in (g, (n_max - 1) // g * g):
            if 0 < m < n_max:
                out |= {m - 1, m}
    return sorted(out)


# ---- gate_full.hip: grid-stride loops over rows (depthwise) and over wave tasks (grouped 1x1) ---------------------

# launch_full_dw_window: threads (= output rows) per chunk; launch_full_pw_tiles: wave tasks per chunk (512 threads)
FULL_DW_ROWS, _, _, FULL_PW_WAVES, _, _, _, _ = part("full.const")


def _ceil(a: int, b: int) -> int:
    return -(-a // b)


def full_dw_chunks(n: int, C: int, ho: int) -> int:
    """launch_full_dw_window: grid (C, chunks), one thread per (image, output row)."""
    return part("full.dw", n, C, ho)[0]


def full_dw_sweeps(n: int, C: int, ho: int) -> int:
    return _ceil(n * ho, FULL_DW_ROWS * full_dw_chunks(n, C, ho))


def row_bundle(H: int, W: int) -> Tuple[int, int]:
    """RowBundle: (rows per 64-lane wave task, tasks per image)."""
    return part("full.row_bundle", H, W)


def full_pw_chunks(n: int, groups: int, H: int, W: int) -> int:
    """launch_full_pw_tiles: grid (groups, chunks), 8 waves per workgroup, one task per wave and sweep."""
    return part("full.pw", n, groups, H, W)[1]


def full_pw_sweeps(n: int, groups: int, H: int, W: int) -> int:
    return _ceil(n * row_bundle(H, W)[1], FULL_PW_WAVES * full_pw_chunks(n, groups, H, W))


def full_fix_xchunks(n: int, groups: int, H: int, W: int) -> int:
    """launch_full_pw_tiles: the y extent of full_pw_mfma_kernel<OT, true>'s grid."""
    return part("full.pw", n, groups, H, W)[3]


def full_fix_sweeps(n: int, groups: int, H: int, W: int, listed: int) -> int:
    """Sweeps of the float64 pass of one group that has ``listed`` pixels on its list (at most all n * H * W)."""
    tasks, xchunks = part("full.fix", n, groups, H, W, listed)
    return _ceil(tasks, FULL_PW_WAVES * xchunks)


class FullKernel(NamedTuple):
    """One main kernel launch of a block of the full variant: chunks = min(ceil(n * unit / per_chunk), cap)."""
    name: str
    block: int
    kind: str           # "dw" (conv1, conv2) or "pw" (conv3, convf)
    unit: int           # rows (dw) or wave tasks (pw) per image
    per_chunk: int
    cap: int            # chunks at most
    outputs: int        # what the kernel may list, per image: C * ho * wo outputs (dw), groups * H * W pairs (pw); 0: lists nothing
    groups: int
    hw: Tuple[int, int]  # pixel grid (pw) or output size (dw)

    def chunks(self, n: int) -> int:
        return max(1, min(_ceil(n * self.unit, self.per_chunk), self.cap))

    def sweeps(self, n: int) -> int:
        return _ceil(n * self.unit, self.per_chunk * self.chunks(n))


def full_kernels(spec) -> List[FullKernel]:
    """conv1, conv2, conv3 and convf of every block, as run_full_block (plan.hip) launches them."""
    out = []
    for i, b in enumerate(spec.blocks):
        H, W = b.in_hw
        for c in (b.conv1, b.conv2):
            ho, wo = c.out_hw(H, W)
            out.append(FullKernel(f"{b.name} {c.name.rsplit('_', 1)[1]}", i, "dw", ho, FULL_DW_ROWS, part("full.dw", 1, b.in_planes, ho)[1],
                                  b.in_planes * ho * wo, b.in_planes, (ho, wo)))
        for c, (h, w) in ((b.conv3, (H, W)), (b.convf, b.out_hw)):
            out.append(FullKernel(f"{b.name} {c.name.rsplit('_', 1)[1]}", i, "pw", row_bundle(h, w)[1], FULL_PW_WAVES,
                                  part("full.pw", 1, c.groups, h, w)[2], 0 if c.last else part("full.fix_entries", c.groups, h, w)[0], c.groups, (h, w)))
    for k in out:                                     # the two statements of each grid agree
        for n in (1, 7, 40, 200):
            if k.kind == "dw":
                assert (k.chunks(n), k.sweeps(n)) == (full_dw_chunks(n, k.groups, k.unit), full_dw_sweeps(n, k.groups, k.unit))
            else:
                assert (k.chunks(n), k.sweeps(n)) == (full_pw_chunks(n, k.groups, *k.hw), full_pw_sweeps(n, k.groups, *k.hw))
    return out


def full_dw_outputs(spec) -> int:
    """Depthwise outputs per image: C * ho * wo over conv1 and conv2 of every block (ho and wo differ: (6,5) / (5,6) windows)."""
    return sum(k.outputs for k in full_kernels(spec) if k.kind == "dw")


def full_pw_pairs(spec) -> int:
    """(pixel, group) pairs per image over every binarised 1x1 block (the last convf emits floats and lists nothing)."""
    return sum(k.outputs for k in full_kernels(spec) if k.kind == "pw")


def full_fix_cap(spec, max_batch: int) -> int:
    """plan.hip: list entries of a lane: the largest groups * H * W of a binarised 1x1 block, times the reserved batch.
    The depthwise kernels share that area, so it also caps their list (Lane::full_fix, FullDwArgs::fix_cap)."""
    return max(k.outputs for k in full_kernels(spec) if k.kind == "pw") * max_batch


def full_last_single_sweep(k: FullKernel) -> int:
    """The largest batch that kernel k finishes in one sweep (n * unit <= per_chunk * cap; below the cap there is one sweep)."""
    return k.per_chunk * k.cap // k.unit


def full_sizes(spec) -> List[int]:
    """Batch sizes for the full variant: 1, 2, 3 (every grid below its cap); per kernel of every block the last batch of
    one sweep and the first of two; and the largest of these plus 13 (N_max: several kernels deep in their second sweep)."""
    sizes = {1, 2, 3}
    for k in full_kernels(spec):
        n1 = full_last_single_sweep(k)
        sizes |= {n1, n1 + 1}
    sizes.add(max(sizes) + 13)
    return sorted(sizes)


def full_second_sweep(k: FullKernel, n: int) -> Tuple[int, int]:
    """(first, last) image that kernel k touches in its second sweep at batch n, or () if it has none.  Work item t (row or
    wave task) belongs to image t // unit, and sweep s covers items [s, s + 1) * per_chunk * chunks."""
    if k.sweeps(n) < 2:
        return ()
    per_sweep = k.per_chunk * k.chunks(n)
    return per_sweep // k.unit, (min(2 * per_sweep, n * k.unit) - 1) // k.unit


def full_edge_images(spec, sizes: List[int]) -> List[int]:
    """Where the constant images of the sweep go: first and last image of the second sweep of every kernel, at its first
    two-sweep size and at the largest size; and images 0 and N_max - 1."""
    n_max, out = max(sizes), {0, max(sizes) - 1}
    for k in full_kernels(spec):
        for n in (full_last_single_sweep(k) + 1, n_max):
            if n <= n_max:
                out |= set(full_second_sweep(k, n))
    return sorted(out)


FULL = [(6, 10, 1)]                                                      # the shipped full model: p = 60 --layers 1
FULL_CPU_ONLY = [(6, 10, 0)]                                             # sizes asserted on the CPU only
# tests/test_gpu_full_fallback.py, every output listed: (reserved batch, n whose depthwise lists hold everything, n at which
# features.4 alone overflows, n at which every block overflows); test_gate_batch_sizes_cpu.py asserts that they do
FULL_FALLBACK = (40, 5, 6, 40)

# ---- the geometries of the sweep: (nfilter, tfilter, --layers) ---------------------------------------------------
FUSED_ONLY = [(2, 8, 1), (6, 8, 1), (12, 8, 1), (16, 8, 1)]             # TT-small p = 16, 48, 96, 128
BOTH_PATHS = [(8, 8, 0), (8, 8, 1), (8, 8, 2), (4, 8, 1)]               # p = 64 --layers 0, 1, 2 and p = 32: fused AND two-launch by switch
TWO_LAUNCH_BY_GEOMETRY = [(8, 8, 3), (8, 8, 4)]                         # stride-1 blocks: never fused
XSMALL = [(8, 8, 0), (8, 8, 1), (8, 8, 2), (4, 8, 1)]
