// How a batch is cut into slices, rounds, runs and chunks: the launch partition of the stem and of every gate path, once.
// Plain integer functions and named constants, no HIP calls.  The launchers size their grids with them, the kernels find
// their share of the batch with them, plan.hip sizes buffers with them, and ttnet_launch_partition (partition.hip) reads
// them out to the tests, which derive their batch sizes and edge images from what they return.
#pragma once

#include <stdint.h>

#include "va_block.h"

#if defined(__HIPCC__)
#define TT_PART_FN __host__ __device__ constexpr
#else
#define TT_PART_FN constexpr
#endif

namespace ttnet::part {

TT_PART_FN int imin(int a, int b) { return a < b ? a : b; }
TT_PART_FN int imax(int a, int b) { return a > b ? a : b; }
TT_PART_FN int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- common ---------------------------------------------------------------------------------------------------------
// batch slices per table set so that `units` table sets spread over at most `target` workgroups
TT_PART_FN int slices_for(int n, int units, int target) { return imax(1, imin(n, target / imax(1, units))); }
// slice sl of `slices` holds images [slice_begin(sl), slice_begin(sl + 1)): (almost) equal sizes, empty where n < slices
// (Index: int, or the unsigned of a blockIdx)
template <class Index>
TT_PART_FN int slice_begin(Index sl, int n, int slices) { return (int)((long long)sl * n / slices); }

// ---- fused path (gate_fused.hip) --------------------------------------------------------------------------------------
constexpr int kFT = 1024;              // threads per workgroup: 16 waves, 4 per SIMD
constexpr int kFBuf = 65536;           // one table buffer
constexpr int kFMaxScratch = 160 * 1024 - 2 * kFBuf;
constexpr int kFusedTarget = 256;      // workgroups of a block at most: one per CU

// images per round of a workgroup: one depthwise (channel, output row) task per thread, the branch dwords
// of a round in the LDS left over by the two table buffers (8, 16, 32, 32 for HO = 29, 15, 8, 5)
TT_PART_FN int fused_round(int HO) {
  return imin(imin(kFT / (16 * ceil_div(HO, 4)), kFMaxScratch / (HO * HO * 4)), 32);
}
// batch slices per strand (8 input channels): the grid of a block is (C / 8) * slices workgroups
TT_PART_FN int fused_block_slices(int C, int n) {
  const int strands = C / 8;
  int slices = slices_for(n, strands, kFusedTarget);
  if (strands == 8 && slices > 1 && (slices & 1)) slices -= 1;       // (the pair placement wants an even count)
  return slices;
}
// images per round at a launch: no more than the largest slice holds
TT_PART_FN int fused_launch_round(int HO, int n, int slices) { return imax(1, imin(fused_round(HO), ceil_div(n, slices))); }

// Workgroup b -> (strand, slice).  All batch slices of a strand pair get block ids that land on one XCD (round-robin
// dispatch over 8 XCDs; speed only): a table is pulled into one L2 once, and the two strands of a pair share their
// Block_conv3 rows.  Three orders: whole multiples of 8 strand pairs (p = 64: 8, 16, 32 pairs), 4 pairs with an even
// slice count, and the plain order for every other width.  gate_block_kernel keeps these lines a second time (see there).
enum FusedPlacement { kPlain = 0, kQuad = 1, kPairs8 = 2 };
TT_PART_FN FusedPlacement fused_placement(int strands, int slices) {
  const int P = strands / 2;
  return (P >= 8 && P % 8 == 0) ? kPairs8 : ((P == 4 && (slices & 1) == 0) ? kQuad : kPlain);
}
struct FusedOwner { int strand, slice; };
TT_PART_FN FusedOwner fused_owner(int b, int strands, int slices) {
  const int P = strands / 2, x = b & 7, k = b >> 3;
  int st = 0, sl = 0;
  if (P >= 8 && P % 8 == 0) {
    const int m = P / 8, pair = x + 8 * (k % m), kk = k / m;
    st = 2 * pair + (kk & 1);
    sl = kk >> 1;
  } else if (P == 4 && (slices & 1) == 0) {
    st = 2 * (x >> 1) + (k & 1);
    sl = (x & 1) * (slices / 2) + (k >> 1);
  } else {
    st = b % strands;
    sl = b / strands;
  }
  return {st, sl};
}

// ---- two-launch path (gate.hip) ---------------------------------------------------------------------------------------
// stage 1 is one round of the chip: 208 depthwise + 48 conv3 workgroups (measured best split at B = 256; a second round
// of conv3 blocks cost 3-5 us per launch); stage 2 (Block_convf) one workgroup per CU
constexpr int kDwTarget = 208, kPwTarget = 48, kPfTarget = 256;

struct Stage1Grid {
  int n_dw, sl_dw, n_pw, sl_pw;        // depthwise units (2 per 16 channels) and conv3 units (1 per 16), each with its batch slices
  TT_PART_FN int dw_blocks() const { return n_dw * sl_dw; }
  TT_PART_FN int blocks() const { return n_dw * sl_dw + n_pw * sl_pw; }
};
TT_PART_FN Stage1Grid stage1_grid(int C, int n) {
  const int n_dw = (C / 16) * 2, n_pw = C / 16;
  return {n_dw, slices_for(n, n_dw, kDwTarget), n_pw, slices_for(n, n_pw, kPwTarget)};
}
// stage 2: grid (units, slices), one unit per output channel word
TT_PART_FN int pf_units(int C) { return C / 8; }
TT_PART_FN int pf_slices(int C, int n) { return slices_for(n, pf_units(C), kPfTarget); }

// ---- flat grids (gate_xs.hip, gate_va.hip): one thread per task, ceil(n * tasks per image / threads) workgroups ------------
struct FlatGrid {
  int per_image, threads;
  TT_PART_FN size_t tasks(int n) const { return (size_t)n * per_image; }
  TT_PART_FN unsigned workgroups(int n) const { return (unsigned)((tasks(n) + threads - 1) / threads); }
};
TT_PART_FN FlatGrid xs_branches_grid(int C, int Ho) { return {(C / 4) * Ho, 128}; }
TT_PART_FN FlatGrid xs_pf_grid(int C, int Ho) { return {C * Ho, 128}; }
TT_PART_FN FlatGrid xs_last_grid(int C, int Ho, int Wo) { return {C * (Ho / 2) * (Wo / 2), 128}; }
// vAlexnet: (channel, row) of the 11 x 11 planes; (group of 8 channels, row); k-steps of 16 features
constexpr int kVaDwTasks = va::kStemCh * va::kSide, kVaC3Groups = va::kStemCh / 8, kVaC3Tasks = kVaC3Groups * va::kSide, kVaFeatTasks = va::kFeat / 16;
TT_PART_FN FlatGrid va_dw_grid() { return {kVaDwTasks, 128}; }
TT_PART_FN FlatGrid va_c3_grid() { return {kVaC3Tasks, 128}; }
TT_PART_FN FlatGrid va_feat_grid() { return {kVaFeatTasks, 256}; }

// ---- patch sweep (certify.hip): one workgroup per (image, position), cut into launches of at most kPatchGrid workgroups -------
// n * P has no bound that the interface states (max_batch is the caller's), so the sweep is cut whatever n is.  2,048 is four
// rounds of two workgroups on each of 256 CUs: large enough that the tail of a launch is a small share of it, small enough that
// the tests' 3 x 1,024 positions take the cut (two launches), not only batches no test can afford.
constexpr int kPatchGrid = 2048;
TT_PART_FN int patch_positions(int patch, int stride) { return (32 - patch) / stride + 1; }       // along one side of the image
TT_PART_FN long long patch_launches(long long tasks) { return (tasks + kPatchGrid - 1) / kPatchGrid; }
TT_PART_FN int patch_launch_size(long long tasks, long long launch) {      // workgroups of launch 0 .. patch_launches - 1
  return (int)((tasks - launch * kPatchGrid) < kPatchGrid ? (tasks - launch * kPatchGrid) : kPatchGrid);
}

// ---- full variant (gate_full.hip): grid-stride loops, grid (channels or groups, chunks) ---------------------------------
constexpr int kFullDwRows = 256, kFullDwGrid = 1024;      // depthwise: threads (= output rows) per chunk, workgroups at most
constexpr int kFullDwFixGrid = 1024;                      // its float64 pass over the list: workgroups
constexpr int kFullPwWaves = 8, kFullPwGrid = 512;        // grouped 1x1: wave tasks per chunk (512 threads), workgroups at most
constexpr int kFullFixGrid = 256, kFullFixPixels = 16;    // its float64 pass over the list: workgroups at most, listed pixels per wave task
constexpr int kFullFixShare = 4;                          // ... sized for a quarter of the main pass's wave tasks

// chunks = the y extent of the grid: enough for one sweep of the work, but no more than `grid` workgroups over all units
TT_PART_FN int full_cap(int units, int grid) { return imax(1, grid / units); }
TT_PART_FN int full_chunks(int work, int per_chunk, int units, int grid) {
  return imax(1, imin(ceil_div(work, per_chunk), full_cap(units, grid)));
}
// one thread per (image, output row)
TT_PART_FN int full_dw_chunks(int n, int C, int ho) { return full_chunks(n * ho, kFullDwRows, C, kFullDwGrid); }

// A wave task covers as many whole image rows as fit its 64 lanes (one row of 56 pixels, two of 29, four of 16, seven
// of 9): lane = (row r of the bundle, column x).
struct RowBundle {
  int W, rpw, bundles;                 // row width; rows per bundle, bundles per image
  TT_PART_FN RowBundle(int H, int W_) : W(W_), rpw(64 / W_), bundles((H + rpw - 1) / rpw) {}
  struct Pixel { int r, x; };          // row inside the bundle, column
  TT_PART_FN Pixel pixel(int p) const {        // pixel p = 0 .. 63 of a bundle (r >= rpw: beyond it)
    const int r = p / W;
    return {r, p - r * W};
  }
};
TT_PART_FN int full_pw_tasks(int n, int H, int W) { return n * RowBundle(H, W).bundles; }
TT_PART_FN int full_pw_chunks(int tasks, int groups) { return full_chunks(tasks, kFullPwWaves, groups, kFullPwGrid); }
TT_PART_FN int full_fix_xchunks(int tasks, int groups) { return full_chunks(tasks / kFullFixShare, kFullPwWaves, groups, kFullFixGrid); }
TT_PART_FN uint32_t full_fix_tasks(uint32_t listed) { return (listed + (uint32_t)kFullFixPixels - 1u) / (uint32_t)kFullFixPixels; }
// list entries per image that a binarised 1x1 block may need: every (pixel, group) pair.  A lane's list holds the
// largest of them times the reserved batch (plan.hip: full_fix_cap); the depthwise kernels share that area.
TT_PART_FN size_t full_fix_entries(int groups, int H, int W) { return (size_t)groups * H * W; }

// ---- stem (stem.hip): items of one image x 8 output rows, a run of consecutive items per persistent workgroup ----------
constexpr int kStemItemRows = 8;                 // output rows per item
constexpr int NBLK = 56 / kStemItemRows;         // row blocks (items) per image
constexpr int NSTAGE = 3;                    // stage buffers of row-word pieces: written (item j), completed late (j-1), read (j-2)
// workgroups asked for: one per CU, or half the CUs for float32 input where the plan keeps batches in flight (not the full variant)
constexpr int kStemGrid = 256, kStemHalfGrid = 128;
TT_PART_FN int stem_workgroups(int lanes, bool u8, bool full_variant) { return (lanes >= 2 && !u8 && !full_variant) ? kStemHalfGrid : kStemGrid; }
TT_PART_FN int stem_grid(int n, int G) { return imin(n * NBLK, imax(1, G)); }
TT_PART_FN int stem_first_item(int bid, int n, int grid) { return (int)(bid * ((long long)n * NBLK) / grid); }
TT_PART_FN int stem_my_items(int bid, int n, int grid) { return stem_first_item(bid + 1, n, grid) - stem_first_item(bid, n, grid); }
// item j of a run continues the image of item j - 1 (halo copy inside LDS); otherwise a whole tile is loaded
TT_PART_FN bool stem_continues(int first_item, int j) { return j > 0 && (first_item + j) % NBLK != 0; }

}  // namespace ttnet::part
