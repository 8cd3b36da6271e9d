// The geometry of TT_FHE_XSMALL_vAlexnet's block, once, for the forward (gate_va.hip), the certificate (certify.hip), the
// witness search (attack.hip) and the plan's buffer sizes; valexnet_block.py holds the same for the numpy twins.
//   stem bits  [64][10][10], row-packed: one word per (channel, row), bit x = column x
//   features   [256][11][11] = conv1 (3x2 window, pad 1: 10 x 11) | conv2 (2x3, pad 1: 11 x 10) | conv3 (1x1 over the 8 channels
//              of a group) | out4 = the stem bits, each zero-padded to 11 x 11
//   window input p of a feature = bit p of its table index: conv1 p = 2 kh + kw, conv2 p = 3 kh + kw, conv3 p = channel & 7
// Two orders are contractual (the byte-identity tests against the twins rest on them): reach()'s t, in which a flip gain sums
// its terms and stage 2 lists its entries, and window_input()'s p.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ttnet::va {

constexpr int kStemCh = 64, kPool = 10, kStemRows = kStemCh * kPool, kStemBits = kStemRows * kPool;
constexpr int kFeatCh = 256, kSide = 11, kFeatRows = kFeatCh * kSide, kPlane = kSide * kSide, kFeat = kFeatCh * kPlane;
constexpr int kClasses = 10, kImg = 32 * 32 * 3;
constexpr int kWsum = kStemCh * 3 * 25;                 // attack's summed stem kernels: [64][3][5][5]
constexpr int kReach = 21;                              // a stem bit sits in the windows of at most 21 features

// the 64-entry table of channel c from the striped dword layout of lut_build.hip ([c/16][2][16])
__device__ inline uint64_t table_word(const uint32_t *__restrict__ t, int c) {
  const size_t tb = (size_t)(c >> 4) * 2 * 16 + (c & 15);
  return t[tb] | ((uint64_t)t[tb + 16] << 32);
}

// stem row iy as row(iy) loads it, shifted so that bit 0 = column -1; a row outside the plane is padding: known zeros
template <class Load> __device__ inline auto shifted_row(int iy, Load row) -> decltype(row(0)) {
  return (iy >= 0 && iy < kPool) ? (decltype(row(0)))(row(iy) << 1) : 0;
}

// window indices: conv1 at column ox from the shifted rows oy-1..oy+1, conv2 from oy-1..oy, conv3 at column x from the
// (unshifted) rows of the group's 8 channels.  The three-valued kernels take them of the value and of the unknown words.
template <class W> __device__ inline uint32_t conv1_index(W a, W b, W d, int ox) {
  return (uint32_t)((a >> ox) & 3) | ((uint32_t)((b >> ox) & 3) << 2) | ((uint32_t)((d >> ox) & 3) << 4);
}
template <class W> __device__ inline uint32_t conv2_index(W a, W b, int ox) {
  return (uint32_t)((a >> ox) & 7) | ((uint32_t)((b >> ox) & 7) << 3);
}
template <class W> __device__ inline uint32_t conv3_index(const W (&rows)[8], int x) {
  uint32_t idx = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) idx |= (uint32_t)((rows[k] >> x) & 1) << k;
  return idx;
}

// Feature t (0..20) of those whose windows hold stem bit (ch, y, x): conv1 with doy = -1, 0, 1 outer and dox = 0, 1 inner,
// conv2 with doy = 0, 1 outer and dox = -1, 0, 1 inner, the eight conv3 outputs of the group, out4.
struct Reach {
  bool valid;           // the window lies in the plane
  int fc, oy, ox, p;    // channel of the 256 (fc / 64: the branch), row, column; the stem bit is input p of that window
  __host__ __device__ int row() const { return fc * kSide + oy; }
  __host__ __device__ int flat() const { return fc * kPlane + oy * kSide + ox; }
};
__host__ __device__ inline Reach reach(int ch, int y, int x, int t) {
  if (t < 6) {
    const int doy = t / 2 - 1, dox = t % 2;
    return {y + doy >= 0 && y + doy < kPool, ch, y + doy, x + dox, (1 - doy) * 2 + (1 - dox)};
  }
  if (t < 12) {
    const int doy = (t - 6) / 3, dox = (t - 6) % 3 - 1;
    return {x + dox >= 0 && x + dox < kPool, 64 + ch, y + doy, x + dox, (1 - doy) * 3 + (1 - dox)};
  }
  if (t < 20) return {true, 128 + (ch & ~7) + (t - 12), y, x, ch & 7};
  return {true, 192 + ch, y, x, 0};
}

// The inverse: input p of the window of feature (kind, ch, oy, ox) is stem bit (ch, y, x), or padding (in = false).
struct StemBit {
  bool in;
  int ch, y, x;
};
__host__ __device__ inline int window_size(int kind) { return kind < 2 ? 6 : kind == 2 ? 8 : 1; }
__host__ __device__ inline StemBit window_input(int kind, int ch, int oy, int ox, int p) {
  const int y = kind == 0 ? oy - 1 + p / 2 : kind == 1 ? oy - 1 + p / 3 : oy;
  const int x = kind == 0 ? ox - 1 + p % 2 : kind == 1 ? ox - 1 + p % 3 : ox;
  return {y >= 0 && y < kPool && x >= 0 && x < kPool, kind == 2 ? (ch & ~7) + p : ch, y, x};
}

// The pooled cells whose 5 x 5 pixel field (pixel rows 3 py - 1 .. 3 py + 3; likewise columns) meets the pixel rows
// [y0, y0 + h): cells first .. first + count - 1.  At most 4 for h <= 8; none for a patch in row 31 alone, which lies in no field.
struct FieldSpan {
  int first, count;
  __host__ __device__ int last() const { return first + count - 1; }
};
__host__ __device__ inline FieldSpan field_span(int y0, int h) {
  const int first = y0 < 3 ? 0 : (y0 - 1) / 3, last = (y0 + h) / 3 < kPool - 1 ? (y0 + h) / 3 : kPool - 1;
  return {first, last >= first ? last - first + 1 : 0};
}
constexpr int kPatchMax = 8, kFieldCells = 4, kFieldPixels = 3 * kFieldCells + 2;   // patch side at most; cells, pixel rows a span holds at most

}  // namespace ttnet::va
