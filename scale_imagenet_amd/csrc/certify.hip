// Certified L-infinity robustness of TT_FHE_XSMALL_vAlexnet (include/ttnet.h: ttnet_certify_u8; DESIGN: certified robustness).
//
//   stage 0  certify_stem_kernel    interval arithmetic through conv3x3 + bias -> ReLU -> BatchNorm -> MaxPool(3) in float64,
//                                   widened by the per-channel slack: two row-packed planes, lo_bit = (lo >= 0), hi_bit = (hi >= 0)
//   stage 1  certify_dw_kernel,     the block on three-valued bits: an output bit can be 1 iff a table entry compatible with
//            certify_c3_kernel      the known inputs is 1 -- the table word ANDed with one selector word per input
//            certify_margin_kernel  lb_j = c0_c - c0_j + sum_f D_f ylo_f + sum_{f unknown} min(0, D_f), D = A_c - A_j
//   stage 2  certify_enum_kernel    all 2^k completions of the k unknown stem bits; only the features whose windows hold one
//                                   are re-evaluated, the others enter through a base sum
//   certify_head_kernel, certify_t3_words_kernel: the effective head A = lin2 diag(bn_scale) lin1, c0, and the 256-entry
//   tables of Block_conv3 as four 64-bit words per output bit; once per loaded state
//
//   ttnet_certify_box_u8 is the same with stage 0's intervals taken from two images (a loader parameter of certify_stem_kernel).
//   ttnet_certify_patch_u8: all positions of a patch.  Per image the clean planes and sums (the stages above on the degenerate
//   box), then certify_patch_kernel, one workgroup per (image, position): the stem bounds of the <= 4 x 4 pooled cells whose
//   field meets the patch, the features those cells reach, lb_j = clean sums + the changed features' differences -- the steps of
//   patch_position.h, which the patch search (attack.hip) takes too --, stage 2 in the workgroup (enumerate_completions, the body
//   of certify_enum_kernel), and certify_patch_rows_kernel, which folds an image's positions into its record.
//
// Everything is float64 and integer work in a fixed order: no float atomics, the same bytes on every run.

#include <math.h>

#include "certify_lookup.h"
#include "partition.h"
#include "patch_position.h"
#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

using namespace va;

namespace {

constexpr int kInter = 100, kMaxEnum = 12, kMaxEnt = kMaxEnum * kReach;

struct Row {            // one record of ttnet_certify_u8, 32 bytes
  double lb_interval, lb;
  int32_t worst, stage, unknown_stem, unknown_feat;
};
static_assert(sizeof(Row) == 32, "record layout of include/ttnet.h");

// A[j][f] = sum_i lin2[j][i] * s[i] * lin1[i][f] (i ascending; stored [f][j]), c0[j] = sum_i lin2[j][i] * t[i] + bias[j]
__global__ __launch_bounds__(256) void certify_head_kernel(const float *__restrict__ lin1, const float *__restrict__ lin2,
                                                           const float *__restrict__ bias, const double *__restrict__ bn,
                                                           double *__restrict__ A, double *__restrict__ c0) {
  __shared__ double m_s[kClasses][kInter];
  for (int i = threadIdx.x; i < kClasses * kInter; i += blockDim.x) m_s[i / kInter][i % kInter] = (double)lin2[i] * bn[i % kInter];
  __syncthreads();
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < kClasses) {
    double acc = 0.0;
    for (int i = 0; i < kInter; ++i) acc += (double)lin2[threadIdx.x * kInter + i] * bn[kInter + i];
    c0[threadIdx.x] = acc + (double)bias[threadIdx.x];
  }
  if (f >= kFeat) return;
  double acc[kClasses];
#pragma unroll
  for (int j = 0; j < kClasses; ++j) acc[j] = 0.0;
  for (int i = 0; i < kInter; ++i) {
    const double v = (double)lin1[(size_t)i * kFeat + f];
#pragma unroll
    for (int j = 0; j < kClasses; ++j) acc[j] += m_s[j][i] * v;
  }
#pragma unroll
  for (int j = 0; j < kClasses; ++j) A[(size_t)f * kClasses + j] = acc[j];      // [feature][class]: what one feature adds is 80 contiguous bytes
}

// t3w[(g * 8 + o) * 4 + w] bit b = output o of entry 64 w + b of group g
__global__ void certify_t3_words_kernel(const uint8_t *__restrict__ t3, uint64_t *__restrict__ t3w) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 8 * 8 * 4) return;
  const int w = t & 3, o = (t >> 2) & 7, g = t >> 5;
  uint64_t word = 0;
  for (int b = 0; b < 64; ++b) word |= (uint64_t)((t3[g * 256 + 64 * w + b] >> o) & 1u) << b;
  t3w[t] = word;
}

// stage 0: five workgroups per image, each two pooled rows: thread = (channel, pooled row) as va_stem_kernel.  The eight
// image rows those need (image rows 3 p0 - 1 .. 3 p0 + 6, p0 = the first pooled row) live in LDS as the centre and the
// radius of each normalised pixel's interval, with the zero column on the left (the padding is zero in normalised space:
// centre 0, radius 0; the pooled outputs never touch the right or bottom padding).  13 KiB of LDS per workgroup.
// The loader takes the interval of byte b from eps (xhi == nullptr) or from the two images (the box [b, max(b, xhi's byte)]).
constexpr int kStemRowsPerWg = 2, kStemLdsRows = 3 * kStemRowsPerWg + 2;

__global__ __launch_bounds__(64 * kStemRowsPerWg) void certify_stem_kernel(
    const uint8_t *__restrict__ x, const uint8_t *__restrict__ xhi, CertifyNorm nm, const float *__restrict__ w,
    const float *__restrict__ bias, const double *__restrict__ bn, const double *__restrict__ slack, double eps,
    uint64_t *__restrict__ lo_rp, uint64_t *__restrict__ hi_rp, int n) {
  __shared__ double img_s[2][3][kStemLdsRows][34];
  constexpr int kParts = kPool / kStemRowsPerWg;
  const int img = blockIdx.x / kParts, p0 = (blockIdx.x % kParts) * kStemRowsPerWg;
  if (img >= n) return;                                              // (whole workgroups: no barrier is left behind)
  const int r0 = 3 * p0 - 1;                                         // image row of LDS row 0 (-1: the top padding)
  for (int i = threadIdx.x; i < 3 * kStemLdsRows * 34; i += blockDim.x) {   // the zero column, and the zero row of the first part
    const int r = (i / 34) % kStemLdsRows, q = i % 34;
    if (q == 0 || q == 33 || r0 + r < 0) (&img_s[0][0][0][0])[i] = (&img_s[1][0][0][0])[i] = 0.0;
  }
  const uint32_t *src = (const uint32_t *)(x + (size_t)img * kImg);   // (4-byte aligned: checked by the plan; a row is 96 bytes)
  const uint32_t *srch = xhi ? (const uint32_t *)(xhi + (size_t)img * kImg) : nullptr;
  for (int i = threadIdx.x; i < kStemLdsRows * 24; i += blockDim.x) {
    const int lr = i / 24, ir = r0 + lr;                             // ir <= 3 * 8 - 1 + 7 = 30
    if (ir < 0) continue;
    const uint32_t v = src[ir * 24 + (i - lr * 24)], vh = srch ? srch[ir * 24 + (i - lr * 24)] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * (i - lr * 24) + k, q = e / 3, c = e - 3 * q;
      const double b = (double)((v >> (8 * k)) & 0xFFu);
      const double bl = srch ? b : fmax(0.0, b - eps), bh = srch ? fmax(b, (double)((vh >> (8 * k)) & 0xFFu)) : fmin(255.0, b + eps);
      pixel_interval(bl, bh, nm, c, img_s[0][c][lr][q + 1], img_s[1][c][lr][q + 1]);
    }
  }
  __syncthreads();
  const int ch = threadIdx.x & 63, pl = threadIdx.x >> 6, py = p0 + pl;   // one wave per pooled row
  double wr[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) wr[i] = (double)w[ch * 27 + i];
  const double b = (double)bias[ch], sc = bn[ch], sh = bn[64 + ch], sl = slack[ch];
  uint64_t out_lo = 0, out_hi = 0;
#pragma unroll 1
  for (int px = 0; px < 10; ++px) {
#define STEM_AT(k, c, r, q) img_s[k][c][3 * pl + (r)][3 * px + (q)]
#include "certify_stem_cell.inc"
#undef STEM_AT
    out_lo |= (uint64_t)lo_bit << px;
    out_hi |= (uint64_t)hi_bit << px;
  }
  lo_rp[((size_t)img * kStemCh + ch) * kPool + py] = out_lo;
  hi_rp[((size_t)img * kStemCh + ch) * kPool + py] = out_hi;
}

// stage 1, Block_conv1 / Block_conv2 / out4: thread = (image, channel, output row of the 11x11 plane), as va_dw_kernel.
// ylo = the bits that are certainly 1, yhi = the bits that can be 1.
__global__ void certify_dw_kernel(const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi, const uint32_t *__restrict__ t1,
                                  const uint32_t *__restrict__ t2, uint64_t *__restrict__ ylo, uint64_t *__restrict__ yhi, int n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * kStemCh * kSide) return;
  const int oy = t % kSide, c = (t / kSide) % kStemCh, img = t / (kSide * kStemCh);
  const uint64_t *pl = slo + ((size_t)img * kStemCh + c) * kPool, *ph = shi + ((size_t)img * kStemCh + c) * kPool;
  uint64_t l[3], u[3];                                               // rows oy-1 .. oy+1: the values, the unknown bits
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    l[k] = shifted_row(oy - 1 + k, [&](int iy) { return pl[iy]; });
    u[k] = l[k] ^ shifted_row(oy - 1 + k, [&](int iy) { return ph[iy]; });
  }
  const uint64_t T1 = table_word(t1, c), T2 = table_word(t2, c);
  uint64_t r1l = 0, r1h = 0, r2l = 0, r2h = 0;
  if (oy < kPool) {   // conv1: 3x2 window, 11 output columns; bottom row 10 is zero padding
    const bool known = ((u[0] | u[1] | u[2]) & 0xFFFull) == 0;       // the common case at small eps: plain lookups
    for (int ox = 0; ox < kSide; ++ox) {
      const uint32_t idx = conv1_index(l[0], l[1], l[2], ox), un = known ? 0u : conv1_index(u[0], u[1], u[2], ox);
      if (un == 0) {
        const uint64_t bit = (T1 >> idx) & 1ull;
        r1l |= bit << ox;
        r1h |= bit << ox;
      } else {
        const uint64_t S = selector(idx, un);
        r1l |= (uint64_t)((~T1 & S) == 0) << ox;                     // no compatible entry is 0
        r1h |= (uint64_t)((T1 & S) != 0) << ox;                      // some compatible entry is 1
      }
    }
  }
  {                   // conv2: 2x3 window, rows oy-1..oy, 10 output columns; right column 10 is zero padding
    const bool known = ((u[0] | u[1]) & 0xFFFull) == 0;
    for (int ox = 0; ox < kPool; ++ox) {
      const uint32_t idx = conv2_index(l[0], l[1], ox), un = known ? 0u : conv2_index(u[0], u[1], ox);
      if (un == 0) {
        const uint64_t bit = (T2 >> idx) & 1ull;
        r2l |= bit << ox;
        r2h |= bit << ox;
      } else {
        const uint64_t S = selector(idx, un);
        r2l |= (uint64_t)((~T2 & S) == 0) << ox;
        r2h |= (uint64_t)((T2 & S) != 0) << ox;
      }
    }
  }
  const size_t o = (size_t)img * kFeatRows + oy;
  ylo[o + (size_t)c * kSide] = r1l;
  yhi[o + (size_t)c * kSide] = r1h;
  ylo[o + (size_t)(64 + c) * kSide] = r2l;
  yhi[o + (size_t)(64 + c) * kSide] = r2h;
  ylo[o + (size_t)(192 + c) * kSide] = oy < kPool ? pl[oy] : 0ull;   // out4 = x, padded right / bottom
  yhi[o + (size_t)(192 + c) * kSide] = oy < kPool ? ph[oy] : 0ull;
}

// stage 1, Block_conv3: thread = (image, group of 8 channels, row), as va_c3_kernel
__global__ void certify_c3_kernel(const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi, const uint8_t *__restrict__ t3,
                                  const uint64_t *__restrict__ t3w, uint64_t *__restrict__ ylo, uint64_t *__restrict__ yhi, int n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * 8 * kSide) return;
  const int oy = t % kSide, g = (t / kSide) % 8, img = t / (8 * kSide);
  uint64_t l[8], u[8], ol[8], oh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const size_t r = ((size_t)img * kStemCh + 8 * g + k) * kPool + oy;
    l[k] = oy < kPool ? slo[r] : 0ull;
    u[k] = oy < kPool ? slo[r] ^ shi[r] : 0ull;
    ol[k] = oh[k] = 0;
  }
  if (oy < kPool)
    for (int xx = 0; xx < kPool; ++xx) {
      uint32_t idx = 0, un = 0;                                      // conv3_index of l and of u in one pass (two calls: 83 more instructions)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        idx |= (uint32_t)((l[k] >> xx) & 1ull) << k;
        un |= (uint32_t)((u[k] >> xx) & 1ull) << k;
      }
      if (un == 0) {                                                 // plain lookup
        const uint32_t v = t3[g * 256 + idx];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          ol[k] |= (uint64_t)((v >> k) & 1u) << xx;
          oh[k] |= (uint64_t)((v >> k) & 1u) << xx;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          bool can0, can1;
          lookup8(t3w + (g * 8 + k) * 4, idx, un, can0, can1);
          ol[k] |= (uint64_t)(!can0) << xx;
          oh[k] |= (uint64_t)can1 << xx;
        }
      }
    }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    ylo[((size_t)img * kFeatCh + 128 + 8 * g + k) * kSide + oy] = ol[k];
    yhi[((size_t)img * kFeatCh + 128 + 8 * g + k) * kSide + oy] = oh[k];
  }
}

// stage 1, margin: one workgroup per image.  Thread t owns the feature rows t, t + 256, ..; its partial sums meet in a
// fixed tree, so the bytes do not depend on anything but the input.  The sum over the certain features is kept apart
// (sums[img][j] = sum_f D_f ylo_f): stage 2 starts from it.
__global__ __launch_bounds__(256) void certify_margin_kernel(const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi,
                                                             const uint64_t *__restrict__ ylo, const uint64_t *__restrict__ yhi,
                                                             const double *__restrict__ A, const double *__restrict__ c0,
                                                             const int32_t *__restrict__ classes, double min_margin,
                                                             Row *__restrict__ rows, double *__restrict__ sums,
                                                             double *__restrict__ sums_un, int n) {
  __shared__ double red[2 * kClasses][256];                          // [j]: the certain features, [10 + j]: the unknown ones
  __shared__ int cnt_s[2];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (img >= n) return;
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  const int c = classes[img];
  const bool valid = c >= 0 && c < kClasses;
  int us = 0, uf = 0;
  for (int r = tid; r < kStemRows; r += 256) us += __popcll(slo[(size_t)img * kStemRows + r] ^ shi[(size_t)img * kStemRows + r]);
  double acc[2 * kClasses];
#pragma unroll
  for (int j = 0; j < 2 * kClasses; ++j) acc[j] = 0.0;
  for (int r = tid; r < kFeatRows; r += 256) {
    const uint64_t l = ylo[(size_t)img * kFeatRows + r], h = yhi[(size_t)img * kFeatRows + r];
    uf += __popcll(l ^ h);
    if (!valid) continue;
    const int f0 = (r / kSide) * kPlane + (r % kSide) * kSide;
    for (uint64_t m = h & 0x7FFull; m; m &= m - 1) {
      const int bit = __builtin_ctzll(m);
      const double *af = A + (size_t)(f0 + bit) * kClasses;          // the ten classes of a feature are contiguous
      const bool one = (l >> bit) & 1ull;
      const double ac = af[c];
#pragma unroll
      for (int j = 0; j < kClasses; ++j) {
        const double d = ac - af[j];
        acc[j] += one ? d : 0.0;
        acc[kClasses + j] += one ? 0.0 : fmin(0.0, d);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2 * kClasses; ++j) red[j][tid] = acc[j];
  atomicAdd(&cnt_s[0], us);                                          // (integers: any order gives the same sum)
  atomicAdd(&cnt_s[1], uf);
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int j = 0; j < 2 * kClasses; ++j) red[j][tid] += red[j][tid + s];
    __syncthreads();
  }
  if (tid < kClasses) sums[(size_t)img * kClasses + tid] = red[tid][0];
  if (sums_un && tid < kClasses) sums_un[(size_t)img * kClasses + tid] = red[kClasses + tid][0];
  if (tid != 0) return;
  Row out;
  out.lb_interval = -INFINITY;
  out.worst = -1;
  if (valid) {
    double best = INFINITY;
    for (int j = 0; j < kClasses; ++j) {
      if (j == c) continue;
      const double lb = c0[c] - c0[j] + (red[j][0] + red[kClasses + j][0]);
      if (lb < best) {
        best = lb;
        out.worst = j;
      }
    }
    out.lb_interval = best;
  }
  out.lb = out.lb_interval;
  out.stage = out.lb > min_margin ? 1 : 0;
  out.unknown_stem = cnt_s[0];
  out.unknown_feat = cnt_s[1];
  rows[img] = out;
}

// stage 2 for one set of stem planes, by a whole workgroup of 256 threads (every thread calls it, under a condition that is
// uniform over the workgroup): s_lo / s_un = the values and the unknown bits [640] in LDS, written and barriered by the caller;
// k = the number of unknown bits (1 .. kMaxEnum); ylo_bit(feature row, column) = stage 1's lower plane; sums10 = stage 1's
// sum over the certain features.  The unknown bits (channel, row, column ascending) and the features they reach (per unknown
// bit: conv1, conv2, conv3, out4; the first mention of a feature wins) are listed in that fixed order, so the sums below are
// taken in a fixed order too.  Every thread returns the bound and its class.
template <class YLo>
__device__ inline void enumerate_completions(const uint64_t *s_lo, const uint64_t *s_un, int k, int c, YLo ylo_bit, const double *sums10,
                                             const uint32_t *__restrict__ t1, const uint32_t *__restrict__ t2,
                                             const uint64_t *__restrict__ t3w, const double *__restrict__ A,
                                             const double *__restrict__ c0, double &lb, int &worst) {
  __shared__ uint64_t e_T[kMaxEnt][4];
  __shared__ double e_D[kMaxEnt][kClasses];
  __shared__ uint16_t e_key[kMaxEnt], c_key[kMaxEnt];                // feature row * 16 + column: of the entries, of the candidates
  __shared__ uint8_t c_new[kMaxEnt];
  __shared__ uint8_t e_one[kMaxEnt], e_base[kMaxEnt], e_cnt[kMaxEnt], e_pos[kMaxEnt][8], e_unk[kMaxEnt][8];
  __shared__ uint16_t u_pos[kMaxEnum];                               // unknown stem bit i: stem row * 16 + column
  __shared__ int n_ent_s;
  __shared__ double base_s[kClasses];
  __shared__ double rv[256];
  __shared__ int rj[256];
  const int tid = threadIdx.x;
  if (tid < kStemCh) {               // the unknown bits in order: lane = channel, a scan of the lanes' counts gives each its place
    int cnt = 0;
    for (int y = 0; y < kPool; ++y) cnt += __popcll(s_un[tid * kPool + y]);
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (tid >= d) incl += v;
    }
    int at = incl - cnt;
    for (int y = 0; y < kPool; ++y)
      for (uint64_t m = s_un[tid * kPool + y]; m; m &= m - 1, ++at)
        if (at < kMaxEnum) u_pos[at] = (uint16_t)((tid * kPool + y) * 16 + __builtin_ctzll(m));
  }
  __syncthreads();
  // candidate q = 21 i + t: feature t of those that unknown bit i reaches (0xFFFF: it falls outside the plane)
  const int n_cand = kReach * k;                                     // <= kMaxEnt
  uint32_t key = 0xFFFFu;
  if (tid < n_cand) {
    const int i = tid / kReach, t = tid - kReach * i, r = u_pos[i] >> 4, x = u_pos[i] & 15, ch = r / kPool, y = r - kPool * ch;
    const Reach f = reach(ch, y, x, t);
    if (f.valid) key = (uint32_t)(f.row() * 16 + f.ox);
    c_key[tid] = (uint16_t)key;
  }
  __syncthreads();
  if (tid < n_cand) {
    bool fresh = key != 0xFFFFu;
    for (int q = 0; q < tid && fresh; ++q) fresh = c_key[q] != key;
    c_new[tid] = fresh;
  }
  __syncthreads();
  if (tid < n_cand) {
    int at = 0;
    for (int q = 0; q < tid; ++q) at += c_new[q];
    if (c_new[tid]) e_key[at] = (uint16_t)key;
    if (tid == n_cand - 1) n_ent_s = at + c_new[tid];
  }
  __syncthreads();
  const int n_ent = n_ent_s;
  // what each re-evaluated feature needs: its table, the known part of its index, where the unknown bits enter, its D
  for (int e = tid; e < n_ent; e += 256) {
    const int row = e_key[e] >> 4, bit = e_key[e] & 15, fc = row / kSide, oy = row % kSide, kind = fc >> 6, ch = fc & 63;
    uint32_t base = 0;
    int cnt = 0;
    for (int p = 0; p < window_size(kind); ++p) {                    // window input p: an unknown bit, a known one, or padding
      const StemBit s = window_input(kind, ch, oy, bit, p);
      if (!s.in) continue;
      const int r = s.ch * kPool + s.y;
      if ((s_un[r] >> s.x) & 1ull) {
        for (int i = 0; i < k; ++i)
          if (u_pos[i] == r * 16 + s.x) {
            e_pos[e][cnt] = (uint8_t)p;
            e_unk[e][cnt] = (uint8_t)i;
            ++cnt;
          }
      } else if ((s_lo[r] >> s.x) & 1ull) {
        base |= 1u << p;
      }
    }
    uint64_t T[4] = {0, 0, 0, 0};
    if (kind < 2) {
      T[0] = table_word(kind == 0 ? t1 : t2, ch);
    } else if (kind == 2) {
      for (int w = 0; w < 4; ++w) T[w] = t3w[ch * 4 + w];            // (ch = 8 group + output)
    } else {
      T[0] = 2ull;                                                   // out4: the identity on one input
    }
    for (int w = 0; w < 4; ++w) e_T[e][w] = T[w];
    e_base[e] = (uint8_t)base;
    e_cnt[e] = (uint8_t)cnt;
    e_one[e] = (uint8_t)ylo_bit(row, bit);
    const double *af = A + (size_t)(fc * kPlane + oy * kSide + bit) * kClasses;
    const double ac = af[c];
    for (int j = 0; j < kClasses; ++j) e_D[e][j] = ac - af[j];
  }
  __syncthreads();
  // the base: stage 1's sum over the certain features, without those of them that are re-evaluated below
  if (tid < kClasses) {
    double sub = 0.0;
    for (int e = 0; e < n_ent; ++e) sub += e_one[e] ? e_D[e][tid] : 0.0;
    base_s[tid] = tid == c ? INFINITY : c0[c] - c0[tid] + (sums10[tid] - sub);
  }
  __syncthreads();
  double best = INFINITY;
  int best_j = kClasses;
  for (uint32_t a = tid; a < (1u << k); a += 256) {
    double m[kClasses];
#pragma unroll
    for (int j = 0; j < kClasses; ++j) m[j] = base_s[j];
    for (int e = 0; e < n_ent; ++e) {
      uint32_t idx = e_base[e];
      for (int q = 0; q < e_cnt[e]; ++q) idx |= ((a >> e_unk[e][q]) & 1u) << e_pos[e][q];
      if ((e_T[e][idx >> 6] >> (idx & 63)) & 1ull)
#pragma unroll
        for (int j = 0; j < kClasses; ++j) m[j] += e_D[e][j];        // (e_D[e][c] = 0: m[c] stays +inf)
    }
#pragma unroll
    for (int j = 0; j < kClasses; ++j)
      if (m[j] < best || (m[j] == best && j < best_j)) {
        best = m[j];
        best_j = j;
      }
  }
  rv[tid] = best;
  rj[tid] = best_j;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {                               // min of (value, class): the order does not matter
    if (tid < s && (rv[tid + s] < rv[tid] || (rv[tid + s] == rv[tid] && rj[tid + s] < rj[tid]))) {
      rv[tid] = rv[tid + s];
      rj[tid] = rj[tid + s];
    }
    __syncthreads();
  }
  lb = rv[0];
  worst = rj[0];
}

// stage 2: one workgroup per image that stage 1 left open with 1 <= k <= enum_bits unknown stem bits
__global__ __launch_bounds__(256) void certify_enum_kernel(const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi,
                                                           const uint64_t *__restrict__ ylo, const uint32_t *__restrict__ t1,
                                                           const uint32_t *__restrict__ t2, const uint64_t *__restrict__ t3w,
                                                           const double *__restrict__ A, const double *__restrict__ c0,
                                                           const int32_t *__restrict__ classes, int enum_bits, double min_margin,
                                                           Row *__restrict__ rows, const double *__restrict__ sums, int n) {
  __shared__ uint64_t s_lo[kStemRows], s_un[kStemRows];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (img >= n) return;
  const int c = classes[img];
  const int k = rows[img].unknown_stem;
  if (rows[img].stage != 0 || k < 1 || k > enum_bits || k > kMaxEnum || c < 0 || c >= kClasses) return;   // (whole workgroups)
  for (int r = tid; r < kStemRows; r += 256) {
    const uint64_t l = slo[(size_t)img * kStemRows + r];
    s_lo[r] = l;
    s_un[r] = (l ^ shi[(size_t)img * kStemRows + r]) & 0x3FFull;
  }
  __syncthreads();
  double lb;
  int worst;
  enumerate_completions(s_lo, s_un, k, c, [&](int row, int bit) { return (ylo[(size_t)img * kFeatRows + row] >> bit) & 1ull; },
                        sums + (size_t)img * kClasses, t1, t2, t3w, A, c0, lb, worst);
  if (tid != 0) return;
  rows[img].lb = lb;
  rows[img].worst = worst;
  rows[img].stage = lb > min_margin ? 2 : 0;
}

// ---- all positions of a patch (include/ttnet.h: ttnet_certify_patch_u8) -------------------------------------------------------
struct MapRec {         // one (image, position) record, 16 bytes
  double lb;
  int32_t worst;
  uint16_t stage, unknown_stem;
};
struct PatchRow {       // one image's record, 32 bytes
  double lb_min;
  int32_t pos_min, worst, certified, interval, enumeration, positions;
};
static_assert(sizeof(MapRec) == 16 && sizeof(PatchRow) == 32, "record layouts of include/ttnet.h");


// One workgroup per (image, position); task = first_task + blockIdx.x = image * P + position.  The steps are patch_position.h's:
//   1. the clean planes of the image into LDS; the window of the position's box (load_patch_window): at most 14 x 14 x 3
//   2. thread (channel, cell row) recomputes that row's cells and rewrites its words of the planes (rewrite_stem_row)
//   3. the differences of the features those cells reach against the clean feature planes (reached_sums)
//   4. lb_j from the clean sums and their changes (patch_margin); stage 2 in the workgroup
__global__ __launch_bounds__(256, 2) void certify_patch_kernel(
    const uint8_t *__restrict__ x, CertifyNorm nm, const float *__restrict__ w, const float *__restrict__ bias,
    const double *__restrict__ bn, const double *__restrict__ slack, const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi,
    const uint64_t *__restrict__ ylo, const uint64_t *__restrict__ yhi, const uint32_t *__restrict__ t1, const uint32_t *__restrict__ t2,
    const uint64_t *__restrict__ t3w, const double *__restrict__ A, const double *__restrict__ c0, const int32_t *__restrict__ classes,
    const double *__restrict__ sums, const double *__restrict__ sums_un, const Row *__restrict__ clean_rows, PatchGeom g, int enum_bits,
    double min_margin, MapRec *__restrict__ map, long long first_task, long long n_tasks) {
  __shared__ uint64_t s_lo[kStemRows], s_un[kStemRows];
  __shared__ PatchWindow win;
  __shared__ double part[4][2 * kClasses];
  __shared__ double pos_sums[kClasses];
  __shared__ double lb_s;
  __shared__ int dk_s, worst_s, stage_s;
  const long long task = first_task + blockIdx.x;
  if (task >= n_tasks) return;                                       // (whole workgroups)
  const PatchPos p = patch_pos(task, g);
  const int img = p.img, tid = threadIdx.x;
  const int c = classes[img];
  const bool valid = c >= 0 && c < kClasses;
  load_stem_planes(s_lo, s_un, slo, shi, img, tid);
  if (tid == 0) dk_s = 0;
  load_patch_window(win, x, nm, p, g, nullptr, tid);
  __syncthreads();
  if (p.touched() && tid < 64 * p.fr.count) {
    const int ch = tid & 63, cy = tid >> 6, r = ch * kPool + p.fr.first + cy;   // one wave per row of cells
    const int before = __popcll(s_un[r]);
    rewrite_stem_row(s_lo, s_un, r, win, ch, cy, p.fq, w, bias, bn, slack);
    const int dk = __popcll(s_un[r]) - before;
    if (dk) atomicAdd(&dk_s, dk);                                    // (integers: any order gives the same sum)
  }
  __syncthreads();
  reached_sums(s_lo, s_un, p, c, p.touched() && valid, ylo, yhi, t1, t2, t3w, A, part, tid);
  __syncthreads();
  const int k = clean_rows[img].unknown_stem + dk_s;
  if (tid == 0) {
    patch_margin(part, sums, sums_un, c0, img, c, lb_s, worst_s, pos_sums);
    stage_s = (valid && lb_s > min_margin) ? 1 : 0;
  }
  __syncthreads();
  double lb = lb_s;
  int worst = worst_s, stage = stage_s;
  if (valid && stage == 0 && k >= 1 && k <= enum_bits && k <= kMaxEnum) {   // (uniform over the workgroup)
    enumerate_completions(s_lo, s_un, k, c,
                          [&](int row, int bit) {
                            const int fc = row / kSide;
                            bool lo, hi;
                            feature3(s_lo, s_un, fc >> 6, fc & 63, row % kSide, bit, t1, t2, t3w, lo, hi);
                            return lo;
                          },
                          pos_sums, t1, t2, t3w, A, c0, lb, worst);
    stage = lb > min_margin ? 2 : 0;
  }
  if (tid != 0) return;
  MapRec out;
  out.lb = lb;
  out.worst = worst;
  out.stage = (uint16_t)stage;
  out.unknown_stem = (uint16_t)k;                                    // <= 6400
  map[task] = out;
}

// an image's positions into its record: one workgroup per image; the smallest lb, ties to the first position
__global__ __launch_bounds__(256) void certify_patch_rows_kernel(const MapRec *__restrict__ map, PatchRow *__restrict__ rows, int P, int n) {
  __shared__ double rv[256];
  __shared__ int rp[256], cnt_s[2];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (img >= n) return;
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  double best = INFINITY;
  int best_p = P, n1 = 0, n2 = 0;
  for (int p = tid; p < P; p += 256) {
    const MapRec m = map[(size_t)img * P + p];
    n1 += m.stage == 1;
    n2 += m.stage == 2;
    if (m.lb < best || (m.lb == best && p < best_p) || best_p == P) {
      best = m.lb;
      best_p = p;
    }
  }
  rv[tid] = best;
  rp[tid] = best_p;
  if (n1) atomicAdd(&cnt_s[0], n1);
  if (n2) atomicAdd(&cnt_s[1], n2);
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {                               // min of (value, position): the order does not matter
    if (tid < s && rp[tid + s] < P && (rp[tid] == P || rv[tid + s] < rv[tid] || (rv[tid + s] == rv[tid] && rp[tid + s] < rp[tid]))) {
      rv[tid] = rv[tid + s];
      rp[tid] = rp[tid + s];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  PatchRow out;
  out.lb_min = rv[0];
  out.pos_min = rp[0];
  out.worst = map[(size_t)img * P + rp[0]].worst;
  out.interval = cnt_s[0];
  out.enumeration = cnt_s[1];
  out.certified = cnt_s[0] + cnt_s[1];
  out.positions = P;
  rows[img] = out;
}

}  // namespace

int launch_certify_head(const float *lin1, const float *lin2, const float *bias, const double *bn, const uint8_t *t3, double *A,
                        double *c0, uint64_t *t3w, hipStream_t s) {
  hipLaunchKernelGGL(certify_head_kernel, dim3((kFeat + 255) / 256), dim3(256), 0, s, lin1, lin2, bias, bn, A, c0);
  hipLaunchKernelGGL(certify_t3_words_kernel, dim3(1), dim3(256), 0, s, t3, t3w);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_certify(const CertifyArgs &a, int step, hipStream_t s) {
  const int n = a.n;
  Row *rows = (Row *)a.rows;
  if (step == kCertifyStem) {
    hipLaunchKernelGGL(certify_stem_kernel, dim3((unsigned)n * (kPool / kStemRowsPerWg)), dim3(64 * kStemRowsPerWg), 0, s, a.x, a.x_hi, a.norm, a.w, a.bias, a.stem_bn, a.slack, a.eps,
                       a.stem_lo, a.stem_hi, n);
  } else if (step == kCertifyBlock) {
    size_t t = (size_t)n * kStemCh * kSide;
    hipLaunchKernelGGL(certify_dw_kernel, dim3((unsigned)((t + 127) / 128)), dim3(128), 0, s, a.stem_lo, a.stem_hi, a.t1, a.t2,
                       a.feat_lo, a.feat_hi, n);
    t = (size_t)n * 8 * kSide;
    hipLaunchKernelGGL(certify_c3_kernel, dim3((unsigned)((t + 127) / 128)), dim3(128), 0, s, a.stem_lo, a.stem_hi, a.t3, a.t3w,
                       a.feat_lo, a.feat_hi, n);
  } else if (step == kCertifyMargin) {
    hipLaunchKernelGGL(certify_margin_kernel, dim3((unsigned)n), dim3(256), 0, s, a.stem_lo, a.stem_hi, a.feat_lo, a.feat_hi, a.A, a.c0,
                       a.classes, a.min_margin, rows, a.sums, a.sums_un, n);
  } else {
    hipLaunchKernelGGL(certify_enum_kernel, dim3((unsigned)n), dim3(256), 0, s, a.stem_lo, a.stem_hi, a.feat_lo, a.t1, a.t2, a.t3w,
                       a.A, a.c0, a.classes, a.enum_bits, a.min_margin, rows, a.sums, n);
  }
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_certify_patch(const PatchArgs &p, int step, hipStream_t s) {
  const CertifyArgs &a = p.clean;
  if (step == kPatchBase) {
    TT_TRY(launch_certify(a, kCertifyStem, s));
    TT_TRY(launch_certify(a, kCertifyBlock, s));
    return launch_certify(a, kCertifyMargin, s);
  }
  const PatchGeom g{p.patch_h, p.patch_w, p.stride, p.amp, p.py, p.px};
  const long long tasks = (long long)a.n * p.py * p.px;
  for (long long l = 0; l < part::patch_launches(tasks); ++l)
    hipLaunchKernelGGL(certify_patch_kernel, dim3((unsigned)part::patch_launch_size(tasks, l)), dim3(256), 0, s, a.x, a.norm, a.w, a.bias,
                       a.stem_bn, a.slack, a.stem_lo, a.stem_hi, a.feat_lo, a.feat_hi, a.t1, a.t2, a.t3w, a.A, a.c0, a.classes, a.sums,
                       a.sums_un, (const Row *)a.rows, g, a.enum_bits, a.min_margin, (MapRec *)p.map, l * part::kPatchGrid, tasks);
  hipLaunchKernelGGL(certify_patch_rows_kernel, dim3((unsigned)a.n), dim3(256), 0, s, (const MapRec *)p.map, (PatchRow *)p.rows,
                     p.py * p.px, a.n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

}  // namespace ttnet
