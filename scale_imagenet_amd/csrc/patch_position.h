// One (image, position) of a patch, evaluated: the steps that the certified sweep (certify.hip: certify_patch_kernel) and the
// patch search (attack.hip: attack_patch_kernel) both take, each written once.  A workgroup of 256 threads holds the image's
// stem planes in LDS as (values, unknown bits) words [640] and
//   load_patch_window   the pixels of the fields that meet the patch, as centres and radii
//   stem_row_pass       thread (channel, cell row) runs certify_stem_cell.inc over the span's columns
//   rewrite_stem_row    .. and rewrites its words of the planes with what the cells became
//   reached_sums        every feature those cells reach, looked up on the planes; its difference against the clean feature
//                       planes, summed per class into part[wave][..]
//   patch_margin        lb_j from the clean sums and part, the smallest wins
// The order of every sum is part of the contract: the twins (certify.py, attack.py) give the same bytes.
#pragma once

#include <math.h>

#include "certify_lookup.h"
#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

// task = image * P + position: the patch's corner and the spans of pooled cells whose 5-wide fields meet it
struct PatchPos {
  int img, pos, y0, x0;
  va::FieldSpan fr, fq;
  __device__ bool touched() const { return fr.count > 0 && fq.count > 0; }
};
__device__ inline PatchPos patch_pos(long long task, const PatchGeom &g) {
  const int P = g.py * g.px, img = (int)(task / P), pos = (int)(task - (long long)img * P);
  const int y0 = (pos / g.px) * g.stride, x0 = (pos % g.px) * g.stride;
  return {img, pos, y0, x0, va::field_span(y0, g.h), va::field_span(x0, g.w)};
}

// an image's stem planes into LDS as (values, unknown bits) words.  The caller's barrier follows.
__device__ inline void load_stem_planes(uint64_t *s_lo, uint64_t *s_un, const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi,
                                        int img, int tid) {
  for (int r = tid; r < va::kStemRows; r += 256) {
    const uint64_t l = slo[(size_t)img * va::kStemRows + r];
    s_lo[r] = l;
    s_un[r] = (l ^ shi[(size_t)img * va::kStemRows + r]) & 0x3FFull;
  }
}

// centre [0] and radius [1] of the normalised pixels of the touched fields: rows 3 fr.first - 1 .., columns 3 fq.first - 1 ..
using PatchWindow = double[2][3][va::kFieldPixels][va::kFieldPixels];

// The bytes inside the patch come from the box [max(0, b - amp), min(255, b + amp)] (fill == nullptr) or from `fill` at radius 0
// (the patch row-major (y, x, channel)); every other byte is exact.  The caller's barrier follows.
__device__ inline void load_patch_window(PatchWindow &win, const uint8_t *__restrict__ x, const CertifyNorm &nm, const PatchPos &p,
                                         const PatchGeom &g, const uint8_t *fill, int tid) {
  using namespace va;
  if (!p.touched()) return;
  const int wr_n = 3 * p.fr.count + 2, wq_n = 3 * p.fq.count + 2;    // <= kFieldPixels
  for (int i = tid; i < 3 * wr_n * wq_n; i += 256) {
    const int k = i % 3, lq = (i / 3) % wq_n, lr = i / (3 * wq_n), ir = 3 * p.fr.first - 1 + lr, iq = 3 * p.fq.first - 1 + lq;   // ir, iq <= 30
    double centre = 0.0, radius = 0.0;                               // the top / left padding: zero in normalised space
    if (ir >= 0 && iq >= 0) {
      const int b = x[(size_t)p.img * kImg + (ir * 32 + iq) * 3 + k];
      const bool in = ir >= p.y0 && ir < p.y0 + g.h && iq >= p.x0 && iq < p.x0 + g.w;
      int bl = b, bh = b;
      if (in && !fill) {
        bl = b - g.amp > 0 ? b - g.amp : 0;
        bh = b + g.amp < 255 ? b + g.amp : 255;
      } else if (in) {
        bl = bh = fill[((ir - p.y0) * g.w + (iq - p.x0)) * 3 + k];
      }
      pixel_interval((double)bl, (double)bh, nm, k, centre, radius);
    }
    win[0][k][lr][lq] = centre;
    win[1][k][lr][lq] = radius;
  }
}

// Channel ch's cells of row cy of the span, columns 0 .. ncols - 1, from the window: cell(cx, lo_bit, hi_bit) for each.  The one
// place besides certify_stem_kernel that includes the cell's text, so a cell has the same bits whoever computes it.
template <class Cell>
__device__ inline void stem_row_pass(const PatchWindow &win, int ch, int cy, int ncols, const float *__restrict__ w,
                                     const float *__restrict__ bias, const double *__restrict__ bn, const double *__restrict__ slack,
                                     Cell &&cell) {
  double wr[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) wr[i] = (double)w[ch * 27 + i];
  const double b = (double)bias[ch], sc = bn[ch], sh = bn[64 + ch], sl = slack[ch];
#pragma unroll 1
  for (int cx = 0; cx < ncols; ++cx) {
#define STEM_AT(k, c, r, q) win[k][c][3 * cy + (r)][3 * cx + (q)]
#include "certify_stem_cell.inc"
#undef STEM_AT
    cell(cx, lo_bit, hi_bit);
  }
}

// Thread tid < 64 * fr.count = (channel, cell row) of a touched position rewrites word r = its row of the planes with the cells
// of the span as the window gives them.  The caller counts what it needs from the words before and after.
__device__ inline void rewrite_stem_row(uint64_t *s_lo, uint64_t *s_un, int r, const PatchWindow &win, int ch, int cy, va::FieldSpan fq,
                                        const float *__restrict__ w, const float *__restrict__ bias, const double *__restrict__ bn,
                                        const double *__restrict__ slack) {
  uint64_t lo_w = s_lo[r], un_w = s_un[r];
  stem_row_pass(win, ch, cy, fq.count, w, bias, bn, slack, [&](int cx, bool lo_bit, bool hi_bit) {
    const int px = fq.first + cx;
    lo_w = (lo_w & ~(1ull << px)) | ((uint64_t)lo_bit << px);
    un_w = (un_w & ~(1ull << px)) | ((uint64_t)(lo_bit != hi_bit) << px);
  });
  s_lo[r] = lo_w;
  s_un[r] = un_w;
}

// Every feature of the four rectangles that the span's cells reach, looked up on the planes; where it differs from the clean
// feature planes its contribution changes.  Thread t sums the differences of the features t, t + 256, .. of a branch (branches
// in order), the 64 lanes of a wave meet by shuffles (xor 32, 16, .., 1) and leave part[wave][j] (the certain part) and
// part[wave][10 + j] (the unknown part); patch_margin adds the four waves in order.  `live` (uniform): false leaves zeros.
// The caller's barrier follows.
__device__ inline void reached_sums(const uint64_t *s_lo, const uint64_t *s_un, const PatchPos &p, int c, bool live,
                                    const uint64_t *__restrict__ ylo, const uint64_t *__restrict__ yhi, const uint32_t *__restrict__ t1,
                                    const uint32_t *__restrict__ t2, const uint64_t *__restrict__ t3w, const double *__restrict__ A,
                                    double (&part)[4][2 * va::kClasses], int tid) {
  using namespace va;
  double acc[2 * kClasses];
#pragma unroll
  for (int j = 0; j < 2 * kClasses; ++j) acc[j] = 0.0;
  if (live)
    for (int kind = 0; kind < 4; ++kind) {
      const FeatRect rc = reached_rect(kind, p.fr, p.fq);
      for (int e = tid; e < 64 * rc.nr * rc.nc; e += 256) {
        const int ch = e & 63, cell = e >> 6, oy = rc.r0 + cell / rc.nc, ox = rc.c0 + cell % rc.nc, fc = 64 * kind + ch;
        bool lo, hi;
        feature3(s_lo, s_un, kind, ch, oy, ox, t1, t2, t3w, lo, hi);
        const size_t row = (size_t)p.img * kFeatRows + fc * kSide + oy;
        const bool clo = (ylo[row] >> ox) & 1ull, chi = (yhi[row] >> ox) & 1ull;
        if (lo == clo && hi == chi) continue;
        const double *af = A + (size_t)(fc * kPlane + oy * kSide + ox) * kClasses;
        const double ac = af[c];
#pragma unroll
        for (int j = 0; j < kClasses; ++j) {
          const double d = ac - af[j], m = fmin(0.0, d);
          acc[j] += (lo ? d : 0.0) - (clo ? d : 0.0);
          acc[kClasses + j] += ((hi && !lo) ? m : 0.0) - ((chi && !clo) ? m : 0.0);
        }
      }
    }
#pragma unroll
  for (int j = 0; j < 2 * kClasses; ++j) {
    double v = acc[j];
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if ((tid & 63) == 0) part[tid >> 6][j] = v;
  }
}

// One thread, between two barriers: lb_j = c0_c - c0_j + ((S_j + dS_j) + (U_j + dU_j)) with the clean sums S, U of the image and
// their changes from part; the smallest lb and its j win, ties go to the first j.  A class outside 0..9 gives -inf and j = -1.
// pos_sums (optional): S_j + dS_j of every class, c included, what stage 2 starts from.  (Without it the loads of class c are dead
// code and the compiler drops them: the search's listing is the same with the class skipped by hand.)
__device__ inline void patch_margin(const double (&part)[4][2 * va::kClasses], const double *__restrict__ sums,
                                    const double *__restrict__ sums_un, const double *__restrict__ c0, int img, int c, double &lb,
                                    int &worst, double *pos_sums = nullptr) {
  using namespace va;
  const bool valid = c >= 0 && c < kClasses;
  double best = valid ? INFINITY : -INFINITY;
  int best_j = -1;
  for (int j = 0; j < kClasses && valid; ++j) {
    const double cert = sums[(size_t)img * kClasses + j] + (((part[0][j] + part[1][j]) + part[2][j]) + part[3][j]);
    const double unk = sums_un[(size_t)img * kClasses + j] + (((part[0][kClasses + j] + part[1][kClasses + j]) + part[2][kClasses + j]) + part[3][kClasses + j]);
    if (pos_sums) pos_sums[j] = cert;
    if (j == c) continue;
    const double cand = c0[c] - c0[j] + (cert + unk);
    if (cand < best) {
      best = cand;
      best_j = j;
    }
  }
  lb = best;
  worst = best_j;
}

}  // namespace ttnet
