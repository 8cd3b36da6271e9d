// Three-valued lookups of TT_FHE_XSMALL_vAlexnet's block and the geometry of a patch's reach, shared by the certificate
// (certify.hip) and the patch search (attack.hip): the selector words, one feature on three-valued stem planes, the rectangle
// of features that a span of pooled cells reaches, and the interval of a byte in normalised space.
#pragma once

#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

// the entries of a 64-entry table that agree with the known inputs: `lo` holds the known values, `un` marks the unknown
// inputs (bits 0..5).  M[p] = the indices whose bit p is 1.
__device__ inline uint64_t selector(uint32_t lo, uint32_t un) {
  constexpr uint64_t M[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                             0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
  uint64_t S = ~0ull;
#pragma unroll
  for (int p = 0; p < 6; ++p) S &= ((un >> p) & 1u) ? ~0ull : (((lo >> p) & 1u) ? M[p] : ~M[p]);
  return S;
}

// centre and radius of the normalised interval of a byte of channel c that may take any value in [bl, bh]:
// w+ x_lo + w- x_hi = w x_c - |w| x_r and w+ x_hi + w- x_lo = w x_c + |w| x_r, two multiply-adds per tap where the bounds
// themselves take four and a choice by the sign of w
__device__ inline void pixel_interval(double bl, double bh, const CertifyNorm &nm, int c, double &centre, double &radius) {
  const double xl = (bl - nm.off[c]) * nm.a[c], xh = (bh - nm.off[c]) * nm.a[c];
  centre = 0.5 * (xl + xh);
  radius = 0.5 * (xh - xl);
}

// can0 / can1 of one output bit of a 256-entry table (four words): inputs 6 and 7 pick the words, inputs 0..5 the selector
__device__ inline void lookup8(const uint64_t *T, uint32_t lo, uint32_t un, bool &can0, bool &can1) {
  const uint64_t S = selector(lo, un);
  can0 = can1 = false;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const bool ok = (((un >> 6) & 1u) || ((lo >> 6) & 1u) == (uint32_t)(w & 1)) && (((un >> 7) & 1u) || ((lo >> 7) & 1u) == (uint32_t)(w >> 1));
    if (!ok) continue;
    can1 = can1 || (T[w] & S) != 0;
    can0 = can0 || (~T[w] & S) != 0;
  }
}

// One feature on three-valued stem planes held as (values, unknown bits) words [640]: what certify_dw_kernel and
// certify_c3_kernel give that feature, by the generic window (window_input).  The caller keeps (oy, ox) inside the plane
// that the branch computes (conv1: oy < 10; conv2: ox < 10; conv3 / out4: both < 10).
__device__ inline void feature3(const uint64_t *s_lo, const uint64_t *s_un, int kind, int ch, int oy, int ox, const uint32_t *__restrict__ t1,
                                const uint32_t *__restrict__ t2, const uint64_t *__restrict__ t3w, bool &lo, bool &hi) {
  using namespace va;
  uint32_t idx = 0, un = 0;
  for (int p = 0; p < window_size(kind); ++p) {
    const StemBit s = window_input(kind, ch, oy, ox, p);
    if (!s.in) continue;
    const int r = s.ch * kPool + s.y;
    idx |= (uint32_t)((s_lo[r] >> s.x) & 1ull) << p;
    un |= (uint32_t)((s_un[r] >> s.x) & 1ull) << p;
  }
  idx &= ~un;
  if (kind < 2) {
    const uint64_t T = table_word(kind == 0 ? t1 : t2, ch), S = selector(idx, un);
    lo = (~T & S) == 0;
    hi = (T & S) != 0;
  } else if (kind == 2) {
    bool can0, can1;
    lookup8(t3w + ch * 4, idx, un, can0, can1);                      // (ch = 8 group + output)
    lo = !can0;
    hi = can1;
  } else {
    lo = idx & 1u;
    hi = (idx | un) & 1u;
  }
}

// a patch sweep's geometry: the patch, the stride, the amplitude, the positions down and across
struct PatchGeom {
  int h, w, stride, amp, py, px;
};

// the features of branch `kind` that the cells rows x cols reach: a rectangle of its plane (inside what the branch computes)
struct FeatRect {
  int r0, nr, c0, nc;
};
__device__ inline FeatRect reached_rect(int kind, va::FieldSpan rows, va::FieldSpan cols) {
  using namespace va;
  int r0 = rows.first, r1 = rows.last(), q0 = cols.first, q1 = cols.last();
  if (kind == 0) {                   // conv1: window rows oy - 1 .. oy + 1, columns ox - 1 .. ox; 10 x 11 outputs
    r0 = r0 > 0 ? r0 - 1 : 0;
    r1 = r1 + 1 < kPool ? r1 + 1 : kPool - 1;
    q1 = q1 + 1;                     // <= 10
  } else if (kind == 1) {            // conv2: window rows oy - 1 .. oy, columns ox - 1 .. ox + 1; 11 x 10 outputs
    r1 = r1 + 1;                     // <= 10
    q0 = q0 > 0 ? q0 - 1 : 0;
    q1 = q1 + 1 < kPool ? q1 + 1 : kPool - 1;
  }
  return {r0, r1 - r0 + 1, q0, q1 - q0 + 1};
}

}  // namespace ttnet
