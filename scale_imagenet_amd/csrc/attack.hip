// Falsified L-infinity robustness of TT_FHE_XSMALL_vAlexnet: the search for uint8 witnesses (include/ttnet.h:
// ttnet_attack_propose_u8, ttnet_attack_select_u8; DESIGN: falsified robustness).
//
//   attack_wsum_kernel     Wsum[ch][k][5][5]: the nine 3x3 stem kernels shifted over the MaxPool(3) window and summed; once
//                          per loaded state, next to the effective head A of certify.hip
//   attack_propose_kernel  one workgroup per image: the flip gain of every unknown stem bit (the tables read at
//                          index ^ mask, at most 21 features per bit), the push per bit, the two score maps by a gather of
//                          at most 256 terms per byte, and the eight candidates
//   attack_select_kernel   one workgroup per image: the margin of every candidate's logits in float32, the smallest wins
//                          and becomes x_cur, the record is updated
//
// Float64 sums in a fixed order (the build switches floating-point contraction off for every file), integer work, maxima:
// the same input gives the same bytes, and the numpy twin (attack.py) the same bytes again.

#include <math.h>

#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

using namespace va;

namespace {

constexpr int kCand = 8;

struct Row {            // one record of ttnet_attack_select_u8, 32 bytes
  float margin0, best;
  int32_t worst, status, round, changed, linf, tried;
};
static_assert(sizeof(Row) == 32, "record layout of include/ttnet.h");

// Wsum[ch][k][r][q] = sum over the pooling positions (dy, dx ascending) of w[ch][k][r - dy][q - dx]
__global__ void attack_wsum_kernel(const float *__restrict__ w, double *__restrict__ wsum) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= kWsum) return;
  const int q = t % 5, r = (t / 5) % 5, ck = t / 25;
  double acc = 0.0;
  for (int dy = 0; dy < 3; ++dy)
    for (int dx = 0; dx < 3; ++dx) {
      const int kh = r - dy, kw = q - dx;
      if (kh >= 0 && kh < 3 && kw >= 0 && kw < 3) acc += (double)w[ck * 9 + kh * 3 + kw];
    }
  wsum[t] = acc;
}

// The cells (pooled rows or columns) whose 5-wide field holds image row / column v, ascending, and v's offset in each field
// (-1: no such cell).  Field of cell p: 3 p - 1 .. 3 p + 3.  Row and column 31 lie in no field.
__device__ inline void cells_of(int v, int cell[2], int off[2]) {
  const int hi = (v + 1) / 3;
  cell[0] = hi - 1;
  cell[1] = hi;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    off[a] = v - 3 * cell[a] + 1;
    if (cell[a] < 0 || cell[a] >= kPool || off[a] < 0 || off[a] > 4) off[a] = -1;
  }
}

__global__ __launch_bounds__(256) void attack_propose_kernel(
    const uint8_t *__restrict__ x0, const uint8_t *__restrict__ xcur, const int32_t *__restrict__ classes,
    const int32_t *__restrict__ worst, const int32_t *__restrict__ active, const uint64_t *__restrict__ stem,
    const uint64_t *__restrict__ feat, const uint64_t *__restrict__ plane_lo, const uint64_t *__restrict__ plane_hi,
    const uint32_t *__restrict__ t1, const uint32_t *__restrict__ t2, const uint64_t *__restrict__ t3w,
    const double *__restrict__ A, const double *__restrict__ bn_scale, const double *__restrict__ wsum, int levels,
    uint8_t *__restrict__ cand, double *__restrict__ gains, int n) {
  __shared__ double s_wt[kStemBits];                                 // the push of every stem bit in mode 1 (50 KiB)
  __shared__ uint16_t s_bit[kStemRows], s_un[kStemRows], s_neg[kStemRows];   // per stem row: the bits, the unknown ones, those with g < 0
  __shared__ double s_max[2][4];
  const int img = blockIdx.x, tid = threadIdx.x;
  if (img >= n) return;                                              // (whole workgroups: no barrier is left behind)
  const int c = classes[img], j = worst[img];
  const bool live = active[img] != 0 && c >= 0 && c < kClasses && j >= 0 && j < kClasses && j != c;
  const uint8_t *cur = xcur + (size_t)img * kImg;
  uint8_t *out = cand + (size_t)img * kCand * kImg;
  if (!live) {                                                       // eight copies: the geometry of a round does not depend on the data
    for (int i = tid; i < kImg; i += 256) {
      const uint8_t b = cur[i];
#pragma unroll
      for (int k = 0; k < kCand; ++k) out[(size_t)k * kImg + i] = b;
    }
    if (gains)
      for (int i = tid; i < kStemBits; i += 256) gains[(size_t)img * kStemBits + i] = 0.0;
    return;
  }
  for (int r = tid; r < kStemRows; r += 256) {
    const size_t g = (size_t)img * kStemRows + r;
    s_bit[r] = (uint16_t)(stem[g] & 0x3FFull);
    s_un[r] = (uint16_t)((plane_lo[g] ^ plane_hi[g]) & 0x3FFull);
  }
  __syncthreads();
  // ---- flip gains: thread = stem row (channel, pooled row) ------------------------------------------------------------------
  const uint64_t *fy = feat + (size_t)img * kFeatRows;
  auto row1 = [&](int ch, int y) {                                   // a stem row of the forward, shifted
    return shifted_row(y, [&](int iy) { return (uint32_t)s_bit[ch * kPool + iy]; });
  };
  for (int r = tid; r < kStemRows; r += 256) {
    const int ch = r / kPool, py = r - kPool * ch;
    const uint64_t T1 = table_word(t1, ch), T2 = table_word(t2, ch);
    const double sgn = bn_scale[ch] >= 0.0 ? 1.0 : -1.0;
    uint32_t neg = 0;
    for (int px = 0; px < kPool; ++px) {
      double g = 0.0;
      if ((s_un[r] >> px) & 1u) {
        // The 21 features of va_block.h's reach(), in its order, written out as three nests: one loop over reach(ch, py, px, t)
        // gives the same sums but a propose step 17 % slower (profiles/va_block_refactor.txt).
        auto term = [&](int fc, int oy, int ox, int ynew, int yold) {  // +D_f, -D_f or nothing
          if (ynew != yold) {
            const size_t f = (size_t)(fc * kPlane + oy * kSide + ox) * kClasses;
            const double d = A[f + c] - A[f + j];
            g += ynew > yold ? d : -d;
          }
        };
        auto old = [&](int fc, int oy, int ox) { return (int)((fy[fc * kSide + oy] >> ox) & 1ull); };
        for (int doy = -1; doy <= 1; ++doy) {                        // conv1: rows oy-1..oy+1, columns ox-1..ox; oy <= 9
          const int oy = py + doy;
          if (oy < 0 || oy >= kPool) continue;
          const uint32_t l0 = row1(ch, oy - 1), l1 = row1(ch, oy), l2 = row1(ch, oy + 1);
          for (int dox = 0; dox <= 1; ++dox) {
            const int ox = px + dox;
            const uint32_t fl = conv1_index(l0, l1, l2, ox) ^ (1u << ((1 - doy) * 2 + (1 - dox)));
            term(ch, oy, ox, (int)((T1 >> fl) & 1ull), old(ch, oy, ox));
          }
        }
        for (int doy = 0; doy <= 1; ++doy) {                         // conv2: rows oy-1..oy, columns ox-1..ox+1; ox <= 9
          const int oy = py + doy;
          const uint32_t l0 = row1(ch, oy - 1), l1 = row1(ch, oy);
          for (int dox = -1; dox <= 1; ++dox) {
            const int ox = px + dox;
            if (ox < 0 || ox >= kPool) continue;
            const uint32_t fl = conv2_index(l0, l1, ox) ^ (1u << ((1 - doy) * 3 + (1 - dox)));
            term(64 + ch, oy, ox, (int)((T2 >> fl) & 1ull), old(64 + ch, oy, ox));
          }
        }
        uint32_t grp[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) grp[k] = s_bit[((ch & ~7) + k) * kPool + py];
        const uint32_t fl = conv3_index(grp, px) ^ (1u << (ch & 7));
        for (int o = 0; o < 8; ++o) {                                // conv3: the 8 outputs of the group
          const int fc = 128 + (ch & ~7) + o;
          term(fc, py, px, (int)((t3w[(fc - 128) * 4 + (fl >> 6)] >> (fl & 63u)) & 1ull), old(fc, py, px));
        }
        const int bit = (s_bit[r] >> px) & 1;
        term(192 + ch, py, px, 1 - bit, bit);                        // out4 carries the bit itself
        s_wt[r * kPool + px] = -g * (bit == 0 ? 1.0 : -1.0) * sgn;
        neg |= (uint32_t)(g < 0.0) << px;
      } else {
        s_wt[r * kPool + px] = 0.0;
      }
      if (gains) gains[(size_t)img * kStemBits + r * kPool + px] = g;
    }
    s_neg[r] = (uint16_t)neg;
  }
  __syncthreads();
  // ---- pixel scores: thread = pixels tid, tid + 256, ..; both modes and the three colour channels in registers ----------------
  double sc[4][2][3];
  double mx[2] = {0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + 256 * i, y = p >> 5, x = p & 31;
    int cy[2], oy[2], cx[2], ox[2];
    cells_of(y, cy, oy);
    cells_of(x, cx, ox);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int k = 0; k < 3; ++k) sc[i][m][k] = 0.0;
    for (int ch = 0; ch < kStemCh; ++ch)                             // ch ascending, then py, then px
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          if (oy[a] < 0 || ox[b] < 0) continue;
          const double w1 = s_wt[(ch * kPool + cy[a]) * kPool + cx[b]];
          if (w1 == 0.0) continue;                                   // (a zero term changes no sum: the sums are never -0)
          const double w0 = ((s_neg[ch * kPool + cy[a]] >> cx[b]) & 1u) ? w1 : 0.0;
          const double *W = wsum + (size_t)ch * 75 + oy[a] * 5 + ox[b];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double wk = W[k * 25];
            sc[i][0][k] += w0 * wk;
            sc[i][1][k] += w1 * wk;
          }
        }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int k = 0; k < 3; ++k) mx[m] = fmax(mx[m], fabs(sc[i][m][k]));
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {                                      // M = max |score| of the image and mode (any order gives the same)
    for (int d = 32; d >= 1; d >>= 1) mx[m] = fmax(mx[m], __shfl_xor(mx[m], d));
    if ((tid & 63) == 0) s_max[m][tid >> 6] = mx[m];
  }
  __syncthreads();
  double M[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) M[m] = fmax(fmax(s_max[m][0], s_max[m][1]), fmax(s_max[m][2], s_max[m][3]));
  // ---- candidates: index 4 mode + tau index ---------------------------------------------------------------------------------------
  constexpr double kTau[4] = {0.0, 0.125, 0.25, 0.5};
  const uint8_t *org = x0 + (size_t)img * kImg;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + 256 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int at = 3 * p + k;
      const int b0 = org[at];
      const uint8_t keep = cur[at], up = (uint8_t)min(255, b0 + levels), dn = (uint8_t)max(0, b0 - levels);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const double s = sc[i][m][k];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const bool sel = s != 0.0 && fabs(s) > kTau[t] * M[m];
          out[(size_t)(4 * m + t) * kImg + at] = sel ? (s > 0.0 ? up : dn) : keep;
        }
      }
    }
  }
}

// One workgroup per image.  Threads 0 .. n_cand - 1 take the margins, thread 0 decides, all copy the winner and recount.
__global__ __launch_bounds__(256) void attack_select_kernel(const uint8_t *__restrict__ cand, const float *__restrict__ logits,
                                                            int n_cand, const int32_t *__restrict__ classes, float min_margin,
                                                            const uint8_t *__restrict__ x0, uint8_t *__restrict__ xcur,
                                                            Row *__restrict__ rows, int32_t *__restrict__ worst,
                                                            int32_t *__restrict__ active, int round, int n) {
  __shared__ float s_m[kCand];
  __shared__ int s_j[kCand];                                         // the runner-up of candidate k; -1: skipped (a NaN logit)
  __shared__ int s_pick, s_changed, s_linf;
  __shared__ Row s_row;
  const int img = blockIdx.x, tid = threadIdx.x;
  if (img >= n) return;
  const int c = classes[img];
  const bool valid = c >= 0 && c < kClasses;
  const uint8_t *org = x0 + (size_t)img * kImg;
  uint8_t *cur = xcur + (size_t)img * kImg;
  if (round == 0)
    for (int i = tid; i < kImg; i += 256) cur[i] = org[i];           // (each thread rewrites its own bytes below: program order)
  if (tid < n_cand) {
    int bj = -1;
    float m = 0.f;
    if (valid) {
      const float *l = logits + ((size_t)img * n_cand + tid) * kClasses;
      bool nan = false;
      float top = 0.f;
      for (int q = 0; q < kClasses; ++q) {
        nan = nan || isnan(l[q]);
        if (q != c && (bj < 0 || l[q] > top)) {                      // the first of equal maxima
          top = l[q];
          bj = q;
        }
      }
      m = l[c] - top;
      if (nan) bj = -1;
    }
    s_m[tid] = m;
    s_j[tid] = bj;
  }
  __syncthreads();
  if (tid == 0) {
    Row r;
    bool act;
    if (round == 0) {
      r.margin0 = NAN;
      r.best = INFINITY;
      r.worst = -1;
      r.status = r.round = r.changed = r.linf = r.tried = 0;
      act = valid;
      if (!valid) r.margin0 = r.best = -INFINITY;                    // as the certificate treats a class outside 0..9
      worst[img] = -1;
    } else {
      r = rows[img];
      act = active[img] != 0;
    }
    int pick = -1;
    if (act) {
      float bm = INFINITY;
      for (int k = 0; k < n_cand; ++k) {
        if (s_j[k] < 0) continue;
        if (round == 0 && k == 0) r.margin0 = s_m[k];
        if (s_m[k] < bm) {                                           // the smallest margin; ties: the lowest index
          bm = s_m[k];
          pick = k;
        }
      }
      r.tried += n_cand;
      if (pick >= 0 && !(bm < r.best)) pick = -1;
      if (pick >= 0) {
        r.best = bm;
        r.worst = s_j[pick];
        r.round = round;
        worst[img] = s_j[pick];
        if (bm < -min_margin) {
          r.status = round == 0 ? 1 : 2;
          act = false;
        }
      }
    }
    if (round == 0 || pick >= 0) active[img] = act ? 1 : 0;
    s_row = r;
    s_pick = pick;
    s_changed = s_linf = 0;
  }
  __syncthreads();
  const int pick = s_pick;
  if (pick >= 0) {
    const uint8_t *win = cand + ((size_t)img * n_cand + pick) * kImg;
    int changed = 0, linf = 0;
    for (int i = tid; i < kImg; i += 256) {
      const int b = win[i], d = abs(b - (int)org[i]);
      cur[i] = (uint8_t)b;
      changed += d != 0;
      linf = max(linf, d);
    }
    atomicAdd(&s_changed, changed);                                  // (integers: any order gives the same)
    atomicMax(&s_linf, linf);
    __syncthreads();
  }
  if (tid == 0) {
    if (pick >= 0) {
      s_row.changed = s_changed;
      s_row.linf = s_linf;
    }
    rows[img] = s_row;
  }
}

}  // namespace

int launch_attack_wsum(const float *w, double *wsum, hipStream_t s) {
  hipLaunchKernelGGL(attack_wsum_kernel, dim3((kWsum + 255) / 256), dim3(256), 0, s, w, wsum);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_attack_propose(const AttackProposeArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(attack_propose_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a.x0, a.xcur, a.classes, a.worst, a.active, a.stem,
                     a.feat, a.plane_lo, a.plane_hi, a.t1, a.t2, a.t3w, a.A, a.bn_scale, a.wsum, a.levels, a.cand, a.gains, a.n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_attack_select(const uint8_t *cand, const float *logits, int n, int n_cand, const int32_t *classes, float min_margin,
                         const uint8_t *x0, uint8_t *xcur, void *rows, int32_t *worst, int32_t *active, int round, hipStream_t s) {
  hipLaunchKernelGGL(attack_select_kernel, dim3((unsigned)n), dim3(256), 0, s, cand, logits, n_cand, classes, min_margin, x0, xcur,
                     (Row *)rows, worst, active, round, n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

}  // namespace ttnet
