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
//   attack_patch_kernel    the patch search (ttnet_attack_patch_u8): one workgroup per (image, position); the movable stem bits
//                          are those the position's box leaves unknown, a candidate fill is judged by its predicted margin
//                          m_pred -- the steps of patch_position.h, which the certified sweep takes too, on a fill at radius
//                          0 -- and the gains, pushes and scores of the propose step choose the candidates
//   patch_paste_kernel     witnesses as images: a fill pasted into its image (ttnet_patch_paste_u8)
//
// The steps of a proposal are written once, for both searches: flip_gain and stem_push, cells_of, and candidate_byte (which states
// the thresholds).  score_terms and block_max2 serve the propose kernel; the patch search keeps its own score loop and block
// maximum, one byte per thread: with the shared forms it was 0.8 - 1.5 % slower (profiles/patch_steps_refactor.txt, section 4).
//
// Float64 sums in a fixed order (the build switches floating-point contraction off for every file), integer work, maxima:
// the same input gives the same bytes, and the numpy twin (attack.py) the same bytes again.

#include <math.h>

#include "certify_lookup.h"
#include "partition.h"
#include "patch_position.h"
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

// The flip gain of stem bit (ch, py, px): the change of logit_c - logit_j when it alone flips.  row(ch, y) gives the 10 bits of a stem
// row; old(kind, fc, oy, ox, at) the bit of feature (fc, oy, ox) of branch `kind` before the flip, `at` being its unflipped table
// index.  The 21 features of va_block.h's reach(), in its order, written out as three nests: one loop over reach(ch, py, px, t)
// gives the same sums but a propose step 12 - 17 % slower (profiles/va_block_refactor.txt, section 3).
template <class RowFn, class OldFn>
__device__ inline double flip_gain(int ch, int py, int px, RowFn row, OldFn old, uint64_t T1, uint64_t T2, const uint64_t *__restrict__ t3w,
                                   const double *__restrict__ A, int c, int j) {
  double g = 0.0;
  auto term = [&](int fc, int oy, int ox, int ynew, int yold) {      // +D_f, -D_f or nothing
    if (ynew != yold) {
      const size_t f = (size_t)(fc * kPlane + oy * kSide + ox) * kClasses;
      const double d = A[f + c] - A[f + j];
      g += ynew > yold ? d : -d;
    }
  };
  auto row1 = [&](int y) { return shifted_row(y, [&](int iy) { return row(ch, iy); }); };
  for (int doy = -1; doy <= 1; ++doy) {                              // conv1: rows oy-1..oy+1, columns ox-1..ox; oy <= 9
    const int oy = py + doy;
    if (oy < 0 || oy >= kPool) continue;
    const uint32_t l0 = row1(oy - 1), l1 = row1(oy), l2 = row1(oy + 1);
    for (int dox = 0; dox <= 1; ++dox) {
      const int ox = px + dox;
      const uint32_t at = conv1_index(l0, l1, l2, ox), fl = at ^ (1u << ((1 - doy) * 2 + (1 - dox)));
      term(ch, oy, ox, (int)((T1 >> fl) & 1ull), old(0, ch, oy, ox, at));
    }
  }
  for (int doy = 0; doy <= 1; ++doy) {                               // conv2: rows oy-1..oy, columns ox-1..ox+1; ox <= 9
    const int oy = py + doy;
    const uint32_t l0 = row1(oy - 1), l1 = row1(oy);
    for (int dox = -1; dox <= 1; ++dox) {
      const int ox = px + dox;
      if (ox < 0 || ox >= kPool) continue;
      const uint32_t at = conv2_index(l0, l1, ox), fl = at ^ (1u << ((1 - doy) * 3 + (1 - dox)));
      term(64 + ch, oy, ox, (int)((T2 >> fl) & 1ull), old(1, 64 + ch, oy, ox, at));
    }
  }
  uint32_t grp[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) grp[k] = row((ch & ~7) + k, py);
  const uint32_t at = conv3_index(grp, px), fl = at ^ (1u << (ch & 7));
  for (int o = 0; o < 8; ++o) {                                      // conv3: the 8 outputs of the group
    const int fc = 128 + (ch & ~7) + o;
    term(fc, py, px, (int)((t3w[(fc - 128) * 4 + (fl >> 6)] >> (fl & 63u)) & 1ull), old(2, fc, py, px, at));
  }
  const int bit = (row(ch, py) >> px) & 1;
  term(192 + ch, py, px, 1 - bit, bit);                              // out4 carries the bit itself
  return g;
}

// the push of a stem bit of gain g in mode 1: towards the flip where the flip lowers the margin; sgn = the sign of the channel's bn_scale
__device__ inline double stem_push(double g, int bit, double sgn) { return -g * (bit == 0 ? 1.0 : -1.0) * sgn; }

// The terms of the score of the bytes of pixel (y, x): ch ascending, then the two row cells, then the two column cells.  A cell
// (ch, py, px) with push(..) = w1 != 0 adds w1 W[25 k] to byte k in mode 1 and, where negative(..), in mode 0 too: add(w0, w1, W)
// with W = the cell's summed kernel at the pixel's offset in its field.  (A zero term changes no sum: the sums are never -0.)
template <class PushFn, class NegFn, class AddFn>
__device__ inline void score_terms(int y, int x, const double *__restrict__ wsum, PushFn push, NegFn negative, AddFn add) {
  int cy[2], oy[2], cx[2], ox[2];
  cells_of(y, cy, oy);
  cells_of(x, cx, ox);
  for (int ch = 0; ch < kStemCh; ++ch)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        if (oy[a] < 0 || ox[b] < 0) continue;
        const double w1 = push(ch, cy[a], cx[b]);
        if (w1 == 0.0) continue;
        add(negative(ch, cy[a], cx[b]) ? w1 : 0.0, w1, wsum + (size_t)ch * 75 + oy[a] * 5 + ox[b]);
      }
}

// M[m] = the workgroup's maximum of mx[m] (any order gives the same); every thread calls it: it holds a barrier
__device__ inline void block_max2(double mx[2], double (&s_max)[2][4], int tid, double M[2]) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    for (int d = 32; d >= 1; d >>= 1) mx[m] = fmax(mx[m], __shfl_xor(mx[m], d));
    if ((tid & 63) == 0) s_max[m][tid >> 6] = mx[m];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 2; ++m) M[m] = fmax(fmax(s_max[m][0], s_max[m][1]), fmax(s_max[m][2], s_max[m][3]));
}

// the byte of the candidate of threshold index t: selected when its score is not 0 and |score| > tau M (attack.py: TAUS)
__device__ inline uint8_t candidate_byte(double s, double M, int t, uint8_t up, uint8_t dn, uint8_t keep) {
  constexpr double kTau[4] = {0.0, 0.125, 0.25, 0.5};
  return (s != 0.0 && fabs(s) > kTau[t] * M) ? (s > 0.0 ? up : dn) : keep;
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
  auto row = [&](int ch, int y) { return (uint32_t)s_bit[ch * kPool + y]; };                                     // the forward's stem rows ..
  auto old = [&](int, int fc, int oy, int ox, uint32_t) { return (int)((fy[fc * kSide + oy] >> ox) & 1ull); };   // .. and its feature planes
  for (int r = tid; r < kStemRows; r += 256) {
    const int ch = r / kPool, py = r - kPool * ch;
    const uint64_t T1 = table_word(t1, ch), T2 = table_word(t2, ch);
    const double sgn = bn_scale[ch] >= 0.0 ? 1.0 : -1.0;
    uint32_t neg = 0;
    for (int px = 0; px < kPool; ++px) {
      double g = 0.0, wt = 0.0;
      if ((s_un[r] >> px) & 1u) {
        g = flip_gain(ch, py, px, row, old, T1, T2, t3w, A, c, j);
        wt = stem_push(g, (s_bit[r] >> px) & 1, sgn);
        neg |= (uint32_t)(g < 0.0) << px;
      }
      s_wt[r * kPool + px] = wt;
      if (gains) gains[(size_t)img * kStemBits + r * kPool + px] = g;
    }
    s_neg[r] = (uint16_t)neg;
  }
  __syncthreads();
  // ---- pixel scores: thread = pixels tid, tid + 256, ..; both modes and the three colour channels in registers ----------------
  double sc[4][2][3];
  double mx[2] = {0.0, 0.0}, M[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + 256 * i;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int k = 0; k < 3; ++k) sc[i][m][k] = 0.0;
    score_terms(p >> 5, p & 31, wsum, [&](int ch, int py, int px) { return s_wt[(ch * kPool + py) * kPool + px]; },
                [&](int ch, int py, int px) { return (s_neg[ch * kPool + py] >> px) & 1u; },
                [&](double w0, double w1, const double *W) {
#pragma unroll
                  for (int k = 0; k < 3; ++k) {
                    const double wk = W[k * 25];
                    sc[i][0][k] += w0 * wk;
                    sc[i][1][k] += w1 * wk;
                  }
                });
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int k = 0; k < 3; ++k) mx[m] = fmax(mx[m], fabs(sc[i][m][k]));
  }
  block_max2(mx, s_max, tid, M);                                     // M = max |score| of the image and mode
  // ---- candidates: index 4 mode + tau index ---------------------------------------------------------------------------------------
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
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) out[(size_t)(4 * m + t) * kImg + at] = candidate_byte(sc[i][m][k], M[m], t, up, dn, keep);
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

// ---- the patch search (include/ttnet.h: ttnet_attack_patch_u8) -------------------------------------------------------------------
constexpr int kFill = 3 * kPatchMax * kPatchMax;                     // bytes of a fill record
constexpr int kHashStream = 11;                                      // slot k of a round hashes stream 11 + k (attack.py: HASH_STREAM)

struct PatchRec {       // one (image, position) record, 16 bytes
  double m_pred;
  int32_t worst;
  uint16_t round, unknown;
};
static_assert(sizeof(PatchRec) == 16, "record layout of include/ttnet.h");

// bit 16 of a 32-bit integer mix of (position, round, stream, byte): attack.py's hash_corner
__device__ inline bool hash_corner(uint32_t pos, int rnd, int stream, uint32_t byte) {
  uint32_t v = pos * 0x9E3779B1u + (uint32_t)(rnd * 8 + stream) * 0x85EBCA6Bu + byte * 0xC2B2AE35u;
  v ^= v >> 15;
  v *= 0x2C1B3C6Du;
  v ^= v >> 12;
  v *= 0x297A2D39u;
  v ^= v >> 15;
  return (v >> 16) & 1u;
}

// One workgroup per (image, position); task = first_task + blockIdx.x = image * P + position.  Thread (channel, cell row) =
// tid < 64 * rows of cells owns one touched row of the stem planes, as in certify_patch_kernel; thread = byte of the patch for
// the scores and the candidates.  s_lo / s_un are the working planes: the clean planes with the touched rows of whatever fill is
// being judged; the touched rows of the current and of the round's best fill are kept apart (cur_*, best_*: 4 x 64 words each).
__global__ __launch_bounds__(256, 2) void attack_patch_kernel(
    const uint8_t *__restrict__ x, CertifyNorm nm, const float *__restrict__ w, const float *__restrict__ bias, const double *__restrict__ bn,
    const double *__restrict__ slack, const uint64_t *__restrict__ slo, const uint64_t *__restrict__ shi, const uint64_t *__restrict__ ylo,
    const uint64_t *__restrict__ yhi, const uint32_t *__restrict__ t1, const uint32_t *__restrict__ t2, const uint64_t *__restrict__ t3w,
    const double *__restrict__ A, const double *__restrict__ c0, const double *__restrict__ wsum, const int32_t *__restrict__ classes,
    const double *__restrict__ sums, const double *__restrict__ sums_un, PatchGeom g, int rounds, double min_margin,
    PatchRec *__restrict__ map, uint8_t *__restrict__ fills, long long first_task, long long n_tasks) {
  __shared__ uint64_t s_lo[kStemRows], s_un[kStemRows];
  __shared__ uint64_t cur_lo[256], cur_un[256], best_lo[256], best_un[256];
  __shared__ PatchWindow win;
  __shared__ double s_wt[kStemCh][kFieldCells][kFieldCells];         // the push of every touched cell in mode 1
  __shared__ uint16_t s_mov[256], s_neg[256];                        // per touched row: the movable bits, those with g < 0 (bit = cell column of the span)
  __shared__ uint8_t s_fill[kFill], s_cand[kCand][kFill];
  __shared__ int s_dup[kCand];
  __shared__ double part[4][2 * kClasses];
  __shared__ double s_max[2][4];
  __shared__ double m_s;
  __shared__ int j_s, unk_s, unk_pub_s, mov_s;
  const long long task = first_task + blockIdx.x;
  if (task >= n_tasks) return;                                       // (whole workgroups)
  const PatchPos p = patch_pos(task, g);
  const FieldSpan fr = p.fr, fq = p.fq;
  const int img = p.img, tid = threadIdx.x, nbytes = 3 * g.h * g.w;
  const bool mine = p.touched() && tid < 64 * fr.count;
  const int ch = tid & 63, cy = tid >> 6, r = ch * kPool + fr.first + cy;   // (of the threads that own a row)
  const int c = classes[img];
  const bool valid = c >= 0 && c < kClasses;
  const int by = p.y0 + tid / (3 * g.w), bx = p.x0 + (tid / 3) % g.w;       // (of the threads that own a byte of the patch)
  int b0 = 0;                                                        // the clean byte of this thread's byte of the patch
  if (tid < nbytes) b0 = x[(size_t)img * kImg + (by * 32 + bx) * 3 + tid % 3];
  if (tid < kFill) s_fill[tid] = (uint8_t)b0;
  load_stem_planes(s_lo, s_un, slo, shi, img, tid);
  if (tid < 2 * kClasses * 4) (&part[0][0])[tid] = 0.0;
  if (tid == 0) unk_s = mov_s = 0;

  // the margin of what the planes hold, from the waves' partial sums: thread 0, between two barriers
  auto margin = [&]() {
    if (tid == 0) {
      patch_margin(part, sums, sums_un, c0, img, c, m_s, j_s);
      unk_pub_s = unk_s;
      unk_s = 0;
    }
  };
  auto span_bits = [&](uint64_t word) { return __popcll((word >> fq.first) & ((1ull << fq.count) - 1ull)); };

  // ---- the movable bits: the bits that the box of this position leaves unknown; the clean margin ------------------------------------
  load_patch_window(win, x, nm, p, g, nullptr, tid);
  __syncthreads();
  if (mine) {
    uint32_t mov = 0;
    stem_row_pass(win, ch, cy, fq.count, w, bias, bn, slack, [&](int cx, bool lo_bit, bool hi_bit) { mov |= (uint32_t)(lo_bit != hi_bit) << cx; });
    s_mov[tid] = (uint16_t)mov;
    cur_lo[tid] = s_lo[r];
    cur_un[tid] = s_un[r];
    const int k0 = span_bits(s_un[r]);                               // round 0: the clean cells of the span within the slack
    if (k0) atomicAdd(&unk_s, k0);                                   // (integers: any order gives the same sum)
    if (mov) atomicOr(&mov_s, 1);
  }
  __syncthreads();
  margin();
  __syncthreads();
  double m_cur = m_s;
  int j_cur = j_s, kept_round = 0, kept_unk = unk_pub_s;
  const bool search = valid && p.touched() && mov_s != 0 && !(m_cur < -min_margin);   // (uniform over the workgroup)

  // the predicted margin of a fill: the touched cells again at radius 0, the features they reach against the clean feature
  // planes, the sums in certify_patch_kernel's order.  Leaves the fill's rows in the working planes.
  auto evaluate = [&](const uint8_t *fill, double &m_out, int &j_out, int &unk_out) {
    load_patch_window(win, x, nm, p, g, fill, tid);
    __syncthreads();
    if (mine) {
      rewrite_stem_row(s_lo, s_un, r, win, ch, cy, fq, w, bias, bn, slack);
      const int unk = span_bits(s_un[r]);
      if (unk) atomicAdd(&unk_s, unk);
    }
    __syncthreads();
    reached_sums(s_lo, s_un, p, c, true, ylo, yhi, t1, t2, t3w, A, part, tid);
    __syncthreads();
    margin();
    __syncthreads();
    m_out = m_s;
    j_out = j_s;
    unk_out = unk_pub_s;
  };

  for (int rnd = 1; search && rnd <= rounds; ++rnd) {
    // (here the working planes hold the current fill's rows)
    const uint8_t up = (uint8_t)min(255, b0 + g.amp), dn = (uint8_t)max(0, b0 - g.amp);
    if (g.h == 1 && g.w == 1 && rnd == 1) {                          // a 1 x 1 patch has three bytes: its eight corners
      if (tid < 3)
#pragma unroll
        for (int k = 0; k < kCand; ++k) s_cand[k][tid] = ((k >> tid) & 1) ? up : dn;
    } else {
      // ---- flip gains and pushes of the movable bits, on the current planes (known bits); the old feature bit is the table's
      if (mine) {
        const int py = fr.first + cy;
        const uint64_t T1 = table_word(t1, ch), T2 = table_word(t2, ch);
        auto row = [&](int c2, int y) { return (uint32_t)(s_lo[c2 * kPool + y] & 0x3FFull); };
        auto old = [&](int kind, int fc, int, int, uint32_t at) {
          return (int)(((kind == 0 ? T1 : kind == 1 ? T2 : t3w[(fc - 128) * 4 + (at >> 6)]) >> (at & 63u)) & 1ull);
        };
        const double sgn = bn[ch] >= 0.0 ? 1.0 : -1.0;
        const uint32_t mov = s_mov[tid];
        uint32_t neg = 0;
        for (int cx = 0; cx < fq.count; ++cx) {
          const int px = fq.first + cx;
          double wt = 0.0;
          if ((mov >> cx) & 1u) {
            const double gain = flip_gain(ch, py, px, row, old, T1, T2, t3w, A, c, j_cur);
            wt = stem_push(gain, (int)((s_lo[r] >> px) & 1ull), sgn);
            neg |= (uint32_t)(gain < 0.0) << cx;
          }
          s_wt[ch][cy][cx] = wt;
        }
        s_neg[tid] = (uint16_t)neg;
      }
      __syncthreads();
      // ---- scores of the bytes of the patch (every other byte scores 0): ch ascending, then py, then px; the kernel's own loop
      double sc[2] = {0.0, 0.0}, M[2];
      if (tid < nbytes) {
        const int k = tid % 3;
        int cyc[2], oyc[2], cxc[2], oxc[2];
        cells_of(by, cyc, oyc);
        cells_of(bx, cxc, oxc);
        for (int c2 = 0; c2 < kStemCh; ++c2)
#pragma unroll
          for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              if (oyc[a] < 0 || oxc[b] < 0) continue;
              const int ly = cyc[a] - fr.first, lx = cxc[b] - fq.first;   // (a cell whose field holds a byte of the patch is in the span)
              const double w1 = s_wt[c2][ly][lx];
              if (w1 == 0.0) continue;                               // (a zero term changes no sum: the sums are never -0)
              const double w0 = ((s_neg[(ly << 6) | c2] >> lx) & 1u) ? w1 : 0.0;
              const double wk = wsum[(size_t)c2 * 75 + k * 25 + oyc[a] * 5 + oxc[b]];
              sc[0] += w0 * wk;
              sc[1] += w1 * wk;
            }
      }
      double mx[2] = {fabs(sc[0]), fabs(sc[1])};
#pragma unroll
      for (int m = 0; m < 2; ++m) {                                  // M = max |score| over the patch, per mode
        for (int d = 32; d >= 1; d >>= 1) mx[m] = fmax(mx[m], __shfl_xor(mx[m], d));
        if ((tid & 63) == 0) s_max[m][tid >> 6] = mx[m];
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < 2; ++m) M[m] = fmax(fmax(s_max[m][0], s_max[m][1]), fmax(s_max[m][2], s_max[m][3]));
      if (tid < nbytes) {
        const uint8_t keep = s_fill[tid];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
          for (int t = 0; t < 3; ++t) s_cand[4 * m + t][tid] = candidate_byte(sc[m], M[m], t, up, dn, keep);
          // the slot of tau = 1/2: the sign corner of mode 1 with a hashed half of its bytes at the opposite end
          const uint8_t base = sc[1] > 0.0 ? up : (sc[1] < 0.0 ? dn : keep), other = sc[1] > 0.0 ? dn : (sc[1] < 0.0 ? up : keep);
          s_cand[4 * m + 3][tid] = hash_corner((uint32_t)p.pos, rnd, kHashStream + 4 * m + 3, (uint32_t)tid) ? other : base;
        }
      }
    }
    __syncthreads();
    if (tid < kCand) {                                               // a candidate byte-equal to an earlier one cannot win: skip it
      int dup = -1;
      for (int k = 0; k < tid && dup < 0; ++k) {
        bool same = true;
        for (int i = 0; i < nbytes && same; ++i) same = s_cand[k][i] == s_cand[tid][i];
        if (same) dup = k;
      }
      s_dup[tid] = dup;
    }
    __syncthreads();
    double best_m = INFINITY;
    int best_k = -1, best_j = -1, best_unk = 0;
    for (int k = 0; k < kCand; ++k) {
      if (s_dup[k] >= 0) continue;                                   // (uniform)
      double m;
      int j, unk;
      evaluate(s_cand[k], m, j, unk);
      if (m < best_m) {                                              // the smallest prediction; ties: the lowest index
        best_m = m;
        best_k = k;
        best_j = j;
        best_unk = unk;
        if (mine) {
          best_lo[tid] = s_lo[r];
          best_un[tid] = s_un[r];
        }
      }
    }
    if (best_k >= 0 && best_m < m_cur) {                             // strictly below the current state: it becomes the state
      m_cur = best_m;
      j_cur = best_j;
      kept_round = rnd;
      kept_unk = best_unk;
      if (mine) {
        cur_lo[tid] = best_lo[tid];
        cur_un[tid] = best_un[tid];
      }
      if (tid < nbytes) s_fill[tid] = s_cand[best_k][tid];
    }
    if (mine) {                                                      // the working planes hold the current fill's rows again
      s_lo[r] = cur_lo[tid];
      s_un[r] = cur_un[tid];
    }
    __syncthreads();
    if (m_cur < -min_margin) break;
  }
  if (tid < kFill) fills[(size_t)task * kFill + tid] = tid < nbytes ? s_fill[tid] : (uint8_t)0;
  if (tid != 0) return;
  PatchRec out;
  out.m_pred = m_cur;
  out.worst = j_cur;
  out.round = (uint16_t)kept_round;
  out.unknown = (uint16_t)(valid ? kept_unk : 0);
  map[task] = out;
}

// out[k] = image tasks[k] / P with the fill of task tasks[k] pasted at position tasks[k] % P; zeros for a task out of range
__global__ __launch_bounds__(256) void patch_paste_kernel(const uint8_t *__restrict__ x, long long n, PatchGeom g, const uint8_t *__restrict__ fills,
                                                          const int64_t *__restrict__ tasks, uint8_t *__restrict__ out, long long m) {
  const long long k = blockIdx.x;
  if (k >= m) return;
  const long long t = tasks[k], P = (long long)g.py * g.px;
  uint8_t *dst = out + (size_t)k * kImg;
  if (t < 0 || t >= n * P) {
    for (int i = threadIdx.x; i < kImg; i += 256) dst[i] = 0;
    return;
  }
  const int pos = (int)(t % P), y0 = (pos / g.px) * g.stride, x0 = (pos % g.px) * g.stride;
  const uint8_t *src = x + (size_t)(t / P) * kImg, *fill = fills + (size_t)t * kFill;
  for (int i = threadIdx.x; i < kImg; i += 256) {
    const int k3 = i % 3, iq = (i / 3) % 32, ir = i / 96;
    const bool in = ir >= y0 && ir < y0 + g.h && iq >= x0 && iq < x0 + g.w;
    dst[i] = in ? fill[((ir - y0) * g.w + (iq - x0)) * 3 + k3] : src[i];
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

int launch_attack_patch(const AttackPatchArgs &p, hipStream_t s) {
  const CertifyArgs &a = p.sweep.clean;
  const PatchGeom g{p.sweep.patch_h, p.sweep.patch_w, p.sweep.stride, p.sweep.amp, p.sweep.py, p.sweep.px};
  const long long tasks = (long long)a.n * g.py * g.px;
  for (long long l = 0; l < part::patch_launches(tasks); ++l)
    hipLaunchKernelGGL(attack_patch_kernel, dim3((unsigned)part::patch_launch_size(tasks, l)), dim3(256), 0, s, a.x, a.norm, a.w, a.bias, a.stem_bn,
                       a.slack, a.stem_lo, a.stem_hi, a.feat_lo, a.feat_hi, a.t1, a.t2, a.t3w, a.A, a.c0, p.wsum, a.classes, a.sums, a.sums_un, g,
                       p.rounds, p.min_margin, (PatchRec *)p.map, p.fills, l * part::kPatchGrid, tasks);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_patch_paste(const uint8_t *x, long long n, int patch_h, int patch_w, int stride, const uint8_t *fills, const int64_t *tasks,
                       long long m, uint8_t *out, hipStream_t s) {
  const PatchGeom g{patch_h, patch_w, stride, 0, part::patch_positions(patch_h, stride), part::patch_positions(patch_w, stride)};
  hipLaunchKernelGGL(patch_paste_kernel, dim3((unsigned)m), dim3(256), 0, s, x, n, g, fills, tasks, out, m);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

}  // namespace ttnet
