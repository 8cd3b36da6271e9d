// CIFAR "vAlexnet" variant: TT_FHE_XSMALL_vAlexnet (models/TT_FHE_XSMALL_vAlexnet.py:434-676).
//
//   features[0:5]  Conv2d(3,64,3,pad 1)+bias -> ReLU -> BatchNorm2d -> MaxPool2d(3) -> (x >= 0)
//   features[5]    one stride-1 block: Block_conv1 (3x2 window, pad 1), Block_conv2 (2x3),
//                  Block_conv3 (1x1, 8 channels per group), out4 = x; branch zero padding of the
//                  W = 10 rule (:544-550) to 11x11; plain concat (no interleave, no convf)
//   features[6:8]  Flatten -> lin1 (30976 -> 100) -> BatchNorm1d -> lin2 (100 -> 10)
//
// 32x32 inputs and 64- / 256-entry truth tables: a small network; the kernels keep every
// activation on row-packed planes and favour clarity.  The head reuses head.hip (the 0/1
// features are exact in the split-operand format).

#include <math.h>

#include "partition.h"
#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

using namespace va;

namespace {

// The nine convolution outputs (without the constant) of pooled pixel (py, px): its 5x5x3 patch of the padded image is read
// once, the taps are accumulated in (c, kh, kw) order with fmaf.  Both float stems run this loop.
__device__ __forceinline__ void va_stem_patch(const float (&img_s)[3][34][34], const float (&wr)[27], int py, int px,
                                              float (&acc)[3][3]) {
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) acc[dy][dx] = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float patch[5][5];
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
      for (int q = 0; q < 5; ++q) patch[r][q] = img_s[c][3 * py + r][3 * px + q];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx)
            acc[dy][dx] = fmaf(patch[dy + kh][dx + kw], wr[(c * 3 + kh) * 3 + kw], acc[dy][dx]);
  }
}

// stem: one workgroup per image, thread = (channel, pooled row); the zero-padded image lives in LDS
// (all 64 channel lanes of a wave read the same address: a broadcast), the 27 weights of the
// channel in registers.  Per pooled pixel the 5x5x3 input patch is read once for its nine
// convolution outputs.  Taps are accumulated in (c, kh, kw) order; a tap in the zero border adds
// w * 0, which leaves the sum unchanged.
__global__ __launch_bounds__(640) void va_stem_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                      const float *__restrict__ bias, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, uint64_t *__restrict__ rp, int n) {
  __shared__ float img_s[3][34][34];
  const int img = blockIdx.x;
  for (int i = threadIdx.x; i < 3 * 34 * 34; i += blockDim.x) {
    const int c = i / (34 * 34), r = (i / 34) % 34, q = i % 34;
    const bool in = r >= 1 && r <= 32 && q >= 1 && q <= 32;
    img_s[c][r][q] = in ? x[((size_t)img * 3 + c) * 1024 + (r - 1) * 32 + (q - 1)] : 0.f;
  }
  __syncthreads();
  const int ch = threadIdx.x & 63, py = threadIdx.x >> 6;            // 10 waves: one pooled row each
  float wr[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) wr[i] = w[ch * 27 + i];
  const float b = bias[ch], sc = scale[ch], sh = shift[ch];
  uint64_t out = 0;
  for (int px = 0; px < 10; ++px) {
    float acc[3][3];
    va_stem_patch(img_s, wr, py, px, acc);
    float best = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) best = fmaxf(best, fmaf(fmaxf(acc[dy][dx] + b, 0.f), sc, sh));   // ReLU, eval BatchNorm, MaxPool2d(3)
    out |= (uint64_t)(best >= 0.f) << px;
  }
  if (img < n) rp[((size_t)img * kStemCh + ch) * kPool + py] = out;
}

// stem from the dataset's bytes: uint8 [n][32][32][3] (HWC) in, the same bits out.  ToTensor + Normalize are folded in
// (va_stem_u8_fold): a byte b of channel c is x = (b - m_c) * a_c + e_c with the integer centre m_c = round(255 mean_c),
// a_c = 1 / (255 std_c) and the remainder e_c = (m_c - 255 mean_c) * a_c.  The centred byte b - m_c is exact in float32
// and is what LDS holds (zero in the padding), a_c is folded into the weights, and e_c -- which only the taps inside the
// image carry, since the padding is zero in NORMALISED space -- goes with the bias into one constant per border class
// of the convolution output (interior, top row, left column, corner; the pooled outputs never touch the bottom or right
// padding).  Taps are accumulated in (c, kh, kw) order as in va_stem_kernel.
// One workgroup = 32 channels of one image: lane = (channel, half of the pooled row), wave = pooled row, so a CU holds
// two workgroups (20 waves) where the float kernel has 10; the two halves of a row word meet through one shuffle.
constexpr int kVaU8TabW = 0, kVaU8TabK = 64 * 27, kVaU8TabCentre = kVaU8TabK + 64 * 4, kVaU8TabElems = kVaU8TabCentre + 4;

__global__ __launch_bounds__(640) void va_stem_u8_kernel(const uint8_t *__restrict__ x, const float *__restrict__ tab,
                                                         const float *__restrict__ scale, const float *__restrict__ shift,
                                                         uint64_t *__restrict__ rp, int n) {
  __shared__ float img_s[3][34][34];
  const int img = blockIdx.x >> 1, ch = ((blockIdx.x & 1) << 5) | (threadIdx.x & 31);
  if (img >= n) return;                                              // (whole workgroups: no barrier is left behind)
  const float centre[3] = {tab[kVaU8TabCentre], tab[kVaU8TabCentre + 1], tab[kVaU8TabCentre + 2]};
  float wr[27];                                                      // (in flight while the image is staged)
#pragma unroll
  for (int i = 0; i < 27; ++i) wr[i] = tab[kVaU8TabW + i * 64 + ch];
  const float4 kc = *(const float4 *)(tab + kVaU8TabK + ch * 4);     // interior, top, left, corner
  const float sc = scale[ch], sh = shift[ch];
  for (int i = threadIdx.x; i < 3 * 34 * 34; i += blockDim.x) {      // the zero border
    const int r = (i / 34) % 34, q = i % 34;
    if (r == 0 || r == 33 || q == 0 || q == 33) (&img_s[0][0][0])[i] = 0.f;
  }
  const uint32_t *src = (const uint32_t *)(x + (size_t)img * 3072);   // (4-byte aligned: checked by the plan)
  for (int i = threadIdx.x; i < 768; i += blockDim.x) {
    const uint32_t v = src[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * i + k, p = e / 3, c = e - 3 * p;
      img_s[c][(p >> 5) + 1][(p & 31) + 1] = (float)((v >> (8 * k)) & 0xFFu) - centre[c];
    }
  }
  __syncthreads();
  const int half = (threadIdx.x >> 5) & 1, py = threadIdx.x >> 6;    // 10 waves: one pooled row each
  uint32_t out = 0;
  for (int j = 0; j < 5; ++j) {
    const int px = 5 * half + j;
    float acc[3][3];
    va_stem_patch(img_s, wr, py, px, acc);
    float best = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const bool top = dy == 0 && py == 0, left = dx == 0 && px == 0;
        const float b = top ? (left ? kc.w : kc.y) : (left ? kc.z : kc.x);
        best = fmaxf(best, fmaf(fmaxf(acc[dy][dx] + b, 0.f), sc, sh));   // ReLU, eval BatchNorm, MaxPool2d(3)
      }
    out |= (uint32_t)(best >= 0.f) << px;
  }
  out |= (uint32_t)__shfl_xor((int)out, 32);                         // columns 0..4 and 5..9 of the row word
  if (half == 0) rp[((size_t)img * kStemCh + ch) * kPool + py] = out;
}

// Block_conv1 / Block_conv2 / out4: thread = (image, channel, output row of the 11x11 plane).
// Tables: 64 entries, 1 bit, striped dword layout of lut_build.hip ([c/16][2][16]).
__global__ void va_dw_kernel(const uint64_t *__restrict__ x_rp, const uint32_t *__restrict__ t1,
                             const uint32_t *__restrict__ t2, uint64_t *__restrict__ y, int n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * part::kVaDwTasks) return;
  const int oy = t % kSide, c = (t / kSide) % kStemCh, img = t / part::kVaDwTasks;
  const uint64_t *pl = x_rp + ((size_t)img * kStemCh + c) * kPool;
  auto row = [&](int iy) { return shifted_row(iy, [&](int r) { return pl[r]; }); };
  const uint64_t T1 = table_word(t1, c), T2 = table_word(t2, c);
  uint64_t r1 = 0, r2 = 0;
  if (oy < kPool) {   // conv1: 3x2 window, rows oy-1..oy+1, 11 output columns; bottom row 10 is zero padding
    const uint64_t a = row(oy - 1), b = row(oy), d = row(oy + 1);
    for (int ox = 0; ox < kSide; ++ox) r1 |= ((T1 >> conv1_index(a, b, d, ox)) & 1ull) << ox;
  }
  {                   // conv2: 2x3 window, rows oy-1..oy, 10 output columns; right column 10 is zero padding
    const uint64_t a = row(oy - 1), b = row(oy);
    for (int ox = 0; ox < kPool; ++ox) r2 |= ((T2 >> conv2_index(a, b, ox)) & 1ull) << ox;
  }
  y[((size_t)img * kFeatCh + c) * kSide + oy] = r1;
  y[((size_t)img * kFeatCh + 64 + c) * kSide + oy] = r2;
  y[((size_t)img * kFeatCh + 192 + c) * kSide + oy] = oy < kPool ? pl[oy] : 0ull;   // out4 = x, padded right / bottom
}

// Block_conv3: thread = (image, group of 8 channels, row); table uint8 [8][256]
__global__ void va_c3_kernel(const uint64_t *__restrict__ x_rp, const uint8_t *__restrict__ t3, uint64_t *__restrict__ y,
                             int n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * part::kVaC3Tasks) return;
  const int oy = t % kSide, g = (t / kSide) % part::kVaC3Groups, img = t / part::kVaC3Tasks;
  uint64_t rows[8], out[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    rows[k] = oy < kPool ? x_rp[((size_t)img * kStemCh + 8 * g + k) * kPool + oy] : 0ull;
    out[k] = 0;
  }
  if (oy < kPool)
    for (int xx = 0; xx < kPool; ++xx) {
      const uint32_t v = t3[g * 256 + conv3_index(rows, xx)];
#pragma unroll
      for (int k = 0; k < 8; ++k) out[k] |= (uint64_t)((v >> k) & 1u) << xx;
    }
#pragma unroll
  for (int k = 0; k < 8; ++k) y[((size_t)img * kFeatCh + 128 + 8 * g + k) * kSide + oy] = out[k];
}

// Flatten (C-major over [256][11][11]) into lin1's fragment-ordered operand.  The features are
// bits: 0.0 / 1.0 is exact in the split format with a zero low term, so only plane 0 is written
// (plane 1 stays zero from allocation).  Thread = (image, k-step): its 16 features are two aligned
// 16-byte runs of plane 0 (lane halves k < 8 and k >= 8 of the fragment).
__global__ void va_feat_kernel(const uint64_t *__restrict__ y, uint16_t *__restrict__ feat_frag, int n) {
  constexpr int KS = part::kVaFeatTasks;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * KS) return;
  const int ks = t % KS, img = t / KS;
  constexpr uint32_t ONE = 0x4C00u;                    // fp16(1.0 * ACT_PRESCALE)
  static_assert(ACT_PRESCALE == 16.0f, "ONE encodes the activation prescale");
  uint32_t half[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) {
    const int f = 16 * ks + kk, ch = f / kPlane, rem = f - kPlane * ch, oy = rem / kSide, ox = rem - kSide * oy;
    const uint32_t bit = (uint32_t)(y[((size_t)img * kFeatCh + ch) * kSide + oy] >> ox) & 1u;
    half[kk >> 3][(kk & 7) >> 1] |= (bit ? ONE : 0u) << (16 * (kk & 1));
  }
  uint4 *dst = (uint4 *)feat_frag + ((((size_t)(img >> 5) * KS + ks) * SPLIT_PLANES + 0) * 64 + (img & 31));
  dst[0] = make_uint4(half[0][0], half[0][1], half[0][2], half[0][3]);
  dst[32] = make_uint4(half[1][0], half[1][1], half[1][2], half[1][3]);
}

__global__ void va_frag_to_flat_kernel(const uint16_t *__restrict__ af, float *__restrict__ out, int n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int K = kFeat, KS = K / 16;
  if (t >= (size_t)n * K) return;
  const int f = t % K, img = t / K;
  out[t] = load_feature(af, img, KS, f >> 4, f & 15);
}

}  // namespace

int launch_va_stem(const float *x, const float *w, const float *bias, const float *scale, const float *shift,
                   uint64_t *rp, int n, hipStream_t s) {
  hipLaunchKernelGGL(va_stem_kernel, dim3(n), dim3(640), 0, s, x, w, bias, scale, shift, rp, n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int va_stem_kernel_arg_sizes(const int **sizes) {
  using S = KernelArgSizes<decltype(&va_stem_kernel)>;
  *sizes = S::sizes;
  return S::n;
}

size_t va_stem_u8_table_elems() { return kVaU8TabElems; }

// The table of va_stem_u8_kernel, in float64 from the stem's weights [64][3][3][3], its bias and the normalisation
// constants: weights times a_c as [27 taps][64 channels], the four border-class constants per channel, the integer centres.  (A centre is kept
// inside [0, 255]: b - m_c stays exact whatever mean is given, the remainder e_c takes the rest.)
void va_stem_u8_fold(const float *w, const float *bias, const float *mean3, const float *std3, float *tab) {
  double a[3], e[3];
  for (int c = 0; c < 3; ++c) {
    const double m255 = 255.0 * (double)mean3[c];
    const double centre = std::min(255.0, std::max(0.0, nearbyint(m255)));
    a[c] = 1.0 / (255.0 * (double)std3[c]);
    e[c] = (centre - m255) * a[c];
    tab[kVaU8TabCentre + c] = (float)centre;
  }
  tab[kVaU8TabCentre + 3] = 0.f;
  for (int ch = 0; ch < 64; ++ch) {
    double k[4] = {(double)bias[ch], (double)bias[ch], (double)bias[ch], (double)bias[ch]};
    for (int c = 0; c < 3; ++c)
      for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) {
          const int i = (c * 3 + kh) * 3 + kw;
          const double wv = (double)w[ch * 27 + i];
          tab[kVaU8TabW + i * 64 + ch] = (float)(wv * a[c]);       // [tap][channel]: a wave's loads are contiguous
          // class bit 0: the output is in convolution row 0 (tap row kh = 0 is padding); bit 1: column 0 (kw = 0 is)
          for (int cls = 0; cls < 4; ++cls)
            if (!((cls & 1) && kh == 0) && !((cls & 2) && kw == 0)) k[cls] += wv * e[c];
        }
    for (int cls = 0; cls < 4; ++cls) tab[kVaU8TabK + ch * 4 + cls] = (float)k[cls];
  }
}

int launch_va_stem_u8(const uint8_t *x, const float *tab, const float *scale, const float *shift, uint64_t *rp, int n,
                      hipStream_t s) {
  hipLaunchKernelGGL(va_stem_u8_kernel, dim3(2 * (unsigned)n), dim3(640), 0, s, x, tab, scale, shift, rp, n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int va_stem_u8_kernel_arg_sizes(const int **sizes) {
  using S = KernelArgSizes<decltype(&va_stem_u8_kernel)>;
  *sizes = S::sizes;
  return S::n;
}

int launch_va_block(const uint64_t *x_rp,const void *t1, const void *t2, const void *t3, uint64_t *y, int n, hipStream_t s) {
  constexpr part::FlatGrid dw = part::va_dw_grid(), c3 = part::va_c3_grid();
  hipLaunchKernelGGL(va_dw_kernel, dim3(dw.workgroups(n)), dim3(dw.threads), 0, s, x_rp, (const uint32_t *)t1,
                     (const uint32_t *)t2, y, n);
  hipLaunchKernelGGL(va_c3_kernel, dim3(c3.workgroups(n)), dim3(c3.threads), 0, s, x_rp, (const uint8_t *)t3, y, n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_va_feat(const uint64_t *y, void *feat_frag, int n, hipStream_t s) {
  constexpr part::FlatGrid g = part::va_feat_grid();
  hipLaunchKernelGGL(va_feat_kernel, dim3(g.workgroups(n)), dim3(g.threads), 0, s, y, (uint16_t *)feat_frag, n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_va_frag_to_flat(const void *af, float *out, int n, hipStream_t s) {
  const size_t t = (size_t)n * kFeat;
  hipLaunchKernelGGL(va_frag_to_flat_kernel, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, (const uint16_t *)af, out, n);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

}  // namespace ttnet
