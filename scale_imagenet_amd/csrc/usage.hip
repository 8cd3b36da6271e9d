// Truth-table usage counts (ttnet_table_usage_add): which entry of which table every lookup of a forward read; and
// care-set misses (ttnet_care_misses): per image, how many of those lookups fall outside a chosen set of entries.
//
// Counting is its own launches over what a lane still holds after a forward; the forward kernels are not involved.
// plan.hip brings every block's input and its four branch tensors to one layout -- row-packed uint64 planes
// [n][C][H], pixel x = bit x -- and the two kernels here form, per output position, the CANONICAL table index
// (pattern read MSB first over (c_in_group, kh, kw), zero padding = bit 0: the order of ttnet_plan_get_table) and
// add 1 to int64 counter[group][index].
//
// The histogram is skewed on real images: a flat region sends every lookup of a depthwise group to index 0 or
// 2^n - 1, and a grouped 1x1 block with few groups sends thousands of lookups per image into a handful of tables.
// Two schemes, chosen per launch:
//   kUsagePlain   one 64-bit atomic add per lookup (the correctness baseline).
//   kUsageMerged  equal counters are merged within a wave first: up to kMergeRounds times the wave takes the
//                 counter of its first unserved lane, ballots the lanes that hold the same one, and that lane adds
//                 their number with ONE atomic; whoever is left after the rounds adds 1 on its own.  A wave is 64
//                 consecutive x of (mostly) one row of one group, so a flat row costs one or two atomics instead of
//                 64 to the same address; on scattered indices the rounds serve one lane each and cost their ballots.
// Integer adds only: the counts do not depend on the scheme, the launch geometry, the lane or the stream.
//
// Care-set misses (ttnet_care_misses) run over the same lookups -- the index is formed by the same two device functions --
// and test one bit of a per-block bitmap instead of adding to a counter; their reduction is per image (further down).

#include "ttnet_common.h"

namespace ttnet {

namespace {

constexpr int kMergeRounds = 4;
constexpr int kUsageThreads = 256;

// counter[off] += 1 for every lane with `valid`; called by whole waves (the loop around it is wave-uniform)
template <bool MERGED>
__device__ inline void usage_add(unsigned long long *cnt, uint32_t off, bool valid) {
  if constexpr (MERGED) {
    const uint32_t lane = __lane_id();
    uint64_t todo = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < kMergeRounds && todo; ++r) {
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)off, leader);
      const bool mine = valid && off == key;
      const uint64_t same = __ballot(mine);
      if (lane == (uint32_t)leader) atomicAdd(cnt + key, (unsigned long long)__popcll(same));
      if (mine) valid = false;
      todo &= ~same;
    }
  }
  if (valid) atomicAdd(cnt + off, 1ull);
}

// The canonical index of one lookup, formed in one place for the counting kernels and the care-set kernels below.
// Depthwise: `rows` = the H uint64 rows of the lookup's plane, (ox, oy) its output position.
__device__ inline uint32_t dw_index(const uint64_t *__restrict__ rows, int ox, int oy, int H, int kh, int kw, int stride, int pad) {
  const int nbits = kh * kw;
  const uint64_t wmask = ((uint64_t)1 << kw) - 1;
  uint32_t idx = 0;
  for (int i = 0; i < kh; ++i) {
    const int iy = oy * stride - pad + i;
    uint64_t w = 0;
    if (iy >= 0 && iy < H) w = ((rows[iy] << pad) >> (ox * stride)) & wmask;   // bit j = window column j (LSB-first rows)
    // window column j is index bit nbits - 1 - (i * kw + j): the kw bits go in reversed
    w = __brevll(w) >> (64 - kw);
    idx |= (uint32_t)w << (nbits - (i + 1) * kw);
  }
  return idx;
}

// Depthwise block (one channel per group, kh x kw window, stride, symmetric zero padding): counter [C][2^(kh*kw)]
template <bool MERGED>
__global__ void __launch_bounds__(kUsageThreads)
usage_dw_kernel(const uint64_t *__restrict__ x, unsigned long long *__restrict__ cnt, size_t total, int C, int H, int Ho, int Wo,
                int kh, int kw, int stride, int pad) {
  const int nbits = kh * kw;
  for (size_t base = (size_t)blockIdx.x * kUsageThreads; base < total; base += (size_t)gridDim.x * kUsageThreads) {
    const size_t t = base + threadIdx.x;
    const bool valid = t < total;
    uint32_t off = 0;
    if (valid) {
      const int ox = (int)(t % Wo), oy = (int)((t / Wo) % Ho);
      const size_t plane = t / ((size_t)Wo * Ho);           // img * C + c
      const int c = (int)(plane % C);
      off = ((uint32_t)c << nbits) | dw_index(x + plane * H, ox, oy, H, kh, kw, stride, pad);
    }
    usage_add<MERGED>(cnt, off, valid);
  }
}

// Grouped 1x1 block over the H x W positions of `nsrc` row tensors of Csrc planes each: channel k of the block's
// input is plane k / nsrc of src[k % nsrc] (nsrc = 1: a plain tensor; 4: the interleaved branch concat, channel
// 4c + branch), group g takes channels [g * cg, (g + 1) * cg), channel j of the group is index bit cg - 1 - j.
// Counter [G][2^cg].
struct UsagePwSrc {
  const uint64_t *p[4];
};
// Grouped 1x1: the index of group g of image img at (xx, y)
__device__ inline uint32_t pw_index(const UsagePwSrc &src, int nsrc, size_t img, int Csrc, int g, int cg, int H, int y, int xx) {
  uint32_t idx = 0;
  for (int j = 0; j < cg; ++j) {
    const int k = g * cg + j;
    const uint64_t *sp = nsrc == 1 ? src.p[0] : src.p[k & 3];
    const int plane = nsrc == 1 ? k : k >> 2;
    const uint64_t w = sp[(img * Csrc + plane) * H + y];
    idx |= (uint32_t)((w >> xx) & 1u) << (cg - 1 - j);
  }
  return idx;
}

template <bool MERGED>
__global__ void __launch_bounds__(kUsageThreads)
usage_pw_kernel(UsagePwSrc src, int nsrc, unsigned long long *__restrict__ cnt, size_t total, int Csrc, int G, int cg, int H, int W) {
  for (size_t base = (size_t)blockIdx.x * kUsageThreads; base < total; base += (size_t)gridDim.x * kUsageThreads) {
    const size_t t = base + threadIdx.x;
    const bool valid = t < total;
    uint32_t off = 0;
    if (valid) {
      const int xx = (int)(t % W), y = (int)((t / W) % H);
      const size_t gi = t / ((size_t)W * H);               // img * G + g
      const int g = (int)(gi % G);
      off = ((uint32_t)g << cg) | pw_index(src, nsrc, gi / G, Csrc, g, cg, H, y, xx);
    }
    usage_add<MERGED>(cnt, off, valid);
  }
}

// ---- care-set misses (ttnet_care_misses) ----
// The same lookups, tested against a bitmap instead of counted: care[group][max(1, 2^n / 32)] uint32, bit i % 32 of word
// i / 32 = entry i of the group.  One grid row (blockIdx.y) per image, so no partial sum ever mixes images: a wave
// ballots its misses and adds the popcount to a wave-uniform total, the waves of a workgroup meet in LDS and the
// workgroup adds once into its image's int32 slot (nothing when the total is 0).  Integer adds only.
__device__ inline bool care_miss(const uint32_t *__restrict__ care, int g, int nbits, uint32_t idx) {
  const uint32_t wpg = nbits > 5 ? 1u << (nbits - 5) : 1u;
  return !((care[(size_t)g * wpg + (idx >> 5)] >> (idx & 31u)) & 1u);
}

// misses of this thread's lookups (wave-uniform `wave_total`) -> *slot
__device__ inline void care_reduce(int wave_total, int *slot) {
  __shared__ int part[kUsageThreads / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[wave] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kUsageThreads / 64; ++w) sum += part[w];
    if (sum) atomicAdd(slot, sum);
  }
}

// per_img = C * Ho * Wo lookups of image blockIdx.y; rows[img * row_stride] is that image's slot for this block
__global__ void __launch_bounds__(kUsageThreads)
care_dw_kernel(const uint64_t *__restrict__ x, const uint32_t *__restrict__ care, int *__restrict__ rows, int row_stride, int per_img,
               int C, int H, int Ho, int Wo, int kh, int kw, int stride, int pad) {
  const size_t img = blockIdx.y;
  int total = 0;
  for (int base = blockIdx.x * kUsageThreads; base < per_img; base += gridDim.x * kUsageThreads) {
    const int t = base + threadIdx.x;
    bool miss = false;
    if (t < per_img) {
      const int ox = t % Wo, oy = (t / Wo) % Ho, c = t / (Wo * Ho);
      miss = care_miss(care, c, kh * kw, dw_index(x + (img * C + c) * H, ox, oy, H, kh, kw, stride, pad));
    }
    total += __popcll(__ballot(miss));
  }
  care_reduce(total, rows + img * row_stride);
}

__global__ void __launch_bounds__(kUsageThreads)
care_pw_kernel(UsagePwSrc src, int nsrc, const uint32_t *__restrict__ care, int *__restrict__ rows, int row_stride, int per_img,
               int Csrc, int G, int cg, int H, int W) {
  const size_t img = blockIdx.y;
  int total = 0;
  for (int base = blockIdx.x * kUsageThreads; base < per_img; base += gridDim.x * kUsageThreads) {
    const int t = base + threadIdx.x;
    bool miss = false;
    if (t < per_img) {
      const int xx = t % W, y = (t / W) % H, g = t / (W * H);
      miss = care_miss(care, g, cg, pw_index(src, nsrc, img, Csrc, g, cg, H, y, xx));
    }
    total += __popcll(__ballot(miss));
  }
  care_reduce(total, rows + img * row_stride);
}

unsigned usage_grid(size_t total) {
  const size_t blocks = (total + kUsageThreads - 1) / kUsageThreads;
  return (unsigned)std::max<size_t>(1, std::min<size_t>(blocks, 256 * 32));     // grid-stride beyond 32 workgroups per CU
}

}  // namespace

namespace {

// window bits of one row are cut out of (row << pad): everything must fit the 64-bit word and the 32-bit offset
int check_dw(int C, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int pad) {
  if (W + 2 * pad > 64 || kh * kw > 24 || kw > 8 || ((size_t)C << (kh * kw)) > 0xFFFFFFFFull || (Wo - 1) * stride + kw > W + 2 * pad ||
      (Ho - 1) * stride + kh > H + 2 * pad) {
    set_error("table usage: depthwise geometry %dx%d k%dx%d s%d p%d not served", H, W, kh, kw, stride, pad);
    return TTNET_E_UNSUPPORTED;
  }
  return TTNET_OK;
}

int check_pw(int nsrc, int Csrc, int groups, int cin_g, int W) {
  if ((nsrc != 1 && nsrc != 4) || cin_g < 1 || cin_g > 24 || W > 64 || groups * cin_g != nsrc * Csrc ||
      ((size_t)groups << cin_g) > 0xFFFFFFFFull) {
    set_error("table usage: grouped 1x1 geometry (%d sources x %d planes, %d groups of %d) not served", nsrc, Csrc, groups, cin_g);
    return TTNET_E_UNSUPPORTED;
  }
  return TTNET_OK;
}

int check_care_batch(int n) {
  if (n < 1 || n > 65535) {
    set_error("care misses: %d images, one grid row per image serves 1 .. 65535", n);
    return TTNET_E_UNSUPPORTED;
  }
  return TTNET_OK;
}

// one grid row per image; x: enough workgroups for the image's lookups, grid-stride beyond 64
dim3 care_grid(int per_img, int n) {
  return dim3((unsigned)std::max(1, std::min((per_img + kUsageThreads - 1) / kUsageThreads, 64)), (unsigned)n);
}

}  // namespace

int launch_usage_dw(const uint64_t *x_rp, int n, int C, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int pad,
                    int64_t *counters, int scheme, hipStream_t s) {
  TT_TRY(check_dw(C, H, W, Ho, Wo, kh, kw, stride, pad));
  const size_t total = (size_t)n * C * Ho * Wo;
  auto k = scheme == kUsageMerged ? usage_dw_kernel<true> : usage_dw_kernel<false>;
  hipLaunchKernelGGL(k, dim3(usage_grid(total)), dim3(kUsageThreads), 0, s, x_rp, (unsigned long long *)counters, total, C, H, Ho, Wo,
                     kh, kw, stride, pad);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_usage_pw(const uint64_t *const *src, int nsrc, int n, int Csrc, int groups, int cin_g, int H, int W, int64_t *counters,
                    int scheme, hipStream_t s) {
  TT_TRY(check_pw(nsrc, Csrc, groups, cin_g, W));
  UsagePwSrc sp{};
  for (int i = 0; i < 4; ++i) sp.p[i] = src[i < nsrc ? i : 0];
  const size_t total = (size_t)n * groups * H * W;
  auto k = scheme == kUsageMerged ? usage_pw_kernel<true> : usage_pw_kernel<false>;
  hipLaunchKernelGGL(k, dim3(usage_grid(total)), dim3(kUsageThreads), 0, s, sp, nsrc, (unsigned long long *)counters, total, Csrc, groups,
                     cin_g, H, W);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_care_dw(const uint64_t *x_rp, int n, int C, int H, int W, int Ho, int Wo, int kh, int kw, int stride, int pad,
                   const uint32_t *care, int32_t *rows, int row_stride, hipStream_t s) {
  TT_TRY(check_dw(C, H, W, Ho, Wo, kh, kw, stride, pad));
  TT_TRY(check_care_batch(n));
  const int per_img = C * Ho * Wo;
  hipLaunchKernelGGL(care_dw_kernel, care_grid(per_img, n), dim3(kUsageThreads), 0, s, x_rp, care, rows, row_stride, per_img, C, H, Ho,
                     Wo, kh, kw, stride, pad);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int launch_care_pw(const uint64_t *const *src, int nsrc, int n, int Csrc, int groups, int cin_g, int H, int W, const uint32_t *care,
                   int32_t *rows, int row_stride, hipStream_t s) {
  TT_TRY(check_pw(nsrc, Csrc, groups, cin_g, W));
  TT_TRY(check_care_batch(n));
  UsagePwSrc sp{};
  for (int i = 0; i < 4; ++i) sp.p[i] = src[i < nsrc ? i : 0];
  const int per_img = groups * H * W;
  hipLaunchKernelGGL(care_pw_kernel, care_grid(per_img, n), dim3(kUsageThreads), 0, s, sp, nsrc, care, rows, row_stride, per_img, Csrc,
                     groups, cin_g, H, W);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

}  // namespace ttnet
