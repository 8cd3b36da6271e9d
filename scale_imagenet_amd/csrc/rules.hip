// Rule support: which cubes of a cover the data uses.  For every function of a batch, a cover (the keys of
// ttnet_minimise_covers, in that call's order) is joined with the lookup counts u[p] of its table (ttnet_table_usage_add):
// per cube the lookups it holds (hits), those it is the first kept cube to hold (first) and those no other kept cube holds
// (sole); per function the covered and the lost mass; optionally the bitmap of the lost patterns.  Definitions: include/ttnet.h.
//
// One workgroup of four waves per function, a grid of at most kSupGroups workgroups striding over the functions.
//   Lanes own patterns, four each, and walk the cubes: the keys are staged in LDS in chunks of kSupChunk, read back four at a
//   time (one 16-byte broadcast read for all lanes) and tested with an AND and a compare per pattern.  Matches are rare
//   against tests: a match takes a branch in which the lane updates its pattern's state and adds u[p] to the cube's 64-bit
//   LDS accumulator.  After the walk of a chunk the accumulators go out as plain stores: a cube lies in one chunk only.
//   Per-pattern state across chunks: the index of the first kept cube that holds the pattern, the number of kept cubes that
//   hold it saturated at 2, and whether any cube of the full list holds it -- 8 bytes per pattern in the workgroup's slice of
//   the workspace, always read and written by the thread that owns the pattern.  first / sole follow from that state alone:
//   one pass over the patterns per chunk of cubes, LDS adds again, plain stores out.
//   Without keep flags nothing can be lost, so a pattern with u = 0 changes no output: the walk then runs over the compacted
//   list of the patterns with u != 0 (2 bytes per pattern in the workspace).  With keep flags every pattern is walked,
//   because lost_patterns and lost_bits count patterns whatever their u.
//   LDS: 4 KB keys, 1 KB keep flags, 16 KB accumulators, 8 KB lost bitmap: 29 KB with pruning, 20 KB without.
// Integer adds only, so the bytes do not depend on the launch geometry or on the order of the compacted list.  Every index
// into the cubes is below min(counts[f], cube_cap), every pattern below 2^n, every usage row checked against n_usage_rows.

#include "ttnet_common.h"

namespace ttnet {

namespace {

constexpr int kSupThreads = 256;
constexpr int kSupChunk = 1024;                     // cubes staged at a time
constexpr int kSupPer = 4;                          // patterns per lane and pass
constexpr int kSupGroups = 1024;                    // four per CU: the workspace is sized for them, not for n_funcs
constexpr int kSupMaxBits = 16;
constexpr int kSupMaxWords = 1 << (kSupMaxBits - 5);
constexpr int kSupHeader = 256;                     // the workspace starts with the count of bad usage rows
constexpr int kSupBytes = 10;                       // workspace per pattern and workgroup: state (8) and list (2)
constexpr uint32_t kSupNone = 0xFFFFFFFFu;
constexpr uint32_t kSupNoMatch = 1u;                // mask 0, value 1: holds no pattern (pads a chunk to a multiple of four)
constexpr uint32_t kSupFull = 4u;                   // state flag: some cube of the full list holds the pattern

size_t support_stride(int n_bits) { return (((size_t)kSupBytes << n_bits) + 255) & ~(size_t)255; }
int64_t support_groups(int64_t n_funcs) { return std::min<int64_t>(n_funcs, kSupGroups); }

// kPrune: keep flags are given.  Without them every cube is kept, nothing is lost and the patterns with u = 0 are skipped.
template <bool kPrune>
__global__ void __launch_bounds__(kSupThreads)
support_kernel(const uint32_t *__restrict__ cubes, const int32_t *__restrict__ counts, int64_t cap, const uint8_t *__restrict__ keep,
               const int64_t *__restrict__ usage, const int32_t *__restrict__ usage_row, int64_t n_rows, int n, int64_t n_funcs,
               int64_t *__restrict__ hits, int64_t *__restrict__ first, int64_t *__restrict__ sole, int64_t *__restrict__ totals,
               uint32_t *__restrict__ lost_bits, uint8_t *__restrict__ work, size_t stride) {
  __shared__ __align__(16) uint32_t s_key[kSupChunk];
  __shared__ __align__(4) uint8_t s_keep[kSupChunk];
  __shared__ unsigned long long s_acc[2][kSupChunk];   // the walk: hits; the last passes: first and sole
  __shared__ uint32_t s_lost[kSupMaxWords];
  __shared__ unsigned long long s_tot[4];
  __shared__ uint32_t s_np;
  const uint32_t tid = threadIdx.x;
  const uint32_t npat = 1u << n, lwords = npat >= 32 ? npat >> 5 : 1;
  uint2 *state = (uint2 *)(work + kSupHeader + (size_t)blockIdx.x * stride);
  uint16_t *plist = (uint16_t *)(state + npat);

  for (int64_t f = blockIdx.x; f < n_funcs; f += gridDim.x) {
    __syncthreads();                                   // the previous function's last LDS reads
    int64_t *h_out = hits + (size_t)f * cap, *f_out = first + (size_t)f * cap, *s_out = sole + (size_t)f * cap;
    const int64_t row = usage_row[f];
    if (row < 0 || row >= n_rows) {                    // counted, and every output of the function zero
      for (int64_t c = tid; c < cap; c += kSupThreads) h_out[c] = f_out[c] = s_out[c] = 0;
      if (tid < 4) totals[f * 4 + tid] = 0;
      if (lost_bits)
        for (uint32_t w = tid; w < lwords; w += kSupThreads) lost_bits[(size_t)f * lwords + w] = 0;
      if (tid == 0) atomicAdd((unsigned long long *)work, 1ull);
      continue;
    }
    const int64_t *u = usage + (size_t)row * npat;
    const uint32_t *ck = cubes + (size_t)f * cap;
    const uint8_t *kp = kPrune ? keep + (size_t)f * cap : nullptr;
    const int64_t nc = std::min<int64_t>(std::max<int64_t>(counts[f], 0), cap);      // never past the cap, whatever counts says

    if (tid < 4) s_tot[tid] = 0;
    if (tid == 0) s_np = 0;
    if (kPrune)
      for (uint32_t w = tid; w < lwords; w += kSupThreads) s_lost[w] = 0;
    __syncthreads();
    // ---- the patterns to walk, and used_patterns -----------------------------------------------------------------
    uint32_t used = 0;
    for (uint32_t p = tid; p < npat; p += kSupThreads) {
      const int64_t up = u[p];
      used += up > 0;
      if (!kPrune && up != 0) plist[atomicAdd(&s_np, 1u)] = (uint16_t)p;
    }
    if (used) atomicAdd(&s_tot[2], (unsigned long long)used);
    __syncthreads();                                   // plist, through the CU's own L1
    const uint32_t np = kPrune ? npat : s_np;

    // ---- the walk: chunk by chunk, every lane its patterns against every staged cube --------------------------------
    for (int64_t cb = 0; cb < nc; cb += kSupChunk) {
      const uint32_t cn = (uint32_t)std::min<int64_t>(kSupChunk, nc - cb), cn4 = (cn + 3) & ~3u;
      __syncthreads();                                 // the previous chunk's reads of s_key and s_acc
      for (uint32_t c = tid; c < kSupChunk; c += kSupThreads) {
        s_key[c] = c < cn ? ck[cb + c] : kSupNoMatch;
        if (kPrune) s_keep[c] = c < cn && kp[cb + c] != 0;
        s_acc[0][c] = 0;
      }
      __syncthreads();
      for (uint32_t base = 0; base < np; base += kSupThreads * kSupPer) {
        uint32_t p[kSupPer], fi[kSupPer], fl[kSupPer];
        int64_t uu[kSupPer];
#pragma unroll
        for (int j = 0; j < kSupPer; ++j) {
          const uint32_t i = base + j * kSupThreads + tid;
          p[j] = kSupNone;                             // a pattern no cube holds: the test keeps the high half of p
          uu[j] = 0;
          fi[j] = kSupNone;
          fl[j] = 0;
          if (i < np) {
            p[j] = kPrune ? i : plist[i];
            uu[j] = u[p[j]];
            if (cb) {
              const uint2 st = state[i];
              fi[j] = st.x;
              fl[j] = st.y;
            }
          }
        }
        for (uint32_t c = 0; c < cn4; c += 4) {
          const uint4 k4 = *(const uint4 *)&s_key[c];
          const uint32_t kept4 = kPrune ? *(const uint32_t *)&s_keep[c] : 0x01010101u;
          const uint32_t keys[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t mask = (keys[q] >> 16) | 0xFFFF0000u, value = keys[q] & 0xFFFFu;
            bool m[kSupPer], any = false;
#pragma unroll
            for (int j = 0; j < kSupPer; ++j) {
              m[j] = (p[j] & mask) == value;
              any |= m[j];
            }
            if (any) {
              const bool kept = (kept4 >> (8 * q)) & 1;
#pragma unroll
              for (int j = 0; j < kSupPer; ++j) {
                if (!m[j]) continue;
                if (kept) {
                  const uint32_t cnt = fl[j] & 3u;
                  if (cnt == 0) fi[j] = (uint32_t)cb + c + q;
                  fl[j] = kSupFull | (cnt < 2 ? cnt + 1 : 2u);
                  if (uu[j]) atomicAdd(&s_acc[0][c + q], (unsigned long long)uu[j]);
                } else {
                  fl[j] |= kSupFull;
                }
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < kSupPer; ++j) {
          const uint32_t i = base + j * kSupThreads + tid;
          if (i < np) state[i] = make_uint2(fi[j], fl[j]);
        }
      }
      __syncthreads();
      for (uint32_t c = tid; c < cn; c += kSupThreads) h_out[cb + c] = (int64_t)s_acc[0][c];
    }
    for (int64_t c = nc + tid; c < cap; c += kSupThreads) h_out[c] = f_out[c] = s_out[c] = 0;

    // ---- totals and the lost bitmap, from the state of every walked pattern (no cube: no state, all zero) -----------------
    unsigned long long covered = 0, lost = 0;
    uint32_t lostp = 0;
    if (nc > 0) {
      for (uint32_t i = tid; i < np; i += kSupThreads) {
        const uint2 st = state[i];
        const uint32_t pp = kPrune ? i : plist[i];
        if (st.y & 3u) {
          covered += (unsigned long long)u[pp];
        } else if (kPrune && (st.y & kSupFull)) {
          lost += (unsigned long long)u[pp];
          lostp += 1;
          atomicOr(&s_lost[pp >> 5], 1u << (pp & 31));
        }
      }
    }
    if (covered) atomicAdd(&s_tot[0], covered);
    if (lost) atomicAdd(&s_tot[1], lost);
    if (lostp) atomicAdd(&s_tot[3], (unsigned long long)lostp);

    // ---- first and sole: per chunk of cubes, every pattern adds to the first kept cube that holds it ---------------------
    for (int64_t cb = 0; cb < nc; cb += kSupChunk) {
      const uint32_t cn = (uint32_t)std::min<int64_t>(kSupChunk, nc - cb);
      __syncthreads();
      for (uint32_t c = tid; c < kSupChunk; c += kSupThreads) s_acc[0][c] = s_acc[1][c] = 0;
      __syncthreads();
      for (uint32_t i = tid; i < np; i += kSupThreads) {
        const uint2 st = state[i];
        const uint32_t cnt = st.y & 3u;
        const int64_t at = (int64_t)st.x - cb;
        if (cnt == 0 || at < 0 || at >= (int64_t)cn) continue;
        const unsigned long long up = (unsigned long long)u[kPrune ? i : plist[i]];
        if (up == 0) continue;
        atomicAdd(&s_acc[0][at], up);
        if (cnt == 1) atomicAdd(&s_acc[1][at], up);
      }
      __syncthreads();
      for (uint32_t c = tid; c < cn; c += kSupThreads) {
        f_out[cb + c] = (int64_t)s_acc[0][c];
        s_out[cb + c] = (int64_t)s_acc[1][c];
      }
    }
    __syncthreads();
    if (tid < 4) totals[f * 4 + tid] = (int64_t)s_tot[tid];
    if (lost_bits)
      for (uint32_t w = tid; w < lwords; w += kSupThreads) lost_bits[(size_t)f * lwords + w] = kPrune ? s_lost[w] : 0u;
  }
}

bool support_sizes_ok(const char *who, int n_bits, int64_t n_funcs) {
  if (n_bits < 1 || n_bits > kSupMaxBits || n_funcs < 1) {
    set_error("%s: n_bits %d outside 1..16 or n_funcs %lld < 1", who, n_bits, (long long)n_funcs);
    return false;
  }
  return true;
}

int64_t support_workspace(int n_bits, int64_t n_funcs) {
  return (int64_t)(kSupHeader + support_stride(n_bits) * (size_t)support_groups(n_funcs));
}

}  // namespace

}  // namespace ttnet

extern "C" int64_t ttnet_cover_support_workspace(int n_bits, int64_t n_funcs) {
  if (!ttnet::support_sizes_ok("ttnet_cover_support_workspace", n_bits, n_funcs)) return TTNET_E_INVALID;
  return ttnet::support_workspace(n_bits, n_funcs);
}

extern "C" int ttnet_cover_support(const uint32_t *cubes_dev, const int32_t *counts_dev, int64_t cube_cap, const uint8_t *keep_dev,
                                   const int64_t *usage_dev, const int32_t *usage_row_dev, int64_t n_usage_rows, int n_bits,
                                   int64_t n_funcs, int64_t *hits_dev, int64_t *first_dev, int64_t *sole_dev, int64_t *totals_dev,
                                   uint32_t *lost_bits_dev, void *work_dev, int64_t work_bytes, void *stream) {
  using namespace ttnet;
  const char *who = "ttnet_cover_support";
  if (!cubes_dev || !counts_dev || !usage_dev || !usage_row_dev || !hits_dev || !first_dev || !sole_dev || !totals_dev || !work_dev) {
    set_error("%s: NULL pointer", who);
    return TTNET_E_INVALID;
  }
  if (!support_sizes_ok(who, n_bits, n_funcs)) return TTNET_E_INVALID;
  if (cube_cap < 1 || cube_cap > INT32_MAX || n_usage_rows < 0) {
    set_error("%s: cube_cap %lld outside 1..2^31-1 or n_usage_rows %lld < 0", who, (long long)cube_cap, (long long)n_usage_rows);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)cubes_dev | (uintptr_t)counts_dev | (uintptr_t)usage_row_dev | (uintptr_t)lost_bits_dev) % 4 ||
      ((uintptr_t)usage_dev | (uintptr_t)hits_dev | (uintptr_t)first_dev | (uintptr_t)sole_dev | (uintptr_t)totals_dev) % 8 ||
      (uintptr_t)work_dev % 16) {
    set_error("%s: the cubes, counts, rows and bitmap must be 4-byte aligned, the int64 buffers 8-byte, the workspace 16-byte", who);
    return TTNET_E_INVALID;
  }
  const int64_t need = support_workspace(n_bits, n_funcs);
  if (work_bytes < need) {
    set_error("%s: workspace of %lld bytes, %lld needed (ttnet_cover_support_workspace)", who, (long long)work_bytes, (long long)need);
    return TTNET_E_INVALID;
  }
  TT_HIP(hipMemsetAsync(work_dev, 0, kSupHeader, (hipStream_t)stream));          // the count of bad usage rows
  auto kernel = keep_dev ? support_kernel<true> : support_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)support_groups(n_funcs)), dim3(kSupThreads), 0, (hipStream_t)stream, cubes_dev, counts_dev,
                     cube_cap, keep_dev, usage_dev, usage_row_dev, n_usage_rows, n_bits, n_funcs, hits_dev, first_dev, sole_dev,
                     totals_dev, lost_bits_dev, (uint8_t *)work_dev, support_stride(n_bits));
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}
