// Two-level minimisation of truth tables with don't-cares (ttnet_minimise_covers): a prime, irredundant cover of
// every function of a batch, the four steps of include/ttnet.h (expand, order, cover, irredundant).
//
// One workgroup of four waves per function, a grid of at most kMinGroups workgroups striding over the functions.
//   LDS (24.4 KB, so six workgroups share a CU): the ON and OFF bitmaps of the function (2^n bits each, 8 KB at
//   n = 16) and a third bitmap of the same size, "covered" in step 3 and "removed" in step 4.
//   Workspace (8 bytes per pattern and workgroup, 512 KB at n = 16): cand[2^n] uint32, the cube of every ON minterm;
//   order[2^n] uint16, the minterms in step-2 order, compacted in place to the kept ones by step 3; cover[2^n]
//   uint16, how many kept cubes hold each ON pattern.  A pattern lies in at most ON-count kept cubes and ON-count
//   <= 2^16 - 1 whenever OFF is not empty, so uint16 cannot overflow.
//
// A cube (mask, value) with free variables F = ~mask is walked word-parallel: the free variables among the low five
// index bits become one in-word mask (the same for every word of the cube); the lowest six free bits of the word
// index are spread over the lanes of a wave, the remaining (at most five) are stepped with s = (s - rest) & rest.
// So one wave tests 64 words of the OFF bitmap per step, and a cube takes at most 32 steps.
//   step 1  all four waves, one ON minterm per wave at a time, n sibling tests each.
//   step 2  a counting sort over the n + 1 size classes: every wave owns a contiguous range of patterns, counts its
//           classes, one thread turns the counts into bases (class descending, wave ascending), and every wave
//           places its candidates with ballot ranks -- stable in the minterm index.
//   steps 3, 4 and the output are sequential over cubes by definition: wave 0 walks them, 64 words of a cube per
//           step, while the workgroups that share the CU expand other functions.
// Every loop is bounded by n, 2^n or the ON count; every store to the cubes is guarded by the cap; integers only.

#include "ttnet_common.h"

namespace ttnet {

namespace {

constexpr int kMinThreads = 256;
constexpr int kMinWaves = kMinThreads / kWave;
constexpr int kMinMaxBits = 16;
constexpr int kMinMaxWords = 1 << (kMinMaxBits - 5);
constexpr int kMinGroups = 1024;                    // four per CU: the workspace is sized for them, not for n_funcs
constexpr int kMinClasses = kMinMaxBits + 1;

size_t minimise_stride(int n_bits) { return (((size_t)8 << n_bits) + 255) & ~(size_t)255; }
int64_t minimise_groups(int64_t n_funcs) { return std::min<int64_t>(n_funcs, kMinGroups); }

// the words of one cube as a wave sees them
struct CubeWalk {
  uint32_t inword;   // the cube's patterns inside each of its words
  uint32_t word;     // this lane's word for s = 0
  uint32_t rest;     // free word-index bits left to the loop
  bool active;       // this lane has a word
};

// base: a pattern of the cube with every free bit zero; free_bits: the cube's free index bits
__device__ inline CubeWalk cube_walk(uint32_t base, uint32_t free_bits, uint32_t lane) {
  CubeWalk c;
  uint32_t m = 1u << (base & 31);
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if ((free_bits >> k) & 1) m |= m << (1u << k);
  c.inword = m;
  uint32_t t = free_bits >> 5, sub = 0, used = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const uint32_t low = t & (0u - t);
    if ((lane >> i) & 1) sub |= low;
    used += t != 0;
    t &= t - 1;
  }
  c.word = (base >> 5) | sub;
  c.rest = t;
  c.active = lane < (1u << used);
  return c;
}

// what one lane wrote, another lane of the same wave reads next: LDS and (through the CU's own L1) the workspace
__device__ inline void wave_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ void __launch_bounds__(kMinThreads)
minimise_kernel(const uint32_t *__restrict__ on_g, const uint32_t *__restrict__ dc_g, int n, int64_t n_funcs, uint32_t *__restrict__ cubes,
                int64_t cap, int32_t *__restrict__ counts, uint8_t *__restrict__ work, size_t stride) {
  __shared__ uint32_t s_on[kMinMaxWords], s_off[kMinMaxWords], s_cov[kMinMaxWords];
  __shared__ uint32_t s_cls[kMinWaves][kMinClasses];
  __shared__ uint32_t s_tot[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t npat = 1u << n, full = npat - 1, nwords = npat >= 32 ? npat >> 5 : 1, wmask = nwords - 1;
  const uint32_t valid = n >= 5 ? ~0u : (1u << npat) - 1;
  const uint32_t nchunks = npat >= 64 ? npat >> 6 : 1;
  const uint32_t ch_lo = wave * nchunks / kMinWaves, ch_hi = (wave + 1) * nchunks / kMinWaves;
  uint32_t *cand = (uint32_t *)(work + (size_t)blockIdx.x * stride);
  uint16_t *order = (uint16_t *)(cand + npat);
  uint16_t *cover = order + npat;

  for (int64_t f = blockIdx.x; f < n_funcs; f += gridDim.x) {
    __syncthreads();                                   // the previous function's last LDS reads
    if (tid < 2) s_tot[tid] = 0;
    if (tid < kMinWaves * kMinClasses) (&s_cls[0][0])[tid] = 0;
    __syncthreads();
    uint32_t c_on = 0, c_off = 0;
    for (uint32_t w = tid; w < nwords; w += kMinThreads) {
      const uint32_t on = on_g[(size_t)f * nwords + w] & valid;
      const uint32_t dc = dc_g ? dc_g[(size_t)f * nwords + w] : 0u;
      const uint32_t off = ~(on | dc) & valid;
      s_on[w] = on;
      s_off[w] = off;
      s_cov[w] = 0;
      c_on += __popc(on);
      c_off += __popc(off);
    }
    for (uint32_t i = tid; i < npat / 2; i += kMinThreads) ((uint32_t *)cover)[i] = 0;     // npat uint16
    if (c_on) atomicAdd(&s_tot[0], c_on);
    if (c_off) atomicAdd(&s_tot[1], c_off);
    __syncthreads();
    const uint32_t n_on = s_tot[0], n_off = s_tot[1];
    if (n_on == 0 || n_off == 0) {                     // constant 0: no cube; constant 1: the cube without a literal
      if (tid == 0) {
        if (n_on && cap > 0) cubes[(size_t)f * cap] = 0;
        counts[f] = n_on ? 1 : 0;
      }
      continue;
    }

    // ---- step 1: expand every ON minterm, literals dropped in the order x_0 .. x_{n-1} -------------------------
    for (uint32_t w = wave; w < nwords; w += kMinWaves) {
      uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_on[w]);
      while (bits) {
        const uint32_t m = (w << 5) | (uint32_t)__builtin_ctz(bits);
        bits &= bits - 1;
        uint32_t mask = full, value = m;
        for (int j = 0; j < n; ++j) {
          const uint32_t bit = 1u << (n - 1 - j);
          const CubeWalk c = cube_walk(value ^ bit, ~mask & full, lane);      // the sibling half
          bool blocked = false;
          uint32_t s = 0;
          do {
            const bool hit = c.active && (s_off[(c.word | s) & wmask] & c.inword) != 0;
            if (__ballot(hit)) {
              blocked = true;
              break;
            }
            s = (s - c.rest) & c.rest;
          } while (s);
          if (!blocked) {
            mask &= ~bit;
            value &= ~bit;
          }
        }
        if (lane == 0) cand[m] = (mask << 16) | value;
      }
    }
    __syncthreads();

    // ---- step 2: counting sort by free variables (descending), stable in the minterm index ------------------------
    for (uint32_t ch = ch_lo; ch < ch_hi; ++ch) {
      const uint32_t p = (ch << 6) | lane;
      if (p < npat && ((s_on[p >> 5] >> (p & 31)) & 1)) atomicAdd(&s_cls[wave][__popc(~(cand[p] >> 16) & full)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (int c = n; c >= 0; --c)
        for (int w = 0; w < kMinWaves; ++w) {
          const uint32_t k = s_cls[w][c];
          s_cls[w][c] = run;
          run += k;
        }
    }
    __syncthreads();
    for (uint32_t ch = ch_lo; ch < ch_hi; ++ch) {
      const uint32_t p = (ch << 6) | lane;
      const bool v = p < npat && ((s_on[p >> 5] >> (p & 31)) & 1);
      const uint32_t cls = v ? (uint32_t)__popc(~(cand[p] >> 16) & full) : 0u;
      uint64_t todo = __ballot(v);
      for (int r = 0; r <= n && todo; ++r) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cls, leader);
        const bool mine = v && cls == c;
        const uint64_t same = __ballot(mine);
        const uint32_t at = s_cls[wave][c];
        if (mine) order[(at + (uint32_t)__popcll(same & (((uint64_t)1 << lane) - 1))) & full] = (uint16_t)p;
        wave_handoff();
        if (lane == (uint32_t)leader) s_cls[wave][c] = at + (uint32_t)__popcll(same);
        wave_handoff();
        todo &= ~same;
      }
    }
    __syncthreads();

    if (wave == 0) {
      // ---- step 3: keep a cube iff it holds an ON minterm that no kept cube holds yet -----------------------------
      uint32_t nkept = 0;
      for (uint32_t i0 = 0; i0 < n_on; i0 += 64) {
        const uint32_t here = min(64u, n_on - i0);
        const uint32_t my_m = lane < here ? (uint32_t)order[i0 + lane] & full : 0u;
        const uint32_t my_key = lane < here ? cand[my_m] : 0u;
        for (uint32_t j = 0; j < here; ++j) {
          const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)my_key, (int)j);
          const CubeWalk c = cube_walk(key & 0xFFFFu, ~(key >> 16) & full, lane);
          bool fresh = false;
          uint32_t s = 0;
          do {
            const uint32_t w = (c.word | s) & wmask;
            const bool hit = c.active && (s_on[w] & ~s_cov[w] & c.inword) != 0;
            if (__ballot(hit)) {
              fresh = true;
              break;
            }
            s = (s - c.rest) & c.rest;
          } while (s);
          if (!fresh) continue;
          s = 0;
          do {
            if (c.active) {
              const uint32_t w = (c.word | s) & wmask;
              uint32_t b = s_on[w] & c.inword;
              s_cov[w] |= b;
              while (b) {
                cover[(w << 5) | (uint32_t)__builtin_ctz(b)] += 1;
                b &= b - 1;
              }
            }
            s = (s - c.rest) & c.rest;
          } while (s);
          if (lane == 0) order[nkept] = (uint16_t)__builtin_amdgcn_readlane((int)my_m, (int)j);    // nkept <= i0 + j: in place
          ++nkept;
          wave_handoff();
        }
      }
      // ---- step 4: in reverse, drop a cube whose every ON minterm lies in another kept cube ------------------------
      for (uint32_t w = lane; w < nwords; w += 64) s_cov[w] = 0;          // now: bit k = kept cube k was removed
      wave_handoff();
      for (uint32_t top = nkept; top > 0;) {
        const uint32_t here = min(64u, top), i0 = top - here;
        const uint32_t my_key = lane < here ? cand[(uint32_t)order[i0 + lane] & full] : 0u;
        for (uint32_t j = here; j-- > 0;) {
          const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)my_key, (int)j);
          const CubeWalk c = cube_walk(key & 0xFFFFu, ~(key >> 16) & full, lane);
          bool needed = false;
          uint32_t s = 0;
          do {
            bool alone = false;
            if (c.active) {
              const uint32_t w = (c.word | s) & wmask;
              uint32_t b = s_on[w] & c.inword;
              while (b) {
                alone |= cover[(w << 5) | (uint32_t)__builtin_ctz(b)] < 2;
                b &= b - 1;
              }
            }
            if (__ballot(alone)) {
              needed = true;
              break;
            }
            s = (s - c.rest) & c.rest;
          } while (s);
          if (needed) continue;
          s = 0;
          do {
            if (c.active) {
              const uint32_t w = (c.word | s) & wmask;
              uint32_t b = s_on[w] & c.inword;
              while (b) {
                cover[(w << 5) | (uint32_t)__builtin_ctz(b)] -= 1;
                b &= b - 1;
              }
            }
            s = (s - c.rest) & c.rest;
          } while (s);
          if (lane == 0) s_cov[((i0 + j) >> 5) & wmask] |= 1u << ((i0 + j) & 31);
          wave_handoff();
        }
        top = i0;
      }
      // ---- output: the survivors in step-2 order; the true count, cubes only below the cap ---------------------------
      uint32_t n_out = 0;
      for (uint32_t i0 = 0; i0 < nkept; i0 += 64) {
        const uint32_t k = i0 + lane;
        const bool alive = k < nkept && !((s_cov[(k >> 5) & wmask] >> (k & 31)) & 1);
        const uint64_t b = __ballot(alive);
        const uint32_t pos = n_out + (uint32_t)__popcll(b & (((uint64_t)1 << lane) - 1));
        if (alive && (int64_t)pos < cap) cubes[(size_t)f * cap + pos] = cand[(uint32_t)order[k] & full];
        n_out += (uint32_t)__popcll(b);
      }
      if (lane == 0) counts[f] = (int32_t)n_out;
    }
  }
}

}  // namespace

}  // namespace ttnet

extern "C" int64_t ttnet_minimise_workspace(int n_bits, int64_t n_funcs) {
  using namespace ttnet;
  if (n_bits < 1 || n_bits > kMinMaxBits || n_funcs < 1) {
    set_error("ttnet_minimise_workspace: n_bits %d outside 1..16 or n_funcs %lld < 1", n_bits, (long long)n_funcs);
    return TTNET_E_INVALID;
  }
  return (int64_t)(minimise_stride(n_bits) * (size_t)minimise_groups(n_funcs));
}

extern "C" int ttnet_minimise_covers(const uint32_t *on_dev, const uint32_t *dc_dev, int n_bits, int64_t n_funcs, uint32_t *cubes_dev,
                                     int64_t cube_cap, int32_t *counts_dev, void *work_dev, int64_t work_bytes, void *stream) {
  using namespace ttnet;
  if (!on_dev || !cubes_dev || !counts_dev || !work_dev) {
    set_error("ttnet_minimise_covers: NULL pointer");
    return TTNET_E_INVALID;
  }
  if (n_bits < 1 || n_bits > kMinMaxBits || n_funcs < 1 || cube_cap < 0) {
    set_error("ttnet_minimise_covers: n_bits %d outside 1..16, n_funcs %lld < 1 or cube_cap %lld < 0", n_bits, (long long)n_funcs,
              (long long)cube_cap);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)on_dev | (uintptr_t)dc_dev | (uintptr_t)cubes_dev | (uintptr_t)counts_dev) % 4 || (uintptr_t)work_dev % 16) {
    set_error("ttnet_minimise_covers: the bitmaps, cubes and counts must be 4-byte aligned, the workspace 16-byte aligned");
    return TTNET_E_INVALID;
  }
  const int64_t groups = minimise_groups(n_funcs);
  const size_t stride = minimise_stride(n_bits);
  if (work_bytes < (int64_t)(stride * (size_t)groups)) {
    set_error("ttnet_minimise_covers: workspace of %lld bytes, %lld needed (ttnet_minimise_workspace)", (long long)work_bytes,
              (long long)(stride * (size_t)groups));
    return TTNET_E_INVALID;
  }
  hipLaunchKernelGGL(minimise_kernel, dim3((unsigned)groups), dim3(kMinThreads), 0, (hipStream_t)stream, on_dev, dc_dev, n_bits, n_funcs,
                     cubes_dev, cube_cap, counts_dev, (uint8_t *)work_dev, stride);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}
