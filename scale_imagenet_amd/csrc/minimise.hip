// Two-level minimisation of truth tables with don't-cares: a prime, irredundant cover of every function of a batch.
// ttnet_minimise_covers runs the four steps of include/ttnet.h (expand, order, cover, irredundant);
// ttnet_minimise_covers_rounds runs up to eight reduce / expand rounds on top (steps 5 to 9 there) and returns the smallest
// cover met.  Both are one kernel body; the rounds are compiled in or out (minimise_kernel<kRounds>).
//
// One workgroup of four waves per function, a grid of at most kMinGroups workgroups striding over the functions.
//   LDS (24.4 KB, so six workgroups share a CU): the ON and OFF bitmaps of the function (2^n bits each, 8 KB at
//   n = 16) and a third bitmap of the same size, "covered" in step 3 and "removed" in step 4.
//   Workspace (8 bytes per pattern and workgroup, 512 KB at n = 16): cand[2^n] uint32, the cube of every ON minterm;
//   order[2^n] uint16, the minterms in step-2 order, compacted in place to the kept ones by step 3; cover[2^n]
//   uint16, how many kept cubes hold each ON pattern.  A pattern lies in at most ON-count kept cubes and ON-count
//   <= 2^16 - 1 whenever OFF is not empty, so uint16 cannot overflow.  With rounds, 8 bytes more: list[2^n] and
//   best[2^n] uint32, key lists (a cover has at most ON-count cubes).  The cover in hand lies in list or, once step 2 is
//   done with it, in cand, by turns; order[] then holds positions in that list instead of minterms.
//
// A cube (mask, value) with free variables F = ~mask is walked word-parallel: the free variables among the low five
// index bits become one in-word mask (the same for every word of the cube); the lowest six free bits of the word
// index are spread over the lanes of a wave, the remaining (at most five) are stepped with s = (s - rest) & rest.
// So one wave tests 64 words of the OFF bitmap per step, and a cube takes at most 32 steps.
//   steps 1, 7  all four waves, one cube per wave at a time (an ON minterm, or a reduced cube), at most n sibling tests each.
//   steps 2, 8  a counting sort over the n + 1 size classes: every wave owns a contiguous range of items (patterns, or
//           positions of the cover), counts its classes, one thread turns the counts into bases (class descending, wave
//           ascending), and every wave places its items with ballot ranks -- stable in the item.
//   steps 3, 4, 6 and the output are sequential over cubes by definition: wave 0 walks them, 64 words of a cube per
//           step, while the workgroups that share the CU expand other functions.  Step 5 costs nothing: cover[] after
//           step 4 is the count it asks for.
// Every loop is bounded by n, 2^n, the ON count or the rounds; every store to the cubes is guarded by the cap; integers only.

#include "ttnet_common.h"

namespace ttnet {

namespace {

constexpr int kMinThreads = 256;
constexpr int kMinWaves = kMinThreads / kWave;
constexpr int kMinMaxBits = 16;
constexpr int kMinMaxWords = 1 << (kMinMaxBits - 5);
constexpr int kMinGroups = 1024;                    // four per CU: the workspace is sized for them, not for n_funcs
constexpr int kMinClasses = kMinMaxBits + 1;

constexpr int kMinMaxRounds = 8;
constexpr int kMinBytes = 8, kMinRoundsBytes = 16;  // workspace per pattern and workgroup: without and with the two key lists

size_t minimise_stride(int n_bits, int per_pattern) { return (((size_t)per_pattern << n_bits) + 255) & ~(size_t)255; }
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

// what the whole kernel knows about the function in hand
struct Func {
  const uint32_t *s_on, *s_off;
  int n;
  uint32_t full, nwords, wmask, lane;
};

// steps 1 and 7, one wave: drop every literal of the cube whose sibling half holds no OFF pattern, x_0 first or x_{n-1} first
__device__ inline uint32_t expand(const Func &fn, uint32_t mask, uint32_t value, bool x0_first) {
  for (int j = 0; j < fn.n; ++j) {
    const uint32_t bit = 1u << (x0_first ? fn.n - 1 - j : j);
    if (!(mask & bit)) continue;
    const CubeWalk c = cube_walk(value ^ bit, ~mask & fn.full, fn.lane);      // the sibling half
    bool blocked = false;
    uint32_t s = 0;
    do {
      const bool hit = c.active && (fn.s_off[(c.word | s) & fn.wmask] & c.inword) != 0;
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
  return (mask << 16) | value;
}

// steps 2 and 8, all four waves: order[] = the items of keys[] by free variables, descending, stable in the item.  The items
// are the ON minterms (kCover false: keys = cand) or the positions 0 .. n_items - 1 of a cover.  A counting sort over the n + 1
// size classes: every wave owns a contiguous range of items, counts its classes, one thread turns the counts into bases (class
// descending, wave ascending), and every wave places its items with ballot ranks.  Ends behind a barrier.
template <bool kCover>
__device__ inline void order_by_size(const Func &fn, const uint32_t *keys, uint32_t n_items, uint32_t (*s_cls)[kMinClasses],
                                     uint16_t *order) {
  const uint32_t tid = threadIdx.x, lane = fn.lane, wave = tid >> 6, full = fn.full;
  const uint32_t nchunks = (n_items + 63) >> 6;
  const uint32_t ch_lo = wave * nchunks / kMinWaves, ch_hi = (wave + 1) * nchunks / kMinWaves;
  if (tid < kMinWaves * kMinClasses) (&s_cls[0][0])[tid] = 0;
  __syncthreads();
  for (uint32_t ch = ch_lo; ch < ch_hi; ++ch) {
    const uint32_t p = (ch << 6) | lane;
    if (p < n_items && (kCover || ((fn.s_on[p >> 5] >> (p & 31)) & 1))) atomicAdd(&s_cls[wave][__popc(~(keys[p] >> 16) & full)], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int c = fn.n; c >= 0; --c)
      for (int w = 0; w < kMinWaves; ++w) {
        const uint32_t k = s_cls[w][c];
        s_cls[w][c] = run;
        run += k;
      }
  }
  __syncthreads();
  for (uint32_t ch = ch_lo; ch < ch_hi; ++ch) {
    const uint32_t p = (ch << 6) | lane;
    const bool v = p < n_items && (kCover || ((fn.s_on[p >> 5] >> (p & 31)) & 1));
    const uint32_t cls = v ? (uint32_t)__popc(~(keys[p] >> 16) & full) : 0u;
    uint64_t todo = __ballot(v);
    for (int r = 0; r <= fn.n && todo; ++r) {
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
}

// steps 3 and 4, wave 0: walks keys[order[0 .. n_items)]; s_cov and cover come in zeroed.  Leaves the kept items in
// order[0 .. nkept), bit k of s_cov = kept item k was removed again, cover[p] = how many surviving cubes hold ON pattern p.
__device__ inline uint32_t cover_irredundant(const Func &fn, const uint32_t *keys, uint32_t n_items, uint16_t *order, uint16_t *cover,
                                             uint32_t *s_cov) {
  const uint32_t lane = fn.lane, full = fn.full, wmask = fn.wmask;
  const uint32_t *s_on = fn.s_on;
  // ---- step 3: keep a cube iff it holds an ON minterm that no kept cube holds yet -----------------------------
  uint32_t nkept = 0;
  for (uint32_t i0 = 0; i0 < n_items; i0 += 64) {
    const uint32_t here = min(64u, n_items - i0);
    const uint32_t my_m = lane < here ? (uint32_t)order[i0 + lane] & full : 0u;
    const uint32_t my_key = lane < here ? keys[my_m] : 0u;
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
  for (uint32_t w = lane; w < fn.nwords; w += 64) s_cov[w] = 0;          // now: bit k = kept cube k was removed
  wave_handoff();
  for (uint32_t top = nkept; top > 0;) {
    const uint32_t here = min(64u, top), i0 = top - here;
    const uint32_t my_key = lane < here ? keys[(uint32_t)order[i0 + lane] & full] : 0u;
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
  return nkept;
}

// the survivors of cover_irredundant in their order, wave 0: the true count is returned, cubes are stored only below the cap;
// *literals = the set mask bits of all of them
__device__ inline uint32_t emit(const Func &fn, const uint32_t *keys, const uint16_t *order, uint32_t nkept, const uint32_t *s_cov,
                                uint32_t *dst, int64_t cap, uint32_t *literals) {
  const uint32_t lane = fn.lane;
  uint32_t n_out = 0, lits = 0;
  for (uint32_t i0 = 0; i0 < nkept; i0 += 64) {
    const uint32_t k = i0 + lane;
    const bool alive = k < nkept && !((s_cov[(k >> 5) & fn.wmask] >> (k & 31)) & 1);
    const uint64_t b = __ballot(alive);
    const uint32_t pos = n_out + (uint32_t)__popcll(b & (((uint64_t)1 << lane) - 1));
    if (alive) {
      const uint32_t key = keys[(uint32_t)order[k] & fn.full];
      lits += (uint32_t)__popc(key >> 16);
      if ((int64_t)pos < cap) dst[pos] = key;
    }
    n_out += (uint32_t)__popcll(b);
  }
  for (int d = 1; d < kWave; d <<= 1) lits += (uint32_t)__shfl_xor((int)lits, d);
  *literals = lits;
  return n_out;
}

// steps 5 and 6, wave 0: every cube of list[0 .. nk), from the last to the first, shrinks to the smallest cube that holds its
// ON patterns of count 1 (never none: the cover is irredundant, and a count only falls for patterns a cube leaves), and the
// patterns it leaves lose one count.  A pattern p travels as p | ~p << 16, so one OR over the wave gives both the bits some
// pattern has set and the bits some pattern has clear; a literal stands where only one of the two holds.
__device__ inline void reduce(const Func &fn, uint32_t *list, uint32_t nk, uint16_t *cover) {
  const uint32_t lane = fn.lane, full = fn.full, wmask = fn.wmask;
  for (uint32_t top = nk; top > 0;) {
    const uint32_t here = min(64u, top), i0 = top - here;
    const uint32_t my_key = lane < here ? list[i0 + lane] : 0u;
    for (uint32_t j = here; j-- > 0;) {
      const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)my_key, (int)j);
      const CubeWalk c = cube_walk(key & 0xFFFFu, ~(key >> 16) & full, lane);
      uint32_t acc = 0, s = 0;
      do {
        if (c.active) {
          const uint32_t w = (c.word | s) & wmask;
          uint32_t b = fn.s_on[w] & c.inword;
          while (b) {
            const uint32_t p = (w << 5) | (uint32_t)__builtin_ctz(b);
            if (cover[p] == 1) acc |= p | ((~p & full) << 16);
            b &= b - 1;
          }
        }
        s = (s - c.rest) & c.rest;
      } while (s);
      for (int d = 1; d < kWave; d <<= 1) acc |= (uint32_t)__shfl_xor((int)acc, d);
      const uint32_t mask = ~(acc & (acc >> 16)) & full, value = acc & mask;          // relies on acc != 0: E is never empty
      if (mask == key >> 16) continue;                   // nothing to leave
      s = 0;
      do {
        if (c.active) {
          const uint32_t w = (c.word | s) & wmask;
          uint32_t b = fn.s_on[w] & c.inword;
          while (b) {
            const uint32_t p = (w << 5) | (uint32_t)__builtin_ctz(b);
            if ((p & mask) != value) cover[p] -= 1;
            b &= b - 1;
          }
        }
        s = (s - c.rest) & c.rest;
      } while (s);
      if (lane == 0) list[i0 + j] = (mask << 16) | value;
      wave_handoff();
    }
    top = i0;
  }
}

// kRounds false: the four steps, the cover straight into cubes.  kRounds true: the rounds of ttnet_minimise_covers_rounds on
// top, with two more key lists of 2^n uint32 behind cover[]: round r reads its cover from one of {cand, list} and leaves the next
// in the other; best holds the cover that goes out.
template <bool kRounds>
__global__ void __launch_bounds__(kMinThreads)
minimise_kernel(const uint32_t *__restrict__ on_g, const uint32_t *__restrict__ dc_g, int n, int64_t n_funcs, int rounds,
                uint32_t *__restrict__ cubes, int64_t cap, int32_t *__restrict__ counts, uint8_t *__restrict__ work, size_t stride) {
  __shared__ uint32_t s_on[kMinMaxWords], s_off[kMinMaxWords], s_cov[kMinMaxWords];
  __shared__ uint32_t s_cls[kMinWaves][kMinClasses];
  __shared__ uint32_t s_tot[3];                        // ON count, OFF count, cubes of the current cover
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t npat = 1u << n, full = npat - 1, nwords = npat >= 32 ? npat >> 5 : 1, wmask = nwords - 1;
  const uint32_t valid = n >= 5 ? ~0u : (1u << npat) - 1;
  uint32_t *cand = (uint32_t *)(work + (size_t)blockIdx.x * stride);
  uint16_t *order = (uint16_t *)(cand + npat);
  uint16_t *cover = order + npat;
  uint32_t *list = (uint32_t *)(cover + npat), *best = list + npat;         // kRounds only
  const Func fn = {s_on, s_off, n, full, nwords, wmask, lane};

  for (int64_t f = blockIdx.x; f < n_funcs; f += gridDim.x) {
    __syncthreads();                                   // the previous function's last LDS reads
    if (tid < 2) s_tot[tid] = 0;
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
        const uint32_t key = expand(fn, full, m, true);
        if (lane == 0) cand[m] = key;
      }
    }
    __syncthreads();
    // ---- step 2 ----------------------------------------------------------------------------------------------------
    order_by_size<false>(fn, cand, npat, s_cls, order);

    // ---- steps 3, 4 and the output are sequential over cubes by definition: wave 0 ------------------------------------
    uint32_t best_n = 0, best_lits = 0;                // wave 0, kRounds
    if (wave == 0) {
      const uint32_t nkept = cover_irredundant(fn, cand, n_on, order, cover, s_cov);
      uint32_t lits;
      if (!kRounds) {
        const uint32_t n_out = emit(fn, cand, order, nkept, s_cov, cubes + (size_t)f * cap, cap, &lits);
        if (lane == 0) counts[f] = (int32_t)n_out;
      } else {
        best_n = emit(fn, cand, order, nkept, s_cov, list, npat, &lits);
        best_lits = lits;
        wave_handoff();
        for (uint32_t i = lane; i < best_n; i += 64) best[i] = list[i];
        if (lane == 0) s_tot[2] = best_n;
      }
    }
    if (!kRounds) continue;

    __syncthreads();
    uint32_t nk = s_tot[2];
    uint32_t *src = list, *dst = cand;
    const int todo = nk > 1 ? rounds : 0;              // a one-cube cover goes out as it is
    for (int r = 1; r <= todo; ++r) {
      if (wave == 0) reduce(fn, src, nk, cover);       // steps 5, 6: cover[] is what step 4 left
      __syncthreads();
      // ---- step 7: every reduced cube on its own, x_{n-1} first in odd rounds, x_0 first in even ones ------------------
      for (uint32_t i = wave; i < nk; i += kMinWaves) {
        const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)src[i]);
        const uint32_t grown = expand(fn, key >> 16, key & 0xFFFFu, (r & 1) == 0);
        if (lane == 0) src[i] = grown;
      }
      for (uint32_t w = tid; w < nwords; w += kMinThreads) s_cov[w] = 0;
      for (uint32_t i = tid; i < npat / 2; i += kMinThreads) ((uint32_t *)cover)[i] = 0;
      // ---- step 8: positions instead of minterms, then steps 3 and 4 as they are ------------------------------------------
      order_by_size<true>(fn, src, nk, s_cls, order);
      if (wave == 0) {
        const uint32_t nkept = cover_irredundant(fn, src, nk, order, cover, s_cov);
        uint32_t lits;
        const uint32_t n_out = emit(fn, src, order, nkept, s_cov, dst, npat, &lits);
        wave_handoff();
        if (lits < best_lits || (lits == best_lits && n_out < best_n)) {      // step 9: the earliest of the smallest
          for (uint32_t i = lane; i < n_out; i += 64) best[i] = dst[i];
          best_n = n_out;
          best_lits = lits;
        }
        if (lane == 0) s_tot[2] = n_out;
      }
      __syncthreads();
      nk = s_tot[2];
      uint32_t *t = src;
      src = dst;
      dst = t;
    }
    if (wave == 0) {
      wave_handoff();
      for (uint32_t i = lane; i < best_n && (int64_t)i < cap; i += 64) cubes[(size_t)f * cap + i] = best[i];
      if (lane == 0) counts[f] = (int32_t)best_n;
    }
  }
}

// the argument checks of both entry points and the launch; `per_pattern`: workspace bytes per pattern and workgroup
int minimise_launch(const char *who, const uint32_t *on_dev, const uint32_t *dc_dev, int n_bits, int64_t n_funcs, int rounds,
                    uint32_t *cubes_dev, int64_t cube_cap, int32_t *counts_dev, void *work_dev, int64_t work_bytes, int per_pattern,
                    const char *sizer, void *stream) {
  if (!on_dev || !cubes_dev || !counts_dev || !work_dev) {
    set_error("%s: NULL pointer", who);
    return TTNET_E_INVALID;
  }
  if (n_bits < 1 || n_bits > kMinMaxBits || n_funcs < 1 || cube_cap < 0) {
    set_error("%s: n_bits %d outside 1..16, n_funcs %lld < 1 or cube_cap %lld < 0", who, n_bits, (long long)n_funcs, (long long)cube_cap);
    return TTNET_E_INVALID;
  }
  if (rounds < 0 || rounds > kMinMaxRounds) {
    set_error("%s: rounds %d outside 0..%d", who, rounds, kMinMaxRounds);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)on_dev | (uintptr_t)dc_dev | (uintptr_t)cubes_dev | (uintptr_t)counts_dev) % 4 || (uintptr_t)work_dev % 16) {
    set_error("%s: the bitmaps, cubes and counts must be 4-byte aligned, the workspace 16-byte aligned", who);
    return TTNET_E_INVALID;
  }
  const int64_t groups = minimise_groups(n_funcs);
  const size_t stride = minimise_stride(n_bits, per_pattern);
  if (work_bytes < (int64_t)(stride * (size_t)groups)) {
    set_error("%s: workspace of %lld bytes, %lld needed (%s)", who, (long long)work_bytes, (long long)(stride * (size_t)groups), sizer);
    return TTNET_E_INVALID;
  }
  auto kernel = rounds ? minimise_kernel<true> : minimise_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(kMinThreads), 0, (hipStream_t)stream, on_dev, dc_dev, n_bits, n_funcs, rounds,
                     cubes_dev, cube_cap, counts_dev, (uint8_t *)work_dev, stride);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

int64_t minimise_workspace(const char *who, int n_bits, int64_t n_funcs, int per_pattern) {
  if (n_bits < 1 || n_bits > kMinMaxBits || n_funcs < 1) {
    set_error("%s: n_bits %d outside 1..16 or n_funcs %lld < 1", who, n_bits, (long long)n_funcs);
    return TTNET_E_INVALID;
  }
  return (int64_t)(minimise_stride(n_bits, per_pattern) * (size_t)minimise_groups(n_funcs));
}

}  // namespace

}  // namespace ttnet

extern "C" int64_t ttnet_minimise_workspace(int n_bits, int64_t n_funcs) {
  return ttnet::minimise_workspace("ttnet_minimise_workspace", n_bits, n_funcs, ttnet::kMinBytes);
}

extern "C" int64_t ttnet_minimise_rounds_workspace(int n_bits, int64_t n_funcs) {
  return ttnet::minimise_workspace("ttnet_minimise_rounds_workspace", n_bits, n_funcs, ttnet::kMinRoundsBytes);
}

extern "C" int ttnet_minimise_covers(const uint32_t *on_dev, const uint32_t *dc_dev, int n_bits, int64_t n_funcs, uint32_t *cubes_dev,
                                     int64_t cube_cap, int32_t *counts_dev, void *work_dev, int64_t work_bytes, void *stream) {
  return ttnet::minimise_launch("ttnet_minimise_covers", on_dev, dc_dev, n_bits, n_funcs, 0, cubes_dev, cube_cap, counts_dev, work_dev,
                                work_bytes, ttnet::kMinBytes, "ttnet_minimise_workspace", stream);
}

extern "C" int ttnet_minimise_covers_rounds(const uint32_t *on_dev, const uint32_t *dc_dev, int n_bits, int64_t n_funcs, int rounds,
                                            uint32_t *cubes_dev, int64_t cube_cap, int32_t *counts_dev, void *work_dev, int64_t work_bytes,
                                            void *stream) {
  return ttnet::minimise_launch("ttnet_minimise_covers_rounds", on_dev, dc_dev, n_bits, n_funcs, rounds, cubes_dev, cube_cap, counts_dev,
                                work_dev, work_bytes, ttnet::kMinRoundsBytes, "ttnet_minimise_rounds_workspace", stream);
}
