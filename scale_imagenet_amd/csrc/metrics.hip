// ttnet_eval_metrics: cross-entropy loss and top-1 / top-5 hits of a batch of logits, reduced on the device into a
// small accumulator (include/ttnet.h).  Replaces criterion(outputs, targets) + accuracy(outputs, targets, (1, 5)) +
// AverageMeter.update of the reference's test() (main.py:262-268, utils/bar_show.py:110-148).
//
// Two launches on the caller's stream:
//   eval_rows_kernel    one wave per row: max, rank count and float64 exp-sum from registers (rows of up to 1024
//                       classes are read once, 16-byte loads) -> per-image record {double loss, int32 rank}
//   eval_reduce_kernel  one workgroup: the records summed in a fixed order (thread t takes images t, t + 1024, ..
//                       in order; then a fixed butterfly over the lanes and the 16 waves in order) and ADDED to the
//                       accumulator by one thread.  No floating-point atomics: same batches, same bits.
//
// ttnet_topk_rows and ttnet_class_counts (one launch each) answer "what did it say about each image" and "which classes
// fail" from the same rows: topk_rows_kernel shares the row walk and the float64 exp-sum of eval_rows_kernel, so a
// record's logprob is bit for bit the negative of the loss eval_rows_kernel reports for that class as the target.
#include <math.h>

#include <mutex>

#include "ttnet_common.h"

namespace ttnet {
namespace {

struct PerImage {
  double loss;
  int32_t rank;
  int32_t pad;
};
static_assert(sizeof(PerImage) == 16, "per-image record is 16 bytes (ttnet.h)");
struct TopkRecord {
  int32_t cls;
  float logit;
  double logprob;
};
static_assert(sizeof(TopkRecord) == 16, "top-k record is 16 bytes (ttnet.h)");
static_assert(sizeof(ttnet_eval_acc) == 64, "accumulator is 64 bytes (ttnet.h)");

constexpr int kRowsPerBlock = 4;          // waves of eval_rows_kernel's workgroup
constexpr int kCachedVecs = 4;            // float4 per lane a wave keeps in registers: rows of up to 1027 classes
constexpr int kReduceThreads = 1024;

// the value of lane l ^ S: DPP inside a row of 16 lanes, ds_swizzle across rows of a half wave, one bpermute across halves
template <int S>
__device__ inline uint32_t lane_xor(uint32_t v) {
  if constexpr (S < 16) return lane_xor16<S>(v);
  else if constexpr (S == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (16 << 10));
  else return (uint32_t)__shfl_xor((int)v, 32);
}
template <int S>
__device__ inline double lane_xor_f64(double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  const uint64_t r = (uint64_t)lane_xor<S>((uint32_t)b) | ((uint64_t)lane_xor<S>((uint32_t)(b >> 32)) << 32);
  return __builtin_bit_cast(double, r);
}
// butterflies over the 64 lanes (distance 1, 2, .. 32): every lane ends with the same bits, in the same order each run
__device__ inline float wave_max(float v) {
  static_for<0, 6>([&](auto i) {
    constexpr int S = 1 << decltype(i)::value;
    v = fmaxf(v, __builtin_bit_cast(float, lane_xor<S>(__builtin_bit_cast(uint32_t, v))));
  });
  return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
  static_for<0, 6>([&](auto i) {
    constexpr int S = 1 << decltype(i)::value;
    v += lane_xor<S>(v);
  });
  return v;
}
__device__ inline double wave_sum_f64(double v) {
  static_for<0, 6>([&](auto i) {
    constexpr int S = 1 << decltype(i)::value;
    v += lane_xor_f64<S>(v);
  });
  return v;
}

// A wave's view of one row.  The row starts at any 4-byte address (n_classes = 1001, 10, ..): up to 3 head elements bring
// it to 16 bytes, nv float4 follow, up to 3 tail elements end it; lanes 0..5 take the head / tail elements one each.
struct Row {
  const float *p;
  const float4 *pv;
  int head, nv;
  bool has_edge;                                         // this lane holds one of the <= 6 head / tail elements:
  int ej;                                                //   its index
  float ev;                                              //   and its value
};
__device__ inline Row row_view(const float *p, int C, int lane) {
  Row w;
  w.p = p;
  w.head = min(C, (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));
  w.nv = (C - w.head) >> 2;
  const int tail0 = w.head + 4 * w.nv;
  const int nedge = w.head + (C - tail0);                // <= 6
  w.pv = reinterpret_cast<const float4 *>(p + w.head);
  w.has_edge = lane < nedge;
  w.ej = lane < w.head ? lane : tail0 + (lane - w.head);
  w.ev = w.has_edge ? p[w.ej] : 0.0f;
  return w;
}
// f(value, class index) for every element of the row this lane owns, always in the same order: its edge element, then
// its float4 in index order.  CACHED: nv <= 64 * kCachedVecs, the float4 are read by the LOAD pass and stay in the
// registers r for every later pass; otherwise every pass reads them again.
template <bool CACHED, bool LOAD, typename F>
__device__ inline void row_visit(const Row &w, int lane, float4 (&r)[kCachedVecs], F &&f) {
  if (w.has_edge) f(w.ev, w.ej);
  if constexpr (CACHED) {
#pragma unroll
    for (int k = 0; k < kCachedVecs; ++k) {
      const int vi = lane + 64 * k;
      if (vi < w.nv) {
        if constexpr (LOAD) r[k] = w.pv[vi];
        const int j = w.head + 4 * vi;
        f(r[k].x, j), f(r[k].y, j + 1), f(r[k].z, j + 2), f(r[k].w, j + 3);
      }
    }
  } else {
    for (int vi = lane; vi < w.nv; vi += 64) {
      const float4 q = w.pv[vi];
      const int j = w.head + 4 * vi;
      f(q.x, j), f(q.y, j + 1), f(q.z, j + 2), f(q.w, j + 3);
    }
  }
}
// float64 sum of exp(v - max) over the row: per lane in element order, then the butterfly.  The one place the order of
// that sum is written down: the loss of ttnet_eval_metrics and the logprob of ttnet_topk_rows both come from it.
template <bool CACHED>
__device__ inline double row_exp_sum(const Row &w, int lane, float4 (&r)[kCachedVecs], double md) {
  double s = 0.0;
  row_visit<CACHED, false>(w, lane, r, [&](float v, int) { s += exp((double)v - md); });
  return wave_sum_f64(s);
}
// -log softmax of the row at an element of value v, given the row's max and exp-sum (float64)
__device__ inline double row_loss(double s, double md, float v) { return log(s) + md - (double)v; }

// One wave per row.
template <bool CACHED>
__global__ __launch_bounds__(64 * kRowsPerBlock) void eval_rows_kernel(const float *__restrict__ logits,
                                                                       const int64_t *__restrict__ targets, int n, int C,
                                                                       PerImage *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= n) return;                                  // (the whole wave)
  const float *p = logits + (size_t)row * C;
  const int64_t t64 = targets[row];
  const bool bad = t64 < 0 || t64 >= C;                  // never indexes the row
  const int t = bad ? 0 : (int)t64;
  const float vt = p[t];
  const Row w = row_view(p, C, lane);

  float m = -INFINITY;
  uint32_t cnt = 0;                                      // elements ranked before the target: larger, or equal at a lower index
  bool nan = false;
  float4 r[kCachedVecs];
  row_visit<CACHED, true>(w, lane, r, [&](float v, int j) {
    m = fmaxf(m, v);
    nan |= v != v;
    cnt += (v > vt || (v == vt && j < t)) ? 1u : 0u;
  });
  m = wave_max(m);
  cnt = wave_sum_u32(cnt);
  const bool any_nan = __ballot(nan) != 0;

  const double md = (double)m;
  const double s = row_exp_sum<CACHED>(w, lane, r, md);
  if (lane == 0) {
    PerImage o;
    o.pad = 0;
    if (bad) {
      o.loss = 0.0;
      o.rank = -1;
    } else if (any_nan) {
      o.loss = __builtin_nan("");
      o.rank = INT32_MAX;
    } else {
      o.loss = row_loss(s, md, vt);
      o.rank = (int32_t)cnt;
    }
    out[row] = o;
  }
}

// ttnet_topk_rows: one wave per row, k rounds of "the largest element that comes after the one taken last" over the
// row the wave holds in registers (or reads again, past 1027 classes).  The order is total -- larger value first, equal
// values by lower index -- so "after (pv, pj)" needs no marking of taken elements: v < pv, or v == pv and j > pj.  Each
// round is a per-lane scan of its <= 17 elements and one (value, index) butterfly; lane r keeps the winner of round r
// and lanes 0 .. k-1 store the 16-byte records side by side.
__device__ inline bool ranks_before(float v, int j, float bv, int bj) { return v > bv || (v == bv && j < bj); }

template <bool CACHED>
__global__ __launch_bounds__(64 * kRowsPerBlock) void topk_rows_kernel(const float *__restrict__ logits, int n, int C, int K,
                                                                       TopkRecord *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= n) return;                                  // (the whole wave)
  const Row w = row_view(logits + (size_t)row * C, C, lane);

  float m = -INFINITY;
  bool nan = false;
  float4 r[kCachedVecs];
  row_visit<CACHED, true>(w, lane, r, [&](float v, int) {
    m = fmaxf(m, v);
    nan |= v != v;
  });
  m = wave_max(m);
  const bool any_nan = __ballot(nan) != 0;
  const double md = (double)m;
  const double s = row_exp_sum<CACHED>(w, lane, r, md);

  float pv = INFINITY, mine_v = 0.0f;                    // the element taken last; this lane's record
  int pj = -1, mine_j = -1;
  for (int round = 0; round < K; ++round) {              // (K <= n_classes: every round finds an element)
    float bv = -INFINITY;
    int bj = INT32_MAX;                                  // no element yet: any real one, -inf included, ranks before it
    row_visit<CACHED, false>(w, lane, r, [&](float v, int j) {
      const bool after = v < pv || (v == pv && j > pj);
      if (after && ranks_before(v, j, bv, bj)) bv = v, bj = j;
    });
    static_for<0, 6>([&](auto i) {
      constexpr int S = 1 << decltype(i)::value;
      const float ov = __builtin_bit_cast(float, lane_xor<S>(__builtin_bit_cast(uint32_t, bv)));
      const int oj = (int)lane_xor<S>((uint32_t)bj);
      if (ranks_before(ov, oj, bv, bj)) bv = ov, bj = oj;
    });
    pv = bv, pj = bj;
    if (lane == round) mine_v = bv, mine_j = bj;
  }
  if (lane < K) {
    TopkRecord o;
    if (any_nan) {
      o.cls = -1;
      o.logit = __builtin_nanf("");
      o.logprob = __builtin_nan("");
    } else {
      o.cls = mine_j;
      o.logit = mine_v;
      o.logprob = -row_loss(s, md, mine_v);
    }
    out[(size_t)row * K + lane] = o;
  }
}

// ttnet_class_counts: one thread per image, integer atomics only.
__global__ __launch_bounds__(256) void class_counts_kernel(const int64_t *__restrict__ targets, const PerImage *__restrict__ pi,
                                                           const TopkRecord *__restrict__ topk, int n, int K, int C,
                                                           unsigned long long *__restrict__ counts,
                                                           unsigned long long *__restrict__ confusion) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t t = targets[i];
  if (t < 0 || t >= C) return;                           // a bad target: the accumulator leaves the row out, so do we
  const int32_t rank = pi[i].rank;
  if (rank < 0) return;                                  // (the record says the same)
  atomicAdd(&counts[4 * t + 0], 1ull);
  if (rank == 0) atomicAdd(&counts[4 * t + 1], 1ull);
  if (rank < 5) atomicAdd(&counts[4 * t + 2], 1ull);
  const int32_t c = topk[(size_t)i * K].cls;
  if (c < 0 || c >= C) return;                           // a NaN row predicts nothing (class -1)
  atomicAdd(&counts[4 * (size_t)c + 3], 1ull);
  if (confusion) atomicAdd(&confusion[(size_t)t * C + c], 1ull);
}

// ttnet_mean_views: one thread per (image, class); the V addends are read in ascending v (consecutive threads read
// consecutive floats of a row) and summed in float64.
__global__ __launch_bounds__(256) void mean_views_kernel(const float *__restrict__ logits, int64_t total, int V, int C,
                                                         float *__restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;      // i * C + c
  if (j >= total) return;
  const int64_t i = j / C;
  const float *p = logits + (i * V) * C + (j - i * C);
  double s = 0.0;
  for (int v = 0; v < V; ++v) s += (double)p[(int64_t)v * C];
  out[j] = (float)(s / (double)V);
}

__global__ __launch_bounds__(kReduceThreads) void eval_reduce_kernel(const PerImage *__restrict__ pi, int n,
                                                                     ttnet_eval_acc *acc) {
  __shared__ double s_loss[kReduceThreads / 64];
  __shared__ uint32_t s_cnt[3][kReduceThreads / 64];
  double loss = 0.0;
  uint32_t h1 = 0, h5 = 0, bad = 0;
  for (int i = threadIdx.x; i < n; i += kReduceThreads) {
    const PerImage q = pi[i];
    loss += q.loss;
    h1 += q.rank == 0;
    h5 += q.rank >= 0 && q.rank < 5;
    bad += q.rank < 0;
  }
  loss = wave_sum_f64(loss);
  h1 = wave_sum_u32(h1), h5 = wave_sum_u32(h5), bad = wave_sum_u32(bad);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_loss[wave] = loss;
    s_cnt[0][wave] = h1, s_cnt[1][wave] = h5, s_cnt[2][wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0;
    int64_t c[3] = {0, 0, 0};
    for (int w = 0; w < kReduceThreads / 64; ++w) {
      l += s_loss[w];
      c[0] += s_cnt[0][w], c[1] += s_cnt[1][w], c[2] += s_cnt[2][w];
    }
    acc->loss_sum += l;
    acc->images += n - c[2];
    acc->hits1 += c[0];
    acc->hits5 += c[1];
    acc->bad_targets += c[2];
  }
}

// Scratch for callers that pass no per-image buffer: one per accumulator address (calls that add to one accumulator are
// serialised by their stream anyway), allocated the first time that accumulator is seen and kept for the life of the process.
constexpr size_t kScratchBytes = (size_t)65535 * sizeof(PerImage);
constexpr int kMaxScratch = 64;
struct Scratch {
  int device;
  const void *acc;
  void *buf;
};
std::mutex g_scratch_mutex;
std::vector<Scratch> g_scratch;

int scratch_for(const void *acc, hipStream_t s, void **out) {
  int dev = 0;
  TT_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_scratch_mutex);
  for (const Scratch &e : g_scratch)
    if (e.device == dev && e.acc == acc) {
      *out = e.buf;
      return TTNET_OK;
    }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  TT_HIP(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) {
    set_error("eval_metrics: the first call for an accumulator without a per-image buffer allocates its scratch, which a "
              "stream that is capturing cannot do; call it once before the capture or pass per_image_dev");
    return TTNET_E_STATE;
  }
  if ((int)g_scratch.size() >= kMaxScratch) {
    set_error("eval_metrics: more than %d accumulators without a per-image buffer of their own; pass per_image_dev", kMaxScratch);
    return TTNET_E_NOMEM;
  }
  void *buf = nullptr;
  TT_HIP(hipMalloc(&buf, kScratchBytes));
  g_scratch.push_back({dev, acc, buf});
  *out = buf;
  return TTNET_OK;
}

}  // namespace
}  // namespace ttnet

using namespace ttnet;

extern "C" int ttnet_eval_metrics(const float *logits_dev, const int64_t *targets_dev, int64_t n, int64_t n_classes,
                                  ttnet_eval_acc *acc_dev, void *per_image_dev, void *stream) {
  if (!logits_dev || !targets_dev || !acc_dev || n < 1 || n > 65535 || n_classes < 2 || n_classes > 65536) {
    set_error("eval_metrics: bad argument (n %lld in [1, 65535], n_classes %lld in [2, 65536], no NULL but per_image_dev)",
              (long long)n, (long long)n_classes);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)logits_dev & 3) || ((uintptr_t)targets_dev & 7) || ((uintptr_t)acc_dev & 7) || ((uintptr_t)per_image_dev & 7)) {
    set_error("eval_metrics: the logits must be 4-byte aligned, the targets, the accumulator and the per-image buffer 8-byte aligned");
    return TTNET_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  void *pi = per_image_dev;
  if (!pi) TT_TRY(scratch_for(acc_dev, s, &pi));
  const int C = (int)n_classes;
  const dim3 grid((unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
  if ((C >> 2) <= 64 * kCachedVecs)
    hipLaunchKernelGGL(eval_rows_kernel<true>, grid, block, 0, s, logits_dev, targets_dev, (int)n, C, (PerImage *)pi);
  else
    hipLaunchKernelGGL(eval_rows_kernel<false>, grid, block, 0, s, logits_dev, targets_dev, (int)n, C, (PerImage *)pi);
  hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, s, (const PerImage *)pi, (int)n, acc_dev);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

extern "C" int ttnet_topk_rows(const float *logits_dev, int64_t n, int64_t n_classes, int64_t k, void *topk_dev, void *stream) {
  if (!logits_dev || !topk_dev || n < 1 || n > 65535 || n_classes < 2 || n_classes > 65536 || k < 1 || k > TTNET_TOPK_MAX ||
      k > n_classes) {
    set_error("topk_rows: bad argument (n %lld in [1, 65535], n_classes %lld in [2, 65536], k %lld in [1, min(n_classes, %d)], "
              "no NULL)", (long long)n, (long long)n_classes, (long long)k, TTNET_TOPK_MAX);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)logits_dev & 3) || ((uintptr_t)topk_dev & 7)) {
    set_error("topk_rows: the logits must be 4-byte aligned, the records 8-byte aligned");
    return TTNET_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  const int C = (int)n_classes;
  const dim3 grid((unsigned)((n + kRowsPerBlock - 1) / kRowsPerBlock)), block(64 * kRowsPerBlock);
  if ((C >> 2) <= 64 * kCachedVecs)
    hipLaunchKernelGGL(topk_rows_kernel<true>, grid, block, 0, s, logits_dev, (int)n, C, (int)k, (TopkRecord *)topk_dev);
  else
    hipLaunchKernelGGL(topk_rows_kernel<false>, grid, block, 0, s, logits_dev, (int)n, C, (int)k, (TopkRecord *)topk_dev);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

extern "C" int ttnet_class_counts(const int64_t *targets_dev, const void *per_image_dev, const void *topk_dev, int64_t n,
                                  int64_t k, int64_t n_classes, int64_t *counts_dev, int64_t *confusion_dev, void *stream) {
  if (!targets_dev || !per_image_dev || !topk_dev || !counts_dev || n < 1 || n > 65535 || n_classes < 2 || n_classes > 65536 ||
      k < 1 || k > TTNET_TOPK_MAX || k > n_classes) {
    set_error("class_counts: bad argument (n %lld in [1, 65535], n_classes %lld in [2, 65536], k %lld in [1, min(n_classes, %d)], "
              "no NULL but confusion_dev)", (long long)n, (long long)n_classes, (long long)k, TTNET_TOPK_MAX);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)targets_dev & 7) || ((uintptr_t)per_image_dev & 7) || ((uintptr_t)topk_dev & 7) || ((uintptr_t)counts_dev & 7) ||
      ((uintptr_t)confusion_dev & 7)) {
    set_error("class_counts: every buffer must be 8-byte aligned");
    return TTNET_E_INVALID;
  }
  hipLaunchKernelGGL(class_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, targets_dev,
                     (const PerImage *)per_image_dev, (const TopkRecord *)topk_dev, (int)n, (int)k, (int)n_classes,
                     (unsigned long long *)counts_dev, (unsigned long long *)confusion_dev);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

extern "C" int ttnet_mean_views(const float *logits_dev, int64_t n, int64_t V, int64_t C, float *out_dev, void *stream) {
  if (!logits_dev || !out_dev || n < 1 || V < 1 || V > TTNET_VIEWS_MAX || n * V > (int64_t)65535 * TTNET_VIEWS_MAX || C < 1 ||
      C > 65536) {
    set_error("mean_views: bad argument (n %lld >= 1, V %lld in [1, %d], C %lld in [1, 65536], no NULL)", (long long)n,
              (long long)V, TTNET_VIEWS_MAX, (long long)C);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)logits_dev & 3) || ((uintptr_t)out_dev & 3)) {
    set_error("mean_views: both buffers must be 4-byte aligned");
    return TTNET_E_INVALID;
  }
  const int64_t total = n * C;
  hipLaunchKernelGGL(mean_views_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits_dev,
                     total, (int)V, (int)C, out_dev);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}
