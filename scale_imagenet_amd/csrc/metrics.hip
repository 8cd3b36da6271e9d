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

// One wave per row.  The row starts at any 4-byte address (n_classes = 1001, 10, ..): up to 3 head elements bring it
// to 16 bytes, nv float4 follow, up to 3 tail elements end it; lanes 0..5 take the head / tail elements one each.
// CACHED: nv <= 64 * kCachedVecs, the float4 stay in registers between the two passes; otherwise they are read twice.
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
  const int head = min(C, (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));
  const int nv = (C - head) >> 2;
  const int tail0 = head + 4 * nv;
  const int nedge = head + (C - tail0);                  // <= 6
  const float4 *pv = reinterpret_cast<const float4 *>(p + head);

  const bool has_edge = lane < nedge;
  const int ej = lane < head ? lane : tail0 + (lane - head);
  const float ev = has_edge ? p[ej] : 0.0f;

  float m = -INFINITY;
  uint32_t cnt = 0;                                      // elements ranked before the target: larger, or equal at a lower index
  bool nan = false;
  auto pass1 = [&](float v, int j) {
    m = fmaxf(m, v);
    nan |= v != v;
    cnt += (v > vt || (v == vt && j < t)) ? 1u : 0u;
  };
  if (has_edge) pass1(ev, ej);
  float4 r[kCachedVecs];
  if constexpr (CACHED) {
#pragma unroll
    for (int k = 0; k < kCachedVecs; ++k) {
      const int vi = lane + 64 * k;
      if (vi < nv) {
        r[k] = pv[vi];
        const int j = head + 4 * vi;
        pass1(r[k].x, j), pass1(r[k].y, j + 1), pass1(r[k].z, j + 2), pass1(r[k].w, j + 3);
      }
    }
  } else {
    for (int vi = lane; vi < nv; vi += 64) {
      const float4 q = pv[vi];
      const int j = head + 4 * vi;
      pass1(q.x, j), pass1(q.y, j + 1), pass1(q.z, j + 2), pass1(q.w, j + 3);
    }
  }
  m = wave_max(m);
  cnt = wave_sum_u32(cnt);
  const bool any_nan = __ballot(nan) != 0;

  // float64 sum of exp(v - max): per lane in element order, then the butterfly
  const double md = (double)m;
  double s = 0.0;
  if (has_edge) s += exp((double)ev - md);
  if constexpr (CACHED) {
#pragma unroll
    for (int k = 0; k < kCachedVecs; ++k) {
      if (lane + 64 * k < nv) {
        s += exp((double)r[k].x - md);
        s += exp((double)r[k].y - md);
        s += exp((double)r[k].z - md);
        s += exp((double)r[k].w - md);
      }
    }
  } else {
    for (int vi = lane; vi < nv; vi += 64) {
      const float4 q = pv[vi];
      s += exp((double)q.x - md);
      s += exp((double)q.y - md);
      s += exp((double)q.z - md);
      s += exp((double)q.w - md);
    }
  }
  s = wave_sum_f64(s);
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
      o.loss = log(s) + md - (double)vt;
      o.rank = (int32_t)cnt;
    }
    out[row] = o;
  }
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
