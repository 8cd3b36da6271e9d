// The eval input transform in front of ttnet_forward_u8, on the GPU:
//   transforms.Resize(256) -> transforms.CenterCrop(224)      (utils/preprocess.py:104-105, main.py:208)
// on decoded uint8 HWC images; ToTensor + Normalize (:106-108) are fused into the stem (stem.hip).
//
// torchvision's Resize of a PIL image is Pillow's Image.resize(..., BILINEAR): a separable
// convolution whose support widens with the down-scaling factor (antialiasing), carried out on uint8
// with 22-bit fixed-point coefficients, horizontal pass first, the intermediate image rounded to
// uint8 (Pillow, src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
// ImagingResampleHorizontal_8bpc / Vertical_8bpc).  This file restates that arithmetic exactly
// (integer for integer); the coefficient tables are built on the host in float64 like Pillow's, the
// two passes run in one kernel that computes only what the centre crop keeps (the intermediate image lives in LDS).
//
// Parity: pinned to Pillow 12.x -- tests/golden/ref_resize.npz holds Pillow's own outputs for seeded images of
// nine geometries (oracle/gen_golden.py resize, run in the build container where Pillow imports) and
// tests/test_gpu_preprocess.py compares these kernels with it byte for byte; tests/golden/ref_resize_paths.json
// (tools/gen_resize_paths_fixture.py) holds Pillow's hashes on the geometries that reach every tap-count instantiation, the
// last partial piece, both sides of the size bounds and the WIDE ragged kernel (tests/test_gpu_resize_paths.py).
// torchvision is not importable:
// its output-size and crop-offset rules are restated.

#include <math.h>

#include <algorithm>

#include <mutex>
#include <vector>

#include "ttnet_common.h"

namespace ttnet {

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

struct Coeffs {
  int ksize = 0;
  std::vector<int> bounds;      // [out][2]: first input index, tap count
  std::vector<int> kk;          // [out][ksize] fixed point
};

// Resample.c: precompute_coeffs (bilinear: support 1) + normalize_coeffs_8bpc
Coeffs precompute(int in_size, int out_size) {
  Coeffs c;
  const double scale = (double)((float)in_size - 0.0f) / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  c.ksize = (int)ceil(support) * 2 + 1;
  c.bounds.resize((size_t)out_size * 2);
  c.kk.assign((size_t)out_size * c.ksize, 0);
  std::vector<double> k(c.ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = 0.0 + (xx + 0.5) * scale, ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      const double w = t < 1.0 ? 1.0 - t : 0.0;
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      c.kk[(size_t)xx * c.ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kPrecisionBits)) : (int)(0.5 + k[x] * (1 << kPrecisionBits));
    }
    c.bounds[2 * xx] = xmin;
    c.bounds[2 * xx + 1] = xmax;
  }
  return c;
}

// clip8 of Resample.c: (v >> 22) saturated to 0..255.  Written as clamp-then-shift: from the shift-then-clamp form hipcc 7.2
// selects gfx950's v_ashr_pk_u8_i32 for two of the four bytes of a packed dword and ORs the other two into the upper half of its
// result, which is not zero there -- bytes 2 and 3 of some dwords came out wrong (tests/test_gpu_preprocess.py caught it).
__device__ inline uint32_t clip8(int v) {
  const int hi = (256 << kPrecisionBits) - 1;
  v = v < 0 ? 0 : (v > hi ? hi : v);
  return (uint32_t)v >> kPrecisionBits;
}

// One launch for both passes (round 3).  A workgroup makes TY output rows of one image: it stages the input rows those rows
// depend on, chunk by chunk, as 16-byte pieces in LDS (only the columns the kept output columns depend on; a thread's loads of a
// chunk are issued together), runs the horizontal pass of a chunk into an LDS image of the intermediate rows -- rounded to
// uint8 exactly as Pillow stores its intermediate image -- and then the vertical pass from that image, four output bytes per
// thread and store.  Both passes loop over the table's tap count (uniform; coefficients beyond a window's own count are zero)
// with the four bytes of a dword side by side, so that eight LDS reads are in flight per step.  Input bytes are read once (plus
// the few rows two neighbouring tiles share), the intermediate image never leaves the chip, nothing is allocated or waited for
// on the host: the call is asynchronous on its stream.  (Round 2: two kernels with a byte per thread, a hipMalloc'ed
// intermediate image, a table upload and a stream synchronisation per call: 615 us for 256 images of 375 x 500; now see
// tools/preproc_bench.py.)
constexpr int RS_TY = 16, RS_CHUNK = 16, RS_THREADS = 256, RS_STAGE_LOADS = 6;      // (a chunk: at most RS_CHUNK rows and RS_STAGE_LOADS x RS_THREADS pieces)
struct ResizeArgs {
  const uint8_t *src;
  uint8_t *dst;
  const int *bh, *kh, *bv, *kv;      // bounds [out][2] and coefficients [out][ksize] of the two passes (device)
  int n, h, w, crop, x0, y0, ksh, ksv;
  int c0, cw;                        // first input column and number of input columns the kept output columns depend on
  int rmax;                          // most intermediate rows a tile needs
  int row_q;                         // 16-byte pieces per staged input row (cw * 3 bytes + alignment slack)
  int chunk;                         // input rows staged at a time
};
// KSH / KSV: the tap counts of the two tables when they are one of 1, 3, 5, 7, 9 (the loops unroll and the byte reads of a
// window get immediate offsets); 0 = any count, at run time.
template <int KSH, int KSV>
__global__ __launch_bounds__(RS_THREADS) void resize_crop_kernel(ResizeArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int im = blockIdx.y, ty = blockIdx.x, tid = threadIdx.x;
  const int ksh = KSH ? KSH : a.ksh, ksv = KSV ? KSV : a.ksv;
  const int ow = a.crop * 3, owq = ow >> 2;                // bytes / dwords per output (and intermediate) row
  const float inv_owq = 1.0f / (float)owq, inv_rowq = 1.0f / (float)a.row_q, inv_crop = 1.0f / (float)a.crop;
  const int ya = a.y0 + ty * RS_TY, rows_out = min(RS_TY, a.crop - ty * RS_TY);
  const int r0 = a.bv[2 * ya], rend = a.bv[2 * (ya + rows_out - 1)] + a.bv[2 * (ya + rows_out - 1) + 1], R = rend - r0;
  // LDS: [staged input chunk (16-byte aligned)][intermediate rows][tables of both passes]
  uint4 *s_in = (uint4 *)lds;                                                  // [chunk][row_q]
  uint8_t *s_mid = lds + (size_t)a.chunk * a.row_q * 16;                       // [rmax][ow]
  int *s_xb = (int *)(s_mid + (size_t)a.rmax * ow);                            // [crop] byte offset of a window's first tap  (ow % 4 == 0)
  int *s_kh = s_xb + a.crop;                                                   // [crop][ksh]
  int *s_bv = s_kh + a.crop * ksh;                                             // [RS_TY] first intermediate row of a window
  int *s_kv = s_bv + RS_TY;                                                    // [RS_TY][ksv]
  for (int i = tid; i < a.crop; i += RS_THREADS) s_xb[i] = (a.bh[2 * (a.x0 + i)] - a.c0) * 3;
  for (int i = tid; i < a.crop * ksh; i += RS_THREADS) s_kh[i] = a.kh[(size_t)a.x0 * ksh + i];
  for (int i = tid; i < rows_out; i += RS_THREADS) s_bv[i] = a.bv[2 * (ya + i)] - r0;
  for (int i = tid; i < rows_out * ksv; i += RS_THREADS) s_kv[i] = a.kv[(size_t)ya * ksv + i];
  const size_t total = (size_t)a.n * a.h * a.w * 3, whole_q = total >> 4;
  const uint32_t pitch = (uint32_t)a.w * 3u;               // bytes per input row
  for (int rc = 0; rc < R; rc += a.chunk) {
    const int nr = min(a.chunk, R - rc);
    const size_t first0 = (((size_t)im * a.h + r0 + rc) * a.w + a.c0) * 3;                   // byte address of (first row of the chunk, c0, channel 0)
    const uint32_t al0 = (uint32_t)(first0 & 15);
    __syncthreads();                                       // the previous chunk has been consumed (and the tables are in place)
    // stage: 16-byte pieces from the piece that holds byte (row, c0); all of a thread's loads first
    uint4 v[RS_STAGE_LOADS];
#pragma unroll
    for (int u = 0; u < RS_STAGE_LOADS; ++u) {
      const int i = tid + RS_THREADS * u;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (i < nr * a.row_q) {
        const int rr = (int)(((float)i + 0.5f) * inv_rowq), d = i - rr * a.row_q;
        const size_t q = ((first0 + (size_t)((uint32_t)rr * pitch)) >> 4) + d;
        if (q < whole_q) v[u] = ((const uint4 *)a.src)[q];
        else if (q == whole_q) {                            // (never a byte beyond the buffer: its last, partial piece byte by byte)
          uint32_t t[4] = {0u, 0u, 0u, 0u};
          for (size_t b = 16 * whole_q; b < total; ++b) t[(b & 15) >> 2] |= (uint32_t)a.src[b] << (8 * (b & 3));
          v[u] = make_uint4(t[0], t[1], t[2], t[3]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < RS_STAGE_LOADS; ++u) {
      const int i = tid + RS_THREADS * u;
      if (i < nr * a.row_q) s_in[i] = v[u];
    }
    __syncthreads();
    // horizontal pass: one intermediate pixel (three bytes) per thread and step.  Taps beyond a window's own count carry a
    // zero coefficient, and what they read still lies inside the LDS allocation (the staged chunk is followed by s_mid).
    for (int i = tid; i < nr * a.crop; i += RS_THREADS) {
      const int rr = (int)(((float)i + 0.5f) * inv_crop), xc = i - rr * a.crop;
      const uint8_t *p = (const uint8_t *)s_in + (uint32_t)rr * (uint32_t)(a.row_q * 16) + ((al0 + (uint32_t)rr * pitch) & 15u) + s_xb[xc];
      const int *k = s_kh + xc * ksh;
      int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
      // (24-bit multiplies: a byte times a coefficient below 2^23 -- the full-rate v_mad_i32_i24, not the quarter-rate 32-bit one)
      if constexpr (KSH != 0) {
#pragma unroll
        for (int x = 0; x < KSH; ++x) {
          const int kx = k[x];
          a0 += __mul24((int)p[3 * x], kx);
          a1 += __mul24((int)p[3 * x + 1], kx);
          a2 += __mul24((int)p[3 * x + 2], kx);
        }
      } else {
#pragma nounroll
        for (int x = 0; x < ksh; ++x) {
          const int kx = k[x];
          a0 += __mul24((int)p[3 * x], kx);
          a1 += __mul24((int)p[3 * x + 1], kx);
          a2 += __mul24((int)p[3 * x + 2], kx);
        }
      }
      uint8_t *o = s_mid + (size_t)(rc + rr) * ow + 3 * xc;
      o[0] = (uint8_t)clip8(a0);
      o[1] = (uint8_t)clip8(a1);
      o[2] = (uint8_t)clip8(a2);
    }
  }
  __syncthreads();
  // vertical pass: four consecutive output bytes per thread, one dword store
  for (int i = tid; i < rows_out * owq; i += RS_THREADS) {
    const int yc = (int)(((float)i + 0.5f) * inv_owq), q = i - yc * owq;
    const int ymin = s_bv[yc];
    const int *k = s_kv + yc * ksv;
    int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0, s3 = s0;
    auto tap = [&](int y) {
      const uint32_t v = ((const uint32_t *)(s_mid + (size_t)min(ymin + y, R - 1) * ow))[q];
      const int kvy = k[y];
      s0 += __mul24((int)(v & 255u), kvy);
      s1 += __mul24((int)((v >> 8) & 255u), kvy);
      s2 += __mul24((int)((v >> 16) & 255u), kvy);
      s3 += __mul24((int)(v >> 24), kvy);
    };
    if constexpr (KSV != 0) {
#pragma unroll
      for (int y = 0; y < KSV; ++y) tap(y);
    } else {
#pragma nounroll
      for (int y = 0; y < ksv; ++y) tap(y);
    }
    const uint32_t word = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16) | (clip8(s3) << 24);
    ((uint32_t *)(a.dst + ((size_t)im * a.crop + ty * RS_TY + yc) * ow))[q] = word;
  }
}

int round_half_even(double v) { return (int)nearbyint(v); }     // Python's round(), default rounding mode

}  // namespace

}  // namespace ttnet

using namespace ttnet;

// Device copies of the coefficient tables, per geometry and device: built once, kept for the life of the process (a few KB each).
namespace {
struct ResizeGeo {
  int *tab = nullptr;
  size_t nb_h = 0, nk_h = 0, nb_v = 0, nk_v = 0;
  int ksh = 0, ksv = 0, nw = 0, nh = 0, x0 = 0, y0 = 0, c0 = 0, cw = 0, rmax = 0;
};
std::mutex g_geo_mutex;
std::vector<std::pair<std::vector<int>, ResizeGeo>> g_geos;      // key: device, h, w, resize, crop
Coeffs identity(int size) {
  Coeffs c;
  c.ksize = 1;
  c.bounds.resize((size_t)size * 2);
  c.kk.assign((size_t)size, 1 << kPrecisionBits);
  for (int i = 0; i < size; ++i) { c.bounds[2 * i] = i; c.bounds[2 * i + 1] = 1; }
  return c;
}
}  // namespace

extern "C" int ttnet_resize_center_crop_u8(const uint8_t *src_dev, int64_t n, int h, int w, int resize, int crop, uint8_t *dst_dev,
                                           void *stream) {
  if (!src_dev || !dst_dev || n < 1 || h < 1 || w < 1 || resize < 1 || crop < 1 || n > 65535) {
    set_error("resize_center_crop: bad argument");
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)src_dev & 15) || ((uintptr_t)dst_dev & 3) || (crop * 3) % 4) {
    set_error("resize_center_crop: the input must be 16-byte aligned, the output 4-byte aligned and crop * 3 a multiple of 4");
    return TTNET_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  int dev = 0;
  TT_HIP(hipGetDevice(&dev));
  ResizeGeo g;
  {
    std::lock_guard<std::mutex> lock(g_geo_mutex);
    const std::vector<int> key = {dev, h, w, resize, crop};
    bool found = false;
    for (auto &kv : g_geos)
      if (kv.first == key) { g = kv.second; found = true; break; }
    if (!found) {
      // torchvision.transforms.functional.resize with an int size: the shorter side becomes `resize`,
      // the longer one int(resize * long / short); an image whose shorter side already matches is kept
      int nw = w, nh = h;
      if (!((w <= h && w == resize) || (h <= w && h == resize))) {
        if (w <= h) { nw = resize; nh = (int)((double)resize * h / w); }
        else { nh = resize; nw = (int)((double)resize * w / h); }
      }
      if (nw < crop || nh < crop) {
        set_error("resize_center_crop: %dx%d resized to %dx%d is smaller than the %d crop (torchvision would pad)", w, h, nw, nh, crop);
        return TTNET_E_UNSUPPORTED;
      }
      // CenterCrop: int(round((H - crop) / 2.0)); a pass Pillow skips (size unchanged) is the identity table: the same bytes
      g.nw = nw; g.nh = nh;
      g.y0 = round_half_even((nh - crop) / 2.0);
      g.x0 = round_half_even((nw - crop) / 2.0);
      const Coeffs ch = nw != w ? precompute(w, nw) : identity(w), cv = nh != h ? precompute(h, nh) : identity(h);
      g.ksh = ch.ksize; g.ksv = cv.ksize;
      g.c0 = ch.bounds[2 * g.x0];
      g.cw = ch.bounds[2 * (g.x0 + crop - 1)] + ch.bounds[2 * (g.x0 + crop - 1) + 1] - g.c0;
      for (int t0 = 0; t0 < crop; t0 += RS_TY) {
        const int last = g.y0 + std::min(crop, t0 + RS_TY) - 1;
        g.rmax = std::max(g.rmax, cv.bounds[2 * last] + cv.bounds[2 * last + 1] - cv.bounds[2 * (g.y0 + t0)]);
      }
      g.nb_h = ch.bounds.size(); g.nk_h = ch.kk.size(); g.nb_v = cv.bounds.size(); g.nk_v = cv.kk.size();
      std::vector<int> host(g.nb_h + g.nk_h + g.nb_v + g.nk_v);
      std::copy(ch.bounds.begin(), ch.bounds.end(), host.begin());
      std::copy(ch.kk.begin(), ch.kk.end(), host.begin() + g.nb_h);
      std::copy(cv.bounds.begin(), cv.bounds.end(), host.begin() + g.nb_h + g.nk_h);
      std::copy(cv.kk.begin(), cv.kk.end(), host.begin() + g.nb_h + g.nk_h + g.nb_v);
      TT_HIP(hipMalloc((void **)&g.tab, host.size() * sizeof(int)));
      TT_HIP(hipMemcpy(g.tab, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));      // (synchronous: once per geometry)
      g_geos.emplace_back(key, g);
    }
  }
  ResizeArgs a{};
  a.src = src_dev; a.dst = dst_dev;
  a.bh = g.tab; a.kh = g.tab + g.nb_h; a.bv = g.tab + g.nb_h + g.nk_h; a.kv = g.tab + g.nb_h + g.nk_h + g.nb_v;
  a.n = (int)n; a.h = h; a.w = w; a.crop = crop; a.x0 = g.x0; a.y0 = g.y0; a.ksh = g.ksh; a.ksv = g.ksv;
  a.c0 = g.c0; a.cw = g.cw; a.rmax = g.rmax;
  a.row_q = (g.cw * 3 + 15 + 15) / 16;                    // cw * 3 bytes starting up to 15 bytes into the first piece
  a.chunk = std::min(RS_CHUNK, (RS_STAGE_LOADS * RS_THREADS) / a.row_q);
  const size_t lds = (size_t)a.chunk * a.row_q * 16 + (size_t)g.rmax * crop * 3 +
                     (size_t)(crop + crop * g.ksh + RS_TY + RS_TY * g.ksv) * sizeof(int);
  if (lds > 160 * 1024 || a.chunk < 1) {
    set_error("resize_center_crop: %dx%d -> crop %d needs %zu bytes of LDS per workgroup", w, h, crop, lds);
    return TTNET_E_UNSUPPORTED;
  }
  auto launch = [&](auto kernel) -> int {
    TT_TRY(ensure_dynamic_lds((const void *)kernel, lds));
    hipLaunchKernelGGL(kernel, dim3((crop + RS_TY - 1) / RS_TY, (unsigned)n), dim3(RS_THREADS), lds, s, a);
    return TTNET_OK;
  };
  // the common pairs of tap counts get unrolled loops (the aspect is kept, so both passes have the same scale and count)
  if (g.ksh == 1 && g.ksv == 1) TT_TRY(launch(resize_crop_kernel<1, 1>));
  else if (g.ksh == 3 && g.ksv == 3) TT_TRY(launch(resize_crop_kernel<3, 3>));
  else if (g.ksh == 5 && g.ksv == 5) TT_TRY(launch(resize_crop_kernel<5, 5>));
  else if (g.ksh == 7 && g.ksv == 7) TT_TRY(launch(resize_crop_kernel<7, 7>));
  else if (g.ksh == 9 && g.ksv == 9) TT_TRY(launch(resize_crop_kernel<9, 9>));
  else TT_TRY(launch(resize_crop_kernel<0, 0>));
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Ragged batches (ttnet_resize_center_crop_u8_ragged): images of any mix of sizes in one buffer, one launch, nothing on
// the host per call.  A workgroup makes up to RG_TY output rows of one image, as resize_crop_kernel does, but
//   - it reads its image's descriptor and computes the geometry and the coefficient tables it needs itself, in float64
//     and in the order precompute() computes them (the library builds with -ffp-contract=off and double division is
//     correctly rounded, so the tables are the same integers);
//   - its LDS does not grow with the scale factor beyond the tables: after the horizontal pass of a staged chunk, the
//     chunk's intermediate rows are folded into the vertical sums at once (int32, in registers, four output bytes per
//     item), so only one chunk of intermediate rows is ever kept.  Integer sums do not depend on their order: the
//     result is the byte of the two-pass form.
// The next chunk's global loads are issued before the fold of the current one.
// Views (ttnet_resize_views_u8_ragged) are the same kernel handed another geometry: a box of the image instead of the whole
// image, any resized size and crop window instead of torchvision's, the window's columns optionally reversed.
namespace ttnet {
namespace {

constexpr int RG_TY = 16, RG_THREADS = 256, RG_ITEMS = 16, RG_CHUNK = 16, RG_STAGE_LOADS = 6,
              RG_STAGE_Q = RG_STAGE_LOADS * RG_THREADS;        // items: (output row, dword column) sums per thread

struct RaggedArgs {
  const uint8_t *src;
  int64_t src_bytes;
  const ttnet_image_desc *desc;
  uint8_t *dst;
  int32_t *bad;
  int max_h, max_w, resize, crop;
  int ty;          // output rows per workgroup: RG_ITEMS / ceil(crop * 3 / 4 / RG_THREADS)
  int kmax;        // most taps per window any image within max_h x max_w can need (stride room of the tables)
  int stage_q;     // 16-byte pieces of the staged-input area
  // ttnet_resize_views_u8_ragged only: one workgroup column per view instead of per image
  const ttnet_view_desc *views;
  int n_images;
  double max_scale;
};

// torchvision.transforms.functional.resize with an int size: the shorter side becomes `resize`, the longer one
// int(resize * long / short); an image whose shorter side already matches is kept.  The one statement of that rule on
// the device: the ragged kernel and the view generator both call it.
__device__ inline void resized_size(int h, int w, int resize, int &nh, int &nw) {
  nw = w, nh = h;
  if ((w <= h && w == resize) || (h <= w && h == resize)) return;
  if (w <= h) { nw = resize; nh = (int)((double)resize * h / w); }
  else { nh = resize; nw = (int)((double)resize * w / h); }
}
// CenterCrop's offset, int(round(margin / 2.0)) with Python's round()
__device__ inline int center_offset(int margin) { return (int)nearbyint(margin / 2.0); }

__device__ inline bool image_ok(const ttnet_image_desc &d, int max_h, int max_w, int64_t src_bytes) {
  return d.h >= 1 && d.h <= max_h && d.w >= 1 && d.w <= max_w && d.offset >= 0 && d.offset <= src_bytes &&
         (int64_t)d.h * d.w * 3 <= src_bytes - d.offset;
}

// What a workgroup column resizes: the box [by, by + bh) x [bx, bx + bw) of an image of row pitch w at byte `offset`,
// resampled to nw x nh, of which the crop x crop window at (x0, y0) is kept, its columns reversed when `flip`.
struct Geo {
  int64_t offset;
  int w, bx, by, bw, bh, nw, nh, x0, y0;
  bool flip, ok;
};

// Resize(resize) + CenterCrop(crop) of image im: the whole image is the box
__device__ inline Geo center_geo(const RaggedArgs &a, int im) {
  const ttnet_image_desc d = a.desc[im];
  Geo g;
  g.ok = image_ok(d, a.max_h, a.max_w, a.src_bytes);
  g.offset = d.offset;
  g.w = d.w; g.bx = 0; g.by = 0; g.bw = d.w; g.bh = d.h; g.nw = d.w; g.nh = d.h;
  if (g.ok) resized_size(d.h, d.w, a.resize, g.nh, g.nw);
  g.x0 = center_offset(g.nw - a.crop);
  g.y0 = center_offset(g.nh - a.crop);
  g.flip = false;
  return g;
}

constexpr int kMaxSide = 65536;      // of an image a view names, and of the size a box is resampled to

// view v as its descriptor states it (ttnet.h: when a view is valid)
__device__ inline Geo view_geo(const RaggedArgs &a, int v) {
  const int4 *p = (const int4 *)(a.views + v);
  const int4 q0 = p[0], q1 = p[1], q2 = p[2];      // {image, flags, bx, by} {bw, bh, nw, nh} {x0, y0, 0, 0}
  Geo g;
  g.bx = q0.z; g.by = q0.w; g.bw = q1.x; g.bh = q1.y; g.nw = q1.z; g.nh = q1.w; g.x0 = q2.x; g.y0 = q2.y;
  g.flip = (q0.y & 1) != 0;
  g.ok = q0.x >= 0 && q0.x < a.n_images && (q0.y & ~1) == 0 && q2.z == 0 && q2.w == 0;
  ttnet_image_desc d;
  d.offset = 0; d.h = 0; d.w = 0;
  if (g.ok) d = a.desc[q0.x];
  g.offset = d.offset;
  g.w = d.w;
  g.ok = g.ok && image_ok(d, kMaxSide, kMaxSide, a.src_bytes) &&
         g.bx >= 0 && g.bw >= 1 && g.bw <= d.w && g.bx <= d.w - g.bw && g.by >= 0 && g.bh >= 1 && g.bh <= d.h && g.by <= d.h - g.bh &&
         g.nw >= 1 && g.nw <= kMaxSide && g.nh >= 1 && g.nh <= kMaxSide &&
         g.x0 >= 0 && g.x0 <= g.nw - a.crop && g.y0 >= 0 && g.y0 <= g.nh - a.crop;
  g.ok = g.ok && (double)g.bw / g.nw <= a.max_scale && (double)g.bh / g.nh <= a.max_scale;
  return g;
}

// One axis of Pillow's resampling, as precompute() sets it up; `ident`: a pass Pillow skips (size unchanged).
struct Axis {
  double scale, support, ss;
  int in, ksize;
  bool ident;
};

__device__ inline Axis make_axis(int in, int out) {
  Axis a;
  a.in = in;
  a.ident = in == out;
  a.scale = (double)((float)in - 0.0f) / out;
  const double filterscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = 1.0 * filterscale;
  a.ss = 1.0 / filterscale;
  a.ksize = a.ident ? 1 : (int)ceil(a.support) * 2 + 1;
  return a;
}

// first input index and tap count of output index xx
__device__ inline void axis_window(const Axis &a, int xx, double &center, int &xmin, int &cnt) {
  if (a.ident) { center = 0.0; xmin = xx; cnt = 1; return; }
  center = 0.0 + (xx + 0.5) * a.scale;
  xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > a.in) xmax = a.in;
  cnt = min(xmax - xmin, a.ksize);
}

// k[0 .. ksize): the window's fixed-point coefficients, zeros beyond its count (precompute + normalize_coeffs_8bpc)
__device__ inline void axis_coeffs(const Axis &a, int xx, int *k) {
  if (a.ident) { k[0] = 1 << kPrecisionBits; return; }
  double center;
  int xmin, cnt;
  axis_window(a, xx, center, xmin, cnt);
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) {
    double t = (x + xmin - center + 0.5) * a.ss;
    if (t < 0.0) t = -t;
    ww += t < 1.0 ? 1.0 - t : 0.0;
  }
  for (int x = 0; x < cnt; ++x) {
    double t = (x + xmin - center + 0.5) * a.ss;
    if (t < 0.0) t = -t;
    double w = t < 1.0 ? 1.0 - t : 0.0;
    if (ww != 0.0) w /= ww;
    k[x] = w < 0 ? (int)(-0.5 + w * (1 << kPrecisionBits)) : (int)(0.5 + w * (1 << kPrecisionBits));
  }
  for (int x = cnt; x < a.ksize; ++x) k[x] = 0;
}

// horizontal pass of a staged chunk: one intermediate pixel per thread and step, as in resize_crop_kernel
template <int KSH>
__device__ inline void ragged_hpass(const uint8_t *s_in, uint8_t *s_mid, const int *s_xb, const int *s_kh, int ksh, int nr,
                                    int crop, uint32_t row_bytes, uint32_t al0, uint32_t pitch) {
  const float inv_crop = 1.0f / (float)crop;
  const int ow = crop * 3;
  for (int i = threadIdx.x; i < nr * crop; i += RG_THREADS) {
    const int rr = (int)(((float)i + 0.5f) * inv_crop), xc = i - rr * crop;
    const uint8_t *p = s_in + (uint32_t)rr * row_bytes + ((al0 + (uint32_t)rr * pitch) & 15u) + s_xb[xc];
    const int *k = s_kh + xc * ksh;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    if constexpr (KSH != 0) {
#pragma unroll
      for (int x = 0; x < KSH; ++x) {
        const int kx = k[x];
        a0 += __mul24((int)p[3 * x], kx);
        a1 += __mul24((int)p[3 * x + 1], kx);
        a2 += __mul24((int)p[3 * x + 2], kx);
      }
    } else {
#pragma nounroll
      for (int x = 0; x < ksh; ++x) {
        const int kx = k[x];
        a0 += __mul24((int)p[3 * x], kx);
        a1 += __mul24((int)p[3 * x + 1], kx);
        a2 += __mul24((int)p[3 * x + 2], kx);
      }
    }
    uint8_t *o = s_mid + (size_t)rr * ow + 3 * xc;
    o[0] = (uint8_t)clip8(a0);
    o[1] = (uint8_t)clip8(a1);
    o[2] = (uint8_t)clip8(a2);
  }
}

// WIDE: crop * 3 / 4 > RG_THREADS, several dword columns per thread (fewer rows per tile); otherwise item e is row e, column tid.
// VIEWS: blockIdx.y is a view and the geometry is its descriptor's (ttnet_resize_views_u8_ragged); otherwise it is an image
// and the geometry is torchvision's Resize + CenterCrop.  Everything after the geometry is the same code.
template <bool WIDE, bool VIEWS>
__global__ __launch_bounds__(RG_THREADS) void resize_crop_ragged_kernel(RaggedArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int im = blockIdx.y, tid = threadIdx.x, crop = a.crop, ow = crop * 3, owq = ow >> 2;
  const int y_lo = blockIdx.x * a.ty, rows_out = min(a.ty, crop - y_lo), items = rows_out * owq;
  const int ncol = (owq + RG_THREADS - 1) / RG_THREADS;
  uint32_t *dst = (uint32_t *)(a.dst + ((size_t)im * crop + y_lo) * ow);      // this tile's rows, contiguous
  Geo g;
  if constexpr (VIEWS) g = view_geo(a, im);
  else g = center_geo(a, im);
  bool ok = g.ok;
  const int w = g.w, x0 = g.x0, y0 = g.y0;
  const Axis ax = make_axis(g.bw, g.nw), ay = make_axis(g.bh, g.nh);
  const int ksh = ax.ksize, ksv = ay.ksize;
  double c;
  int c0, cl, nl, r0, rl, rn;
  axis_window(ax, x0, c, c0, nl);
  axis_window(ax, x0 + crop - 1, c, cl, nl);
  const int cw = cl + nl - c0, row_q = (cw * 3 + 15 + 15) / 16;
  axis_window(ay, y0 + y_lo, c, r0, rn);
  axis_window(ay, y0 + y_lo + rows_out - 1, c, rl, rn);
  const int R = rl + rn - r0;
  // (the host sized kmax and stage_q for every image within max_h x max_w; this only keeps LDS safe if that were wrong)
  ok = ok && ksh <= a.kmax && ksv <= a.kmax && row_q <= a.stage_q;
  if (!ok) {
    for (int i = tid; i < items; i += RG_THREADS) dst[i] = 0u;
    if (blockIdx.x == 0 && tid == 0 && a.bad) atomicAdd(a.bad, 1);
    return;
  }
  const int chunk = min(RG_CHUNK, a.stage_q / row_q);
  // LDS: [staged input][one chunk of intermediate rows][pad: taps past a row's end][tables]
  uint8_t *s_in = lds;
  uint8_t *s_mid = lds + (size_t)a.stage_q * 16;                                        // [RG_CHUNK][ow]
  int *s_xb = (int *)(s_mid + (size_t)RG_CHUNK * ow + ((3 * a.kmax + 31) & ~15));       // [crop]
  int *s_kh = s_xb + crop;                                                              // [crop][ksh]
  int *s_bv = s_kh + (size_t)crop * a.kmax;                                             // [RG_TY][2]: first row (tile-relative), count
  int *s_kv = s_bv + 2 * RG_TY;                                                         // [RG_TY][ksv]
  for (int xc = tid; xc < crop; xc += RG_THREADS) {
    const int xo = x0 + (g.flip ? crop - 1 - xc : xc);      // the flip acts on the window: output column xc is resized column xo
    int xmin, cnt;
    axis_window(ax, xo, c, xmin, cnt);
    s_xb[xc] = (xmin - c0) * 3;
    axis_coeffs(ax, xo, s_kh + xc * ksh);
  }
  const int yc_t = RG_THREADS - 1 - tid;                   // the vertical rows on the last threads (idle above at crop 224)
  if (yc_t < rows_out) {
    int ymin, cnt;
    axis_window(ay, y0 + y_lo + yc_t, c, ymin, cnt);
    s_bv[2 * yc_t] = ymin - r0;
    s_bv[2 * yc_t + 1] = cnt;
    axis_coeffs(ay, y0 + y_lo + yc_t, s_kv + yc_t * ksv);
  }
  const size_t whole_q = (size_t)a.src_bytes >> 4;
  const uint32_t pitch = (uint32_t)w * 3u, row_bytes = (uint32_t)row_q * 16u;
  const float inv_rowq = 1.0f / (float)row_q;
  auto first_byte = [&](int rc) { return (size_t)g.offset + ((size_t)(g.by + r0 + rc) * w + g.bx + c0) * 3; };
  uint4 v[RG_STAGE_LOADS];
  // stage: the 16-byte pieces of the buffer from the one that holds byte (row, c0), never past src_bytes
  auto load = [&](int rc) {
    const int nr = min(chunk, R - rc);
    const size_t first0 = first_byte(rc);
#pragma unroll
    for (int u = 0; u < RG_STAGE_LOADS; ++u) {
      const int i = tid + RG_THREADS * u;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      if (i < nr * row_q) {
        const int rr = (int)(((float)i + 0.5f) * inv_rowq), dq = i - rr * row_q;
        const size_t q = ((first0 + (size_t)rr * pitch) >> 4) + dq;
        if (q < whole_q) v[u] = ((const uint4 *)a.src)[q];
        else if (q == whole_q) {                            // the last, partial piece byte by byte
          uint32_t t[4] = {0u, 0u, 0u, 0u};
          for (size_t b = 16 * whole_q; b < (size_t)a.src_bytes; ++b) t[(b & 15) >> 2] |= (uint32_t)a.src[b] << (8 * (b & 3));
          v[u] = make_uint4(t[0], t[1], t[2], t[3]);
        }
      }
    }
  };
  // the vertical sums: a thread owns dword column q = tid + RG_THREADS * c of output rows yc; item e = c * ty + yc
  int acc[RG_ITEMS][4];
#pragma unroll
  for (int e = 0; e < RG_ITEMS; ++e) acc[e][0] = acc[e][1] = acc[e][2] = acc[e][3] = 1 << (kPrecisionBits - 1);
  load(0);
  for (int rc = 0; rc < R; rc += chunk) {
    const int nr = min(chunk, R - rc);
    const uint32_t al0 = (uint32_t)(first_byte(rc) & 15);
    __syncthreads();                                       // the previous chunk has been consumed (and the tables are in place)
#pragma unroll
    for (int u = 0; u < RG_STAGE_LOADS; ++u) {
      const int i = tid + RG_THREADS * u;
      if (i < nr * row_q) ((uint4 *)s_in)[i] = v[u];
    }
    __syncthreads();
    switch (ksh) {
      case 1: ragged_hpass<1>(s_in, s_mid, s_xb, s_kh, ksh, nr, crop, row_bytes, al0, pitch); break;
      case 3: ragged_hpass<3>(s_in, s_mid, s_xb, s_kh, ksh, nr, crop, row_bytes, al0, pitch); break;
      case 5: ragged_hpass<5>(s_in, s_mid, s_xb, s_kh, ksh, nr, crop, row_bytes, al0, pitch); break;
      case 7: ragged_hpass<7>(s_in, s_mid, s_xb, s_kh, ksh, nr, crop, row_bytes, al0, pitch); break;
      case 9: ragged_hpass<9>(s_in, s_mid, s_xb, s_kh, ksh, nr, crop, row_bytes, al0, pitch); break;
      default: ragged_hpass<0>(s_in, s_mid, s_xb, s_kh, ksh, nr, crop, row_bytes, al0, pitch); break;
    }
    __syncthreads();
    if (rc + chunk < R) load(rc + chunk);                  // in flight during the fold
    // fold the chunk's rows [rc, rc + nr) into the sums of the output rows whose windows meet them (row bounds and
    // coefficients are uniform over the workgroup: LDS broadcasts, uniform loops)
#pragma unroll
    for (int e = 0; e < RG_ITEMS; ++e) {
      const int yc = WIDE ? e % a.ty : e, q = WIDE ? tid + RG_THREADS * (e / a.ty) : tid;
      if (e < ncol * a.ty && yc < rows_out) {
        const int ymin = s_bv[2 * yc], lo = max(ymin, rc), hi = min(ymin + s_bv[2 * yc + 1], rc + nr);
        if (q < owq && lo < hi) {
          const int *k = s_kv + yc * ksv - ymin;
          const uint32_t *m = (const uint32_t *)s_mid + q - rc * owq;
#pragma nounroll
          for (int y = lo; y < hi; ++y) {
            const uint32_t wv = m[y * owq];
            const int ky = k[y];
            acc[e][0] += __mul24((int)(wv & 255u), ky);
            acc[e][1] += __mul24((int)((wv >> 8) & 255u), ky);
            acc[e][2] += __mul24((int)((wv >> 16) & 255u), ky);
            acc[e][3] += __mul24((int)(wv >> 24), ky);
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < RG_ITEMS; ++e) {
    const int yc = WIDE ? e % a.ty : e, q = WIDE ? tid + RG_THREADS * (e / a.ty) : tid;
    if (e < ncol * a.ty && yc < rows_out && q < owq)
      dst[yc * owq + q] = clip8(acc[e][0]) | (clip8(acc[e][1]) << 8) | (clip8(acc[e][2]) << 16) | (clip8(acc[e][3]) << 24);
  }
}

}  // namespace
}  // namespace ttnet

// The bound on bw / nw and bh / nh that the CENTER / FLIP / FIVE / TEN views (and the ragged Resize + CenterCrop, whose
// geometry is the CENTER view's) need for images within max_h x max_w.  Scale of an axis (w / nw or h / nh): the shorter
// side s goes to `resize` (scale s / resize), the longer side l to int(resize * l / s) > resize * l / s - 1
// (scale < s / (resize - 1)); s <= min(max_h, max_w).
extern "C" double ttnet_eval_views_max_scale(int max_h, int max_w, int resize) {
  if (max_h < 1 || max_w < 1 || resize < 1) return 1.0;
  return std::max(1.0, (double)std::min(max_h, max_w) / (resize > 1 ? resize - 1.0 : 1.0));
}

namespace {
// Sizes a launch for axis scales up to smax (taps 2 * ceil(max(scale, 1)) + 1; input columns of the crop
// < (crop + 1) * max(scale, 1) + 3) and launches it: `columns` images or views.  The one place both ragged entry points
// get their tap stride, staging area and LDS from.
template <bool VIEWS>
int launch_ragged(const char *who, RaggedArgs a, double smax, int64_t columns, hipStream_t stream) {
  const int crop = a.crop, ow = crop * 3, owq = ow / 4;
  const int ty = std::min(RG_TY, RG_ITEMS / ((owq + RG_THREADS - 1) / RG_THREADS));
  if (ty < 1 || !(smax <= 1e4)) {
    set_error("%s: crop %d or axis scales up to %g are beyond this kernel", who, crop, smax);
    return TTNET_E_UNSUPPORTED;
  }
  a.ty = ty;
  a.kmax = 2 * (int)ceil(smax) + 3;                                  // (+2: slack over the rounding of the bound)
  const int64_t cw_max = (int64_t)ceil((crop + 1) * smax) + 4, row_q_max = (cw_max * 3 + 30) / 16;
  if (row_q_max > RG_STAGE_Q) {
    set_error("%s: axis scales up to %g at crop %d need %lld input bytes per row, more than the %d a workgroup stages", who,
              smax, crop, (long long)(cw_max * 3), RG_STAGE_Q * 16);
    return TTNET_E_UNSUPPORTED;
  }
  a.stage_q = (int)std::min<int64_t>((int64_t)RG_CHUNK * row_q_max, RG_STAGE_Q);
  const size_t lds = (size_t)a.stage_q * 16 + (size_t)RG_CHUNK * ow + ((3 * a.kmax + 31) & ~15) +
                     ((size_t)crop + (size_t)crop * a.kmax + 2 * RG_TY + (size_t)RG_TY * a.kmax) * sizeof(int);
  if (lds > 160 * 1024) {
    set_error("%s: axis scales up to %g at crop %d need %zu bytes of LDS per workgroup", who, smax, crop, lds);
    return TTNET_E_UNSUPPORTED;
  }
  auto launch = [&](auto kernel) -> int {
    TT_TRY(ensure_dynamic_lds((const void *)kernel, lds));
    hipLaunchKernelGGL(kernel, dim3((crop + ty - 1) / ty, (unsigned)columns), dim3(RG_THREADS), lds, stream, a);
    return TTNET_OK;
  };
  if (owq <= RG_THREADS) TT_TRY(launch(resize_crop_ragged_kernel<false, VIEWS>));
  else TT_TRY(launch(resize_crop_ragged_kernel<true, VIEWS>));
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}
}  // namespace

extern "C" int ttnet_resize_center_crop_u8_ragged(const uint8_t *src_dev, int64_t src_bytes, const ttnet_image_desc *desc_dev,
                                                  int64_t n, int max_h, int max_w, int resize, int crop, uint8_t *dst_dev,
                                                  int32_t *bad_dev, void *stream) {
  if (!src_dev || !desc_dev || !dst_dev || src_bytes < 1 || n < 1 || n > 65535 || max_h < 1 || max_w < 1 || crop < 1 ||
      resize < crop) {
    set_error("resize_center_crop_ragged: bad argument (n %lld, src_bytes %lld, max %dx%d, resize %d, crop %d; "
              "resize must be >= crop)", (long long)n, (long long)src_bytes, max_w, max_h, resize, crop);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)src_dev & 15) || ((uintptr_t)desc_dev & 7) || ((uintptr_t)dst_dev & 3) || (crop * 3) % 4) {
    set_error("resize_center_crop_ragged: the input must be 16-byte aligned, the descriptors 8-byte aligned, the output "
              "4-byte aligned and crop * 3 a multiple of 4");
    return TTNET_E_INVALID;
  }
  if (max_h > 65536 || max_w > 65536 || resize > 65536) {
    set_error("resize_center_crop_ragged: images up to %dx%d at resize %d are beyond this kernel", max_w, max_h, resize);
    return TTNET_E_UNSUPPORTED;
  }
  RaggedArgs a{};
  a.src = src_dev; a.src_bytes = src_bytes; a.desc = desc_dev; a.dst = dst_dev; a.bad = bad_dev;
  a.max_h = max_h; a.max_w = max_w; a.resize = resize; a.crop = crop;
  return launch_ragged<false>("resize_center_crop_ragged", a, ttnet_eval_views_max_scale(max_h, max_w, resize), n,
                              (hipStream_t)stream);
}

static_assert(sizeof(ttnet_view_desc) == 48, "a view descriptor is 48 bytes (ttnet.h)");

extern "C" int ttnet_resize_views_u8_ragged(const uint8_t *src_dev, int64_t src_bytes, const ttnet_image_desc *image_desc_dev,
                                            int64_t n_images, const ttnet_view_desc *view_desc_dev, int64_t n_views,
                                            double max_scale, int crop, uint8_t *dst_dev, int32_t *bad_dev, void *stream) {
  if (!src_dev || !image_desc_dev || !view_desc_dev || !dst_dev || src_bytes < 1 || n_images < 1 || n_images > 65535 ||
      n_views < 1 || n_views > 65535 || crop < 1 || crop > kMaxSide || !(max_scale >= 1.0)) {
    set_error("resize_views_ragged: bad argument (n_images %lld, n_views %lld in [1, 65535], src_bytes %lld, crop %d, "
              "max_scale %g >= 1)", (long long)n_images, (long long)n_views, (long long)src_bytes, crop, max_scale);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)src_dev & 15) || ((uintptr_t)image_desc_dev & 7) || ((uintptr_t)view_desc_dev & 15) || ((uintptr_t)dst_dev & 3) ||
      (crop * 3) % 4) {
    set_error("resize_views_ragged: the input and the view descriptors must be 16-byte aligned, the image descriptors 8-byte "
              "aligned, the output 4-byte aligned and crop * 3 a multiple of 4");
    return TTNET_E_INVALID;
  }
  RaggedArgs a{};
  a.src = src_dev; a.src_bytes = src_bytes; a.desc = image_desc_dev; a.dst = dst_dev; a.bad = bad_dev; a.crop = crop;
  a.views = view_desc_dev; a.n_images = (int)n_images; a.max_scale = max_scale;
  return launch_ragged<true>("resize_views_ragged", a, max_scale, n_views, (hipStream_t)stream);
}

// ttnet_make_eval_views: one thread per image writes its V view descriptors, image-major.
namespace {
constexpr int kFamilyViews[4] = {1, 2, 5, 10};      // TTNET_VIEWS_CENTER, _FLIP, _FIVE, _TEN

__global__ __launch_bounds__(256) void make_eval_views_kernel(const ttnet_image_desc *desc, int n, int resize, int crop, int family,
                                                              int V, ttnet_view_desc *out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ttnet_image_desc d = desc[i];
  // (an image that was not decoded, h = w = 0, or any other size the resize refuses: its views are refused too, by their box)
  const bool ok = d.h >= 1 && d.w >= 1;
  int nh = 0, nw = 0;
  if (ok) resized_size(d.h, d.w, resize, nh, nw);
  const int mx = nw - crop, my = nh - crop, cx = center_offset(mx), cy = center_offset(my);
  // the windows in torchvision's order: five_crop is (tl, tr, bl, br, center); ten_crop adds five_crop of the flipped image,
  // whose windows read mirrored: tl <-> tr, bl <-> br, and the centre crop at mx - cx
  auto window = [&](int v, int &x, int &y, int &flip) {
    flip = 0;
    if (family == TTNET_VIEWS_CENTER || (family == TTNET_VIEWS_FLIP && v == 0)) { x = cx; y = cy; return; }
    if (family == TTNET_VIEWS_FLIP) { x = mx - cx; y = cy; flip = 1; return; }
    const int u = v % 5;
    flip = v >= 5;
    if (u == 4) { x = flip ? mx - cx : cx; y = cy; return; }
    const bool right = ((u & 1) != 0) != (flip != 0);
    x = right ? mx : 0;
    y = (u & 2) ? my : 0;
  };
  for (int v = 0; v < V; ++v) {
    int x = 0, y = 0, flip = 0;
    window(v, x, y, flip);
    int4 *p = (int4 *)(out + (size_t)i * V + v);
    p[0] = ok ? make_int4(i, flip, 0, 0) : make_int4(i, 0, 0, 0);
    p[1] = ok ? make_int4(d.w, d.h, nw, nh) : make_int4(0, 0, 0, 0);
    p[2] = ok ? make_int4(x, y, 0, 0) : make_int4(0, 0, 0, 0);
  }
}
}  // namespace

extern "C" int ttnet_make_eval_views(const ttnet_image_desc *image_desc_dev, int64_t n_images, int resize, int crop, int family,
                                     ttnet_view_desc *view_desc_dev, void *stream) {
  if (!image_desc_dev || !view_desc_dev || n_images < 1 || crop < 1 || resize < crop || resize > kMaxSide ||
      family < TTNET_VIEWS_CENTER || family > TTNET_VIEWS_TEN || n_images * kFamilyViews[family] > 65535) {
    set_error("make_eval_views: bad argument (n_images %lld, resize %d >= crop %d, family %d in [0, 3], n_images * views <= 65535)",
              (long long)n_images, resize, crop, family);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)image_desc_dev & 7) || ((uintptr_t)view_desc_dev & 15)) {
    set_error("make_eval_views: the image descriptors must be 8-byte aligned, the view descriptors 16-byte aligned");
    return TTNET_E_INVALID;
  }
  hipLaunchKernelGGL(make_eval_views_kernel, dim3((unsigned)((n_images + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     image_desc_dev, (int)n_images, resize, crop, family, kFamilyViews[family], view_desc_dev);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}
