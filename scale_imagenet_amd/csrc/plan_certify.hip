// libttnet.so -- the plan's certificate and attack entries (vAlexnet): ttnet_certify_u8, ttnet_certify_box_u8,
// ttnet_certify_patch_u8, ttnet_attack_patch_u8, ttnet_patch_paste_u8, ttnet_attack_propose_u8, ttnet_attack_select_u8 of
// include/ttnet.h.
//
// Host code only: argument checks, the state derived once per loaded checkpoint (prepare_certify) and the argument blocks
// of the kernels in certify.hip and attack.hip.

#include <math.h>

#include <utility>

#include "plan.h"

using namespace ttnet;

// what ttnet_certify_u8 derived from the state goes with the state (the lanes' planes hold no state and stay)
void ttnet::drop_certify(ttnet_plan *pl) {
  auto &c = pl->cert;
  for (void *ptr : {(void *)c.A, (void *)c.c0, (void *)c.stem_bn, (void *)c.slack, (void *)c.t3w, (void *)c.wsum}) dev_free(pl, ptr);
  c = ttnet_plan::Certify{};
}

namespace {

// ttnet_certify_u8: the effective head, the stem's BatchNorm in float64, the slack of the stem bounds and Block_conv3's
// table as words, from the state the plan was finalized with.  Host synchronisations and allocations: first call only.
int prepare_certify(ttnet_plan *pl, hipStream_t s) {
  auto &c = pl->cert;
  if (c.ready) return TTNET_OK;
  drop_certify(pl);
  std::vector<float> w, b;
  std::vector<double> sc, sh, hs, ht;
  TT_TRY(fetch(pl->tensors["features.0.weight"], w));
  TT_TRY(fetch(pl->tensors["features.0.bias"], b));
  TT_TRY(fold_bn(pl, "features.2", sc, sh));
  TT_TRY(fold_bn(pl, pl->head + ".BN2", hs, ht));
  // slack_c = 2^-40 ((|w_c|_1 X + |bias_c|) |scale_c| + |shift_c|), X = the largest |normalised value| of a byte (ttnet.h)
  double X = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    const double a = 1.0 / (255.0 * (double)pl->in_std[ch]), off = 255.0 * (double)pl->in_mean[ch];
    X = std::max(X, std::max(fabs((0.0 - off) * a), fabs((255.0 - off) * a)));
  }
  std::vector<double> slack(64), bn(sc), hbn(hs);
  bn.insert(bn.end(), sh.begin(), sh.end());
  hbn.insert(hbn.end(), ht.begin(), ht.end());
  for (int ch = 0; ch < 64; ++ch) {
    double l1 = 0.0;
    for (int i = 0; i < 27; ++i) l1 += fabs((double)w[ch * 27 + i]);
    slack[ch] = ldexp((l1 * X + fabs((double)b[ch])) * fabs(sc[ch]) + fabs(sh[ch]), -40);
  }
  double *hbn_dev = nullptr;                           // the head's folded BatchNorm: needed by the build alone
  auto build = [&]() -> int {
    TT_TRY(dev_alloc(pl, &c.A, (size_t)pl->n_classes * pl->fcsize, false));
    TT_TRY(dev_alloc(pl, &c.c0, pl->n_classes, false));
    TT_TRY(dev_alloc(pl, &c.stem_bn, 128, false));
    TT_TRY(dev_alloc(pl, &c.slack, 64, false));
    TT_TRY(dev_alloc(pl, &c.t3w, 8 * 8 * 4, false));
    TT_TRY(dev_alloc(pl, &c.wsum, va::kWsum, false));
    TT_TRY(dev_alloc(pl, &hbn_dev, hbn.size(), false));
    TT_HIP(hipMemcpy(c.stem_bn, bn.data(), bn.size() * 8, hipMemcpyHostToDevice));
    TT_HIP(hipMemcpy(c.slack, slack.data(), slack.size() * 8, hipMemcpyHostToDevice));
    TT_HIP(hipMemcpy(hbn_dev, hbn.data(), hbn.size() * 8, hipMemcpyHostToDevice));
    TT_TRY(launch_certify_head((const float *)pl->tensors[pl->head + ".lin1.weight"].dev, (const float *)pl->tensors[pl->head + ".lin2.weight"].dev,
                               (const float *)pl->tensors[pl->head + ".lin2.bias"].dev, hbn_dev, (const uint8_t *)pl->blocks[0].c3.table, c.A,
                               c.c0, c.t3w, s));
    TT_TRY(launch_attack_wsum((const float *)pl->tensors["features.0.weight"].dev, c.wsum, s));
    TT_HIP(hipStreamSynchronize(s));
    return TTNET_OK;
  };
  const int st = build();
  dev_free(pl, hbn_dev);                               // on every exit
  if (st != TTNET_OK) {
    drop_certify(pl);                                  // nothing half built stays
    return st;
  }
  c.ready = true;
  return TTNET_OK;
}

// Where the block's tables and the state of prepare_certify stand: what the argument blocks of the certificate and of
// the search point at
struct VaState {
  const float *w, *bias;         // the stem's convolution
  const double *stem_bn, *slack, *A, *c0, *wsum;
  const uint32_t *t1, *t2;
  const uint8_t *t3;
  const uint64_t *t3w;
};
VaState va_state(ttnet_plan *pl) {
  const MultiHead &mh = pl->blocks[0];
  const ttnet_plan::Certify &c = pl->cert;
  return {(const float *)pl->tensors["features.0.weight"].dev, (const float *)pl->tensors["features.0.bias"].dev, c.stem_bn, c.slack, c.A, c.c0,
          c.wsum, (const uint32_t *)mh.c1.table, (const uint32_t *)mh.c2.table, (const uint8_t *)mh.c3.table, c.t3w};
}

// The arguments the three certificate entries share; second_out: the planes (eps and box) or the map (patch)
struct CertifyCall {
  const char *who;
  int lane;
  const uint8_t *x, *x_hi;
  int64_t n;
  const int32_t *classes;
  double eps;
  int enum_bits;
  double min_margin;
  void *rows;
  const void *second_out;
};

// An entry runs certify_ready, its own null checks, its own argument checks, certify_check and certify_fill, and a fault is
// reported in that order.

// the variant and the plan's state
int certify_ready(ttnet_plan *pl, const CertifyCall &c) {
  if (pl && pl->path != GatePath::VAlexnet)
    return refused(TTNET_E_UNSUPPORTED, "certify: only the vAlexnet variant is served: the certificate needs an affine head (no polynomial, no float last "
                   "block) and truth tables of at most 8 inputs");
  return check_ready(pl, c.x, c.n, c.rows, c.who);
}

// the arguments every entry takes, then the lane
int certify_check(ttnet_plan *pl, const CertifyCall &c, ttnet_plan::Lane **lane) {
  if (!(c.eps >= 0.0) || !std::isfinite(c.eps)) return refused(TTNET_E_INVALID, "certify: eps = %g (finite, >= 0)", c.eps);
  if (c.enum_bits < 0 || c.enum_bits > 12 || std::isnan(c.min_margin))
    return refused(TTNET_E_INVALID, "certify: enum_bits = %d (0..12), min_margin = %g", c.enum_bits, c.min_margin);
  if (((uintptr_t)c.x & 3u) || ((uintptr_t)c.x_hi & 3u) || ((uintptr_t)c.classes & 3u) || ((uintptr_t)c.rows & 7u) ||
      ((uintptr_t)c.second_out & 7u))
    return refused(TTNET_E_INVALID, "certify: the images and classes must be 4-byte aligned, the records and planes 8-byte aligned");
  return lane_of(pl, "certify", c.lane, lane);
}

// A / c0 / slack, the lane's planes, and the argument block of the stages with the box [x, x_hi] or x +- eps
int certify_fill(ttnet_plan *pl, const CertifyCall &c, ttnet_plan::Lane &L, hipStream_t s, CertifyArgs &a) {
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(prepare_certify(pl, s));
  const size_t nb = (size_t)pl->desc.max_batch, stem_w = va::kStemRows, feat_w = va::kFeatRows;
  if (!L.cert_planes) TT_TRY(dev_alloc(pl, &L.cert_planes, nb * (2 * (stem_w + feat_w) + va::kClasses), false));
  a = CertifyArgs{};
  a.n = (int)c.n;
  a.x = c.x;
  a.x_hi = c.x_hi;
  a.classes = c.classes;
  for (int ch = 0; ch < 3; ++ch) {
    a.norm.a[ch] = 1.0 / (255.0 * (double)pl->in_std[ch]);
    a.norm.off[ch] = 255.0 * (double)pl->in_mean[ch];
  }
  a.eps = c.eps;
  a.min_margin = c.min_margin;
  a.enum_bits = c.enum_bits;
  const VaState v = va_state(pl);
  a.w = v.w; a.bias = v.bias; a.stem_bn = v.stem_bn; a.slack = v.slack;
  a.t1 = v.t1; a.t2 = v.t2; a.t3 = v.t3; a.t3w = v.t3w;
  a.A = v.A; a.c0 = v.c0;
  a.stem_lo = L.cert_planes;
  a.stem_hi = a.stem_lo + nb * stem_w;
  a.feat_lo = a.stem_hi + nb * stem_w;
  a.feat_hi = a.feat_lo + nb * feat_w;
  a.sums = (double *)(a.feat_hi + nb * feat_w);
  a.rows = c.rows;
  return TTNET_OK;
}

// the four stages on `s`, then the planes [stem lo][stem hi][feature lo][feature hi], each for n images
int certify_run(ttnet_plan *pl, const CertifyArgs &a, uint64_t *planes_dev, hipStream_t s) {
  pl->timing_used = 0;                                // (with profiling on, ttnet_plan_last_timings then speaks of this call)
  TT_TIMED(pl, "certify.stem", s, launch_certify(a, kCertifyStem, s));
  TT_TIMED(pl, "certify.block", s, launch_certify(a, kCertifyBlock, s));
  TT_TIMED(pl, "certify.margin", s, launch_certify(a, kCertifyMargin, s));
  if (a.enum_bits > 0) TT_TIMED(pl, "certify.enum", s, launch_certify(a, kCertifyEnum, s));
  if (planes_dev) {
    uint64_t *dst = planes_dev;
    const size_t stem_w = va::kStemRows, feat_w = va::kFeatRows;
    for (const auto &pw : {std::pair<const uint64_t *, size_t>{a.stem_lo, stem_w}, {a.stem_hi, stem_w}, {a.feat_lo, feat_w}, {a.feat_hi, feat_w}}) {
      TT_HIP(hipMemcpyAsync(dst, pw.first, (size_t)a.n * pw.second * 8, hipMemcpyDeviceToDevice, s));
      dst += (size_t)a.n * pw.second;
    }
  }
  return TTNET_OK;
}

// the ranges the patch entries share, under the entry's name
int patch_ranges(const char *who, int patch_h, int patch_w, int stride, int amp) {
  if (patch_h < 1 || patch_h > va::kPatchMax || patch_w < 1 || patch_w > va::kPatchMax || stride < 1 || stride > 32 || amp < 1 || amp > 255)
    return refused(TTNET_E_INVALID, "%s: patch %d x %d (1..8 each), stride %d (1..32), amp %d (1..255)", who, patch_h, patch_w, stride, amp);
  return TTNET_OK;
}

// the argument block of the patch sweep and of the patch search up to their outputs: the clean pass and the geometry
int patch_fill(ttnet_plan *pl, const CertifyCall &c, ttnet_plan::Lane &L, int patch_h, int patch_w, int stride, int amp, hipStream_t s, PatchArgs &p) {
  TT_TRY(certify_fill(pl, c, L, s, p.clean));
  // per image of max_batch: the clean pass's record (4 doubles) and the unknown part of its sums (10)
  if (!L.patch_base) TT_TRY(dev_alloc(pl, &L.patch_base, (size_t)pl->desc.max_batch * (4 + va::kClasses), false));
  p.clean.rows = L.patch_base;
  p.clean.sums_un = L.patch_base + (size_t)pl->desc.max_batch * 4;
  p.patch_h = patch_h;
  p.patch_w = patch_w;
  p.stride = stride;
  p.amp = amp;
  p.py = part::patch_positions(patch_h, stride);
  p.px = part::patch_positions(patch_w, stride);
  return TTNET_OK;
}

// what the two attack entries share: the variant, the plan's state and the batch size
int attack_ready(ttnet_plan *pl, const void *a, int64_t n, const void *b, const char *who) {
  if (pl && pl->path != GatePath::VAlexnet)
    return refused(TTNET_E_UNSUPPORTED, "%s: only the vAlexnet variant is served: the search needs the certificate's stem planes, an affine head and truth "
                   "tables of at most 8 inputs", who);
  return check_ready(pl, a, n, b, who);
}

}  // namespace

extern "C" {

int ttnet_certify_u8(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, double eps,
                     int enum_bits, double min_margin, void *rows_dev, uint64_t *planes_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const CertifyCall c{"ttnet_certify_u8", lane, x_nhwc_dev, nullptr, n, classes_dev, eps, enum_bits, min_margin, rows_dev, planes_dev};
  TT_TRY(certify_ready(pl, c));
  if (!classes_dev) return refused(TTNET_E_INVALID, "null argument");
  ttnet_plan::Lane *L = nullptr;
  TT_TRY(certify_check(pl, c, &L));
  CertifyArgs a;
  TT_TRY(certify_fill(pl, c, *L, s, a));
  return certify_run(pl, a, planes_dev, s);
}

int ttnet_certify_box_u8(ttnet_plan *pl, int lane, const uint8_t *lo_nhwc_dev, const uint8_t *hi_nhwc_dev, int64_t n,
                         const int32_t *classes_dev, int enum_bits, double min_margin, void *rows_dev, uint64_t *planes_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const CertifyCall c{"ttnet_certify_box_u8", lane, lo_nhwc_dev, hi_nhwc_dev, n, classes_dev, 0.0, enum_bits, min_margin, rows_dev, planes_dev};
  TT_TRY(certify_ready(pl, c));
  // (a null upper image is refused only when the planes are null too)
  if (!classes_dev || (!hi_nhwc_dev && !planes_dev)) return refused(TTNET_E_INVALID, "null argument");
  ttnet_plan::Lane *L = nullptr;
  TT_TRY(certify_check(pl, c, &L));
  CertifyArgs a;
  TT_TRY(certify_fill(pl, c, *L, s, a));
  return certify_run(pl, a, planes_dev, s);
}

int ttnet_certify_patch_u8(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, int patch_h,
                           int patch_w, int stride, int amp, int enum_bits, double min_margin, void *rows_dev, void *map_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const CertifyCall c{"ttnet_certify_patch_u8", lane, x_nhwc_dev, nullptr, n, classes_dev, 0.0, enum_bits, min_margin, rows_dev, map_dev};
  TT_TRY(certify_ready(pl, c));
  if (!classes_dev || !map_dev) return refused(TTNET_E_INVALID, "null argument");
  TT_TRY(patch_ranges("certify_patch", patch_h, patch_w, stride, amp));
  ttnet_plan::Lane *L = nullptr;
  TT_TRY(certify_check(pl, c, &L));
  PatchArgs p{};
  TT_TRY(patch_fill(pl, c, *L, patch_h, patch_w, stride, amp, s, p));
  p.map = map_dev;
  p.rows = rows_dev;
  pl->timing_used = 0;
  TT_TIMED(pl, "patch.base", s, launch_certify_patch(p, kPatchBase, s));
  TT_TIMED(pl, "patch.sweep", s, launch_certify_patch(p, kPatchSweep, s));
  return TTNET_OK;
}

int ttnet_attack_patch_u8(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, int patch_h, int patch_w,
                          int stride, int amp, int rounds, double min_margin, void *map_dev, uint8_t *fills_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const CertifyCall c{"ttnet_attack_patch_u8", lane, x_nhwc_dev, nullptr, n, classes_dev, 0.0, 0, min_margin, map_dev, nullptr};
  TT_TRY(certify_ready(pl, c));
  if (!classes_dev || !fills_dev) return refused(TTNET_E_INVALID, "null argument");
  TT_TRY(patch_ranges("attack_patch", patch_h, patch_w, stride, amp));
  if (rounds < 1 || rounds > 4) return refused(TTNET_E_INVALID, "attack_patch: rounds = %d (1..4)", rounds);
  if ((uintptr_t)fills_dev & 3u) return refused(TTNET_E_INVALID, "attack_patch: the fills must be 4-byte aligned");
  ttnet_plan::Lane *L = nullptr;
  TT_TRY(certify_check(pl, c, &L));
  AttackPatchArgs a{};
  TT_TRY(patch_fill(pl, c, *L, patch_h, patch_w, stride, amp, s, a.sweep));
  a.rounds = rounds;
  a.min_margin = min_margin;
  a.wsum = va_state(pl).wsum;
  a.map = map_dev;
  a.fills = fills_dev;
  pl->timing_used = 0;
  TT_TIMED(pl, "patch.base", s, launch_certify_patch(a.sweep, kPatchBase, s));
  TT_TIMED(pl, "patch.attack", s, launch_attack_patch(a, s));
  return TTNET_OK;
}

int ttnet_patch_paste_u8(ttnet_plan *pl, const uint8_t *x_nhwc_dev, int64_t n, int patch_h, int patch_w, int stride, const uint8_t *fills_dev,
                         const int64_t *tasks_dev, int64_t m, uint8_t *out_nhwc_dev, void *stream) {
  TT_TRY(attack_ready(pl, x_nhwc_dev, n, out_nhwc_dev, "ttnet_patch_paste_u8"));
  if (!fills_dev || !tasks_dev) return refused(TTNET_E_INVALID, "null argument");
  TT_TRY(patch_ranges("patch_paste", patch_h, patch_w, stride, 1));
  if (m < 1 || m > 0x7FFFFFFFll) return refused(TTNET_E_INVALID, "patch_paste: m = %lld (1..2^31 - 1)", (long long)m);
  if ((((uintptr_t)x_nhwc_dev | (uintptr_t)fills_dev | (uintptr_t)out_nhwc_dev) & 3u) || ((uintptr_t)tasks_dev & 7u))
    return refused(TTNET_E_INVALID, "patch_paste: the images and fills must be 4-byte aligned, the tasks 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  pl->timing_used = 0;
  TT_TIMED(pl, "patch.paste", s, launch_patch_paste(x_nhwc_dev, n, patch_h, patch_w, stride, fills_dev, tasks_dev, m, out_nhwc_dev, s));
  return TTNET_OK;
}

int ttnet_attack_propose_u8(ttnet_plan *pl, int lane, const uint8_t *x0_dev, const uint8_t *xcur_dev, int64_t n,
                            const int32_t *classes_dev, const int32_t *worst_dev, const uint64_t *stem_planes_dev, int eps_levels,
                            const int32_t *active_dev, uint8_t *cand_dev, double *gains_dev, void *stream) {
  TT_TRY(attack_ready(pl, x0_dev, n, cand_dev, "ttnet_attack_propose_u8"));
  if (!xcur_dev || !classes_dev || !worst_dev || !stem_planes_dev || !active_dev) return refused(TTNET_E_INVALID, "null argument");
  if (eps_levels < 0 || eps_levels > 64)
    return refused(TTNET_E_INVALID, "attack_propose: eps_levels = %d (0..64)", eps_levels);
  if ((((uintptr_t)x0_dev | (uintptr_t)xcur_dev | (uintptr_t)classes_dev | (uintptr_t)worst_dev | (uintptr_t)active_dev | (uintptr_t)cand_dev) & 3u) ||
      (((uintptr_t)stem_planes_dev | (uintptr_t)gains_dev) & 7u))
    return refused(TTNET_E_INVALID, "attack_propose: the images, classes, runner-ups, flags and candidates must be 4-byte aligned, the planes and gains "
                                    "8-byte aligned");
  ttnet_plan::Lane *L = nullptr;
  TT_TRY(lane_of(pl, "attack_propose", lane, &L));
  if (L->last_n != n)
    return refused(TTNET_E_STATE, "attack_propose: n=%lld but the last forward on lane %d ran %lld images", (long long)n, lane, (long long)L->last_n);
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(prepare_certify(pl, s));
  AttackProposeArgs a{};
  a.n = (int)n;
  a.levels = eps_levels;
  a.x0 = x0_dev;
  a.xcur = xcur_dev;
  a.classes = classes_dev;
  a.worst = worst_dev;
  a.active = active_dev;
  a.stem = L->x_rp[0];
  a.feat = L->va_y;
  a.plane_lo = stem_planes_dev;
  a.plane_hi = stem_planes_dev + (size_t)n * va::kStemRows;
  const VaState v = va_state(pl);
  a.t1 = v.t1; a.t2 = v.t2; a.t3w = v.t3w;
  a.A = v.A; a.bn_scale = v.stem_bn; a.wsum = v.wsum;
  a.cand = cand_dev;
  a.gains = gains_dev;
  pl->timing_used = 0;                                // (with profiling on, ttnet_plan_last_timings then speaks of this call)
  TT_TIMED(pl, "attack.propose", s, launch_attack_propose(a, s));
  return TTNET_OK;
}

int ttnet_attack_select_u8(ttnet_plan *pl, const uint8_t *cand_dev, const float *logits_dev, int64_t n, int n_cand,
                           const int32_t *classes_dev, double min_margin, const uint8_t *x0_dev, uint8_t *xcur_dev, void *rows_dev,
                           int32_t *worst_dev, int32_t *active_dev, int round, void *stream) {
  TT_TRY(attack_ready(pl, cand_dev, n, logits_dev, "ttnet_attack_select_u8"));
  if (!classes_dev || !x0_dev || !xcur_dev || !rows_dev || !worst_dev || !active_dev) return refused(TTNET_E_INVALID, "null argument");
  if (n_cand < 1 || n_cand > 8 || round < 0 || std::isnan(min_margin))
    return refused(TTNET_E_INVALID, "attack_select: n_cand = %d (1..8), round = %d (>= 0), min_margin = %g", n_cand, round, min_margin);
  if ((((uintptr_t)cand_dev | (uintptr_t)logits_dev | (uintptr_t)classes_dev | (uintptr_t)x0_dev | (uintptr_t)xcur_dev | (uintptr_t)worst_dev |
        (uintptr_t)active_dev) & 3u) || ((uintptr_t)rows_dev & 7u))
    return refused(TTNET_E_INVALID, "attack_select: the images, logits, classes, runner-ups and flags must be 4-byte aligned, the records 8-byte "
                                    "aligned");
  if (xcur_dev == cand_dev || xcur_dev == x0_dev) return refused(TTNET_E_INVALID, "attack_select: xcur_dev must be a buffer of its own");
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  pl->timing_used = 0;
  TT_TIMED(pl, "attack.select", s,
           launch_attack_select(cand_dev, logits_dev, (int)n, n_cand, classes_dev, (float)min_margin, x0_dev, xcur_dev, rows_dev, worst_dev,
                                active_dev, round, s));
  return TTNET_OK;
}

}  // extern "C"
