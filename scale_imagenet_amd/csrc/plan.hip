// libttnet.so -- plan object and the C ABI of include/ttnet.h.
//
// Host-side counterpart of the reference's model object (construction, load_state_dict,
// forward dispatch; models/TT_general_imagenet_v2_small.py:151-207,
// models/model_utils/netbin.py:703-708).  No torch types, no CPU compute path: every
// arithmetic step of forward() is a HIP kernel from stem.hip / gate.hip / head.hip, and the
// derived tables are built by lut_build.hip.  Host code here only folds BatchNorm
// parameters (a few thousand scalars, float64) and moves bytes.  (The RCCL all-gather of the same header: comm.hip.)

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <mutex>
#include <unordered_map>

#include "partition.h"
#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

constexpr double kBnEps = 1e-5;   // nn.BatchNorm2d / BatchNorm1d default

struct Tensor {
  std::vector<int64_t> shape;
  int dtype = TTNET_F32;
  void *dev = nullptr;
  size_t bytes = 0;
  bool set = false;
  bool required = true;
};

struct BlockTT {
  BlockGeom g;
  std::vector<uint8_t> perm;     // internal index bit p -> canonical input column
  uint8_t *perm_dev = nullptr;
  double *s1 = nullptr, *t1 = nullptr, *s2 = nullptr, *t2 = nullptr;
  void *table = nullptr;         // internal layout
  unsigned *near_dev = nullptr;
  int64_t near_ties = -1;
  bool user_table = false;
  int64_t *usage = nullptr;      // [groups][2^n] lookups per entry, canonical order (ttnet_plan_table_usage_enable)
  uint32_t *care = nullptr;      // [groups][max(1, 2^n / 32)] care bitmap, canonical order (ttnet_plan_set_care); null: none
};

struct MultiHead {
  std::string name;
  int C = 0, H = 0, W = 0, Ho = 0, Wo = 0, off34 = 0, stride = 2;
  bool last = false;
  BlockTT c1, c2, c3, cf;
  void *img_dw = nullptr, *img_c3 = nullptr;   // block-fused path (gate_fused.hip): table images
};

// How the blocks are evaluated, fixed when the geometry is built
enum class GatePath {
  TwoLaunch,   // TT-small: stage 1 + convf kernels of gate.hip, activations as rows and channel words
  Fused,       // TT-small with stride-2 blocks only: one launch per block (gate_fused.hip), activations as
               // compact rows; TTNET_GATE_UNFUSED=1 keeps TwoLaunch
  XSmall,      // x-small variant: row-packed branch tensors, gate_xs.hip kernels
  Full,        // full variant (fan-in 30): direct float64 evaluation, gate_full.hip
  VAlexnet,    // CIFAR vAlexnet variant, gate_va.hip
};

struct Timing {
  const char *name;
  hipEvent_t e0, e1;
};

size_t dtype_size(int dt) {
  switch (dt) {
    case TTNET_F32: return 4;
    case TTNET_I64: return 8;
    case TTNET_U8: return 1;
    case TTNET_U16: return 2;
    case TTNET_U64: return 8;
  }
  return 0;
}

}  // namespace
}  // namespace ttnet

using namespace ttnet;

struct ttnet_plan {
  ttnet_net_desc desc{};
  int device = 0;
  int p = 0;
  int n_classes = 1000, inter = 1000, fcsize = 0;
  int featC = 0, featPP = 0;        // last block: channels, pooled pixels per channel
  std::string head;
  std::vector<MultiHead> blocks;
  std::map<std::string, Tensor> tensors;
  std::vector<std::string> key_order;
  bool finalized = false;
  GatePath path = GatePath::TwoLaunch;
  uint32_t *tap = nullptr;          // fused path: branch dwords of a non-last block, filled on demand by ttnet_read_stage
  size_t tap_elems = 0;
  float *va_scale = nullptr, *va_shift = nullptr;   // vAlexnet stem BatchNorm folded
  float *va_u8_tab = nullptr;       // vAlexnet, uint8 input: folded weights, border-class constants, centres (va_stem_u8_fold)
  size_t full_fix_cap = 0;          // full variant: list entries of Lane::full_fix
  // vAlexnet, ttnet_certify_u8 (certify.hip): derived from the loaded state by the first call after a (re)load; dropped with
  // every tensor, table or normalisation change (drop_certify)
  struct Certify {
    double *A = nullptr, *c0 = nullptr;       // effective head, stored [30976][10], and [10]
    double *stem_bn = nullptr, *slack = nullptr;   // [2][64] folded features.2, [64] widening of the stem bounds
    uint64_t *t3w = nullptr;                  // Block_conv3's table as 64-entry words
    double *wsum = nullptr;                   // [64][3][5][5] summed stem kernels (attack.hip)
    bool ready = false;
  } cert;
  float *full_gel = nullptr;        // full variant: GELU tables of the fast kernels (launch_full_gelu_tables), shared by all lanes

  // stem
  uint16_t *stem_wt = nullptr;      // fp16 x 2 split weights, fragment order
  float *stem_init = nullptr;       // accumulator start values (folded BN shift), 64 floats
  uint32_t *norm_tab = nullptr;     // uint8 input: centres and border corrections (stem_split_weights_u8)
  uint16_t *stem_wt_u8 = nullptr;   // uint8 input: split weights with the normalisation folded in
  float *stem_init_u8 = nullptr;
  // Normalize of the uint8 input: utils/preprocess.py:107-108 (ImageNet); a vAlexnet plan starts from the CIFAR ones
  float in_mean[3] = {0.485f, 0.456f, 0.406f}, in_std[3] = {0.229f, 0.224f, 0.225f};
  // head
  float *w1p = nullptr;             // scratch for the permuted lin1 weights (finalize only)
  uint16_t *w1f = nullptr;          // lin1 weights, two fp16 planes in fragment order
  float *bn_scale = nullptr, *bn_shift = nullptr;
  uint16_t *w2f = nullptr;          // lin2 weights, split planes in fragment order, K padded to 16
  float lin2_inv = 1.f;             // 1 / (weight prescale x activation prescale)
  size_t part_elems = 0;
  size_t table_bytes = 0, workspace_bytes = 0;
  // truth-table usage counts (usage.hip): the counters live in the BlockTTs, the scratch in the lanes
  bool usage_on = false;
  size_t usage_bytes = 0;
  int usage_scheme_dw = kUsageMerged, usage_scheme_pw = kUsageMerged;   // per table shape: depthwise / grouped 1x1 (DESIGN: table usage)
  // care sets (ttnet_plan_set_care): the bitmaps live in the BlockTTs; the lanes' scratch is the usage add's, kept while
  // either of the two is on and accounted in scratch_bytes
  bool care_on = false;
  size_t care_bytes = 0, scratch_bytes = 0;

  bool profiling = false;
  // captured forward per batch size (hipGraph): one launch instead of ~11 on the host side
  struct GraphEntry {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    // a kernel node and the plan's own copy of its launch parameters (argument values in 8-byte slots)
    struct Kernel {
      hipGraphNode_t node = nullptr;
      hipKernelNodeParams p{};
      uint64_t argv[12] = {};
      void *args[12] = {};
    };
    Kernel first, last;               // the kernels that read x / write the logits
    const void *x = nullptr;
    void *out = nullptr;
  };
  // A lane = one set of activation buffers (+ the graphs captured over them).  Lanes share the
  // weights and truth tables; forwards on different lanes may be in flight at the same time on
  // different streams (ttnet_forward_lane).
  struct Lane {
    struct Block {
      uint16_t *o[4] = {nullptr, nullptr, nullptr, nullptr};   // branch outputs out1..out4
      uint64_t *c3_tmp = nullptr;   // full variant: conv3 output at input resolution, before the majority pool
      uint32_t *idx = nullptr;      // fused path: the branch dwords of a last block
    };
    std::vector<uint64_t *> x_rp;   // x_rp[i] / x_cp[i] = input of block i
    std::vector<uint16_t *> x_cp;
    std::vector<Block> blk;
    uint64_t *va_y = nullptr;       // vAlexnet: the concatenated block output [n][256][11] rows
    double *patch_base = nullptr;      // vAlexnet, ttnet_certify_patch_u8: the clean pass's records [nb][4] and unknown sums [nb][10]; first call
    uint64_t *cert_planes = nullptr;   // vAlexnet, ttnet_certify_u8: stem lo / hi [nb][64][10], feature lo / hi [nb][256][11], sums [nb][10]; first call
    float *last_float = nullptr;    // full variant: relu'd output of the last block before AvgPool2d
    uint32_t *full_fix = nullptr;   // full variant: [64] counters + the pixel lists of one grouped 1x1 block (gate_full.hip)
    float *part = nullptr;          // lin1's partial sums
    uint16_t *feat = nullptr;       // features as two fp16 planes in lin1 fragment order
    uint16_t *mid_frag = nullptr;   // lin2's A operand (head_mid_kernel), rows padded to 64
    // table usage: the block input widened to uint64 rows (fused path), the four branch tensors as uint64 rows
    // (fused and two-launch paths) and the branch dwords of a re-run non-last block (fused path)
    uint64_t *u_rows = nullptr, *u_br[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t *u_tap = nullptr;
    std::map<int64_t, GraphEntry> graphs;
    std::map<int64_t, int> eager_calls;
    int64_t last_n = 0;             // images of the last forward on this lane
  };
  std::vector<Lane> lanes;
  int last_lane = 0;                // lane of the latest forward: ttnet_read_stage, from_stem_bits, full_listed_*
  hipStream_t cap_stream = nullptr;
  bool graphs_ok = getenv("TTNET_NO_GRAPH") == nullptr;   // plain launches only when set (debugging)
  int64_t graph_replays = 0;
  int64_t graph_captures = 0, graph_drops = 0;
  std::string graph_off_reason;     // why graphs_ok went false (query "graphs_enabled" + ttnet_last_error)
  // sticky range flag: one word of host-mapped memory that kernels set when a value leaves the
  // range of the fp16 x 2 split (ttnet_common.h: split_out_of_range)
  uint32_t *range_host = nullptr, *range_dev = nullptr;
  std::vector<Timing> timings;
  size_t timing_used = 0;

  std::vector<void *> owned;        // everything hipMalloc'ed, freed in destroy
};

int ttnet::ensure_dynamic_lds(const void *kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return TTNET_OK;
  static std::mutex mu;
  static std::unordered_map<const void *, size_t> done;
  std::lock_guard<std::mutex> lock(mu);
  auto it = done.find(kernel);
  if (it != done.end() && it->second >= bytes) return TTNET_OK;
  TT_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done[kernel] = bytes;
  return TTNET_OK;
}

namespace {

template <typename T>
int dev_alloc(ttnet_plan *pl, T **out, size_t count, bool zero, size_t *account = nullptr) {
  void *ptr = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&ptr, bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    return TTNET_E_NOMEM;
  }
  if (zero) TT_HIP(hipMemset(ptr, 0, bytes));
  pl->owned.push_back(ptr);
  if (account) *account += bytes;
  *out = (T *)ptr;
  return TTNET_OK;
}

void dev_free(ttnet_plan *pl, void *ptr) {
  if (!ptr) return;
  auto it = std::find(pl->owned.begin(), pl->owned.end(), ptr);
  if (it != pl->owned.end()) pl->owned.erase(it);
  (void)hipFree(ptr);
}

// what ttnet_certify_u8 derived from the state goes with the state (the lanes' planes hold no state and stay)
void drop_certify(ttnet_plan *pl) {
  auto &c = pl->cert;
  for (void *ptr : {(void *)c.A, (void *)c.c0, (void *)c.stem_bn, (void *)c.slack, (void *)c.t3w, (void *)c.wsum}) dev_free(pl, ptr);
  c = ttnet_plan::Certify{};
}

void add_tensor(ttnet_plan *pl, const std::string &key, std::vector<int64_t> shape, int dtype, bool required) {
  Tensor t;
  t.shape = std::move(shape);
  t.dtype = dtype;
  size_t n = 1;
  for (auto d : t.shape) n *= (size_t)d;
  t.bytes = n * dtype_size(dtype);
  t.required = required;
  pl->tensors[key] = t;
  pl->key_order.push_back(key);
}

void add_bn(ttnet_plan *pl, const std::string &prefix, int c) {
  add_tensor(pl, prefix + ".weight", {c}, TTNET_F32, true);
  add_tensor(pl, prefix + ".bias", {c}, TTNET_F32, true);
  add_tensor(pl, prefix + ".running_mean", {c}, TTNET_F32, true);
  add_tensor(pl, prefix + ".running_var", {c}, TTNET_F32, true);
  add_tensor(pl, prefix + ".num_batches_tracked", {}, TTNET_I64, false);
}

// every Block_TT of the plan (vAlexnet's block has no convf: its entry keeps an empty name)
std::vector<BlockTT *> all_block_tts(ttnet_plan *pl) {
  std::vector<BlockTT *> v;
  for (auto &mh : pl->blocks)
    for (BlockTT *b : {&mh.c1, &mh.c2, &mh.c3, &mh.cf})
      if (!b->g.name.empty()) v.push_back(b);
  return v;
}

void add_block_tt(ttnet_plan *pl, const BlockGeom &g) {
  const int mid = 8 * g.in_planes;
  add_tensor(pl, g.name + ".conv1.weight", {mid, g.cin_g(), g.kh, g.kw}, TTNET_F32, true);
  add_bn(pl, g.name + ".bn1", mid);
  add_tensor(pl, g.name + ".conv2.weight", {g.out_planes, mid / g.groups, 1, 1}, TTNET_F32, true);
  add_bn(pl, g.name + ".bn2", g.out_planes);
  add_tensor(pl, g.name + ".act.grad_scale", {}, TTNET_F32, false);
}

BlockGeom make_geom(const std::string &name, int in_planes, int out_planes, int kh, int kw, int stride, int pad,
                    int groups, bool last) {
  BlockGeom g;
  g.name = name; g.in_planes = in_planes; g.out_planes = out_planes; g.kh = kh; g.kw = kw;
  g.stride = stride; g.pad = pad; g.groups = groups; g.last = last;
  return g;
}

// internal index order of a table = the canonical column order
void identity_perm(BlockTT &b) {
  b.perm.resize(b.g.nbits());
  for (int q = 0; q < b.g.nbits(); ++q) b.perm[q] = (uint8_t)q;
}

// Geometry of the network (mirrors make_small_network,
// models/TT_general_imagenet_v2_small.py:159-203, and the shape-keyed branch padding of
// the block forward, :98-139).
// TT_FHE_XSMALL_vAlexnet (models/TT_FHE_XSMALL_vAlexnet.py:585-660): fixed geometry
int build_geometry_valexnet(ttnet_plan *pl) {
  const ttnet_net_desc &d = pl->desc;
  if (d.image_h != 32 || d.image_w != 32) {
    set_error("vAlexnet takes 32x32 inputs (got %dx%d)", d.image_h, d.image_w);
    return TTNET_E_UNSUPPORTED;
  }
  if (d.max_batch < 1) {
    set_error("max_batch must be positive");
    return TTNET_E_INVALID;
  }
  pl->path = GatePath::VAlexnet;
  pl->p = 64;
  pl->n_classes = va::kClasses; pl->inter = 100; pl->fcsize = va::kFeat;
  pl->head = "features.7";
  const float mean[3] = {0.4914f, 0.4822f, 0.4465f}, std[3] = {0.2023f, 0.1994f, 0.2010f};   // cifar_transform, utils/preprocess.py:82-87
  std::copy(mean, mean + 3, pl->in_mean);
  std::copy(std, std + 3, pl->in_std);
  for (const char *pre : {"VGG_Model16_0", "features.0"}) {      // one conv module registered under two names
    add_tensor(pl, std::string(pre) + ".weight", {64, 3, 3, 3}, TTNET_F32, std::string(pre) == "features.0");
    add_tensor(pl, std::string(pre) + ".bias", {64}, TTNET_F32, std::string(pre) == "features.0");
  }
  add_bn(pl, "features.2", 64);
  add_tensor(pl, "features.4.grad_scale", {}, TTNET_F32, false);
  MultiHead mh;
  mh.name = "features.5";
  mh.C = 64; mh.H = 10; mh.W = 10; mh.Ho = 11; mh.Wo = 11; mh.stride = 1; mh.last = true;
  mh.c1.g = make_geom("features.5.Block_conv1", 64, 64, 3, 2, 1, 1, 64, false);
  mh.c2.g = make_geom("features.5.Block_conv2", 64, 64, 2, 3, 1, 1, 64, false);
  mh.c3.g = make_geom("features.5.Block_conv3", 64, 64, 1, 1, 1, 0, 8, false);
  for (BlockTT *b : {&mh.c1, &mh.c2, &mh.c3}) {
    add_block_tt(pl, b->g);
    identity_perm(*b);
  }
  pl->blocks.push_back(mh);
  add_tensor(pl, "features.7.lin1.weight", {pl->inter, pl->fcsize}, TTNET_F32, true);
  add_bn(pl, "features.7.BN2", pl->inter);
  add_tensor(pl, "features.7.lin2.weight", {pl->n_classes, pl->inter}, TTNET_F32, true);
  add_tensor(pl, "features.7.lin2.bias", {pl->n_classes}, TTNET_F32, true);
  return TTNET_OK;
}

int build_geometry(ttnet_plan *pl) {
  const ttnet_net_desc &d = pl->desc;
  if (d.variant == TTNET_VALEXNET) return build_geometry_valexnet(pl);
  int kh = 4, kw = 4, pad = 2, gsize = 16;
  if (d.variant == TTNET_SMALL) {
    pl->path = GatePath::TwoLaunch;    // (Fused below when every block allows it)
  } else if (d.variant == TTNET_XSMALL) {
    kh = kw = 2; pad = 1; gsize = 4;
    pl->path = GatePath::XSmall;
  } else if (d.variant == TTNET_FULL) {
    gsize = 30; pad = 3;               // kernels (6,5) / (5,6): set per branch below
    pl->path = GatePath::Full;
  } else {
    set_error("unknown variant %d", d.variant);
    return TTNET_E_INVALID;
  }
  if (d.image_h != 224 || d.image_w != 224) {
    set_error("only 224x224 inputs are supported (got %dx%d)", d.image_h, d.image_w);
    return TTNET_E_UNSUPPORTED;
  }
  if (d.nfilter < 1 || d.tfilter < 1 || d.max_batch < 1) {
    set_error("nfilter, tfilter and max_batch must be positive");
    return TTNET_E_INVALID;
  }
  const bool full_variant = pl->path == GatePath::Full;
  const int p = d.nfilter * d.tfilter;
  pl->p = p;
  // The reference constructs any p whose group counts divide its channel counts (TT_general_imagenet_v2_small.py:
  // 165-167, :28-76); a fan-in of 16 (the truth tables of the small variant) needs p % 16 == 0, and the depthwise
  // tables of both table variants are striped by 16 channels.  Built: p in {16, 32, .., 128} for the table variants
  // (one, two or four 32-channel M-tiles in the stem kernel), p <= 64 for the full variant; anything else is refused here.
  if (p > 128 || (full_variant && p > 64) || (!full_variant && p % 16 != 0)) {
    set_error("p = nfilter*tfilter = %d: built for p <= 128 with p %% 16 == 0 (fan-in 16 / tables striped by 16 channels; full variant: p <= 64)", p);
    return TTNET_E_UNSUPPORTED;
  }
  if (d.layers >= 3 && p != 64) {
    set_error("--layers %d at p = %d: the stride-1 blocks (two-launch gate kernels, channel-word layout) are built for p = 64", d.layers, p);
    return TTNET_E_UNSUPPORTED;
  }
  std::vector<int> cfg, strides;
  switch (d.layers) {   // TT_general_imagenet_v2_small.py:172-181; a bare entry is a stride-1 block
    case 0: cfg = {p, 2 * p}; strides = {2, 2}; break;
    case 1: cfg = {p, 2 * p, 4 * p}; strides = {2, 2, 2}; break;
    case 2: cfg = {p, 2 * p, 4 * p, 8 * p}; strides = {2, 2, 2, 2}; break;
    case 3: cfg = {p, 2 * p, 4 * p, 8 * p}; strides = {1, 2, 2, 2}; break;
    case 4: cfg = {p, 2 * p, 2 * p, 4 * p, 8 * p}; strides = {1, 2, 1, 2, 2}; break;
    default:
      set_error("--layers %d: the reference defines 0..4", d.layers);
      return TTNET_E_UNSUPPORTED;
  }
  if (d.layers >= 3 && d.variant != TTNET_SMALL) {
    set_error("--layers %d (stride-1 blocks) is built for the small variant only", d.layers);
    return TTNET_E_UNSUPPORTED;
  }
  add_tensor(pl, "features.1.weight", {p, 3, 7, 7}, TTNET_F32, true);
  add_bn(pl, "features.2", p);
  add_tensor(pl, "features.3.grad_scale", {}, TTNET_F32, false);

  int h = 56, w = 56, in_planes = p;
  for (size_t i = 0; i < cfg.size(); ++i) {
    MultiHead mh;
    mh.name = "features." + std::to_string(4 + i);
    const int out_planes = cfg[i];
    mh.last = (out_planes == cfg.back());
    mh.C = in_planes; mh.H = h; mh.W = w;
    const int stride = strides[i];
    mh.stride = stride;
    int ho = (h + 2 * pad - kh) / stride + 1, wo = (w + 2 * pad - kw) / stride + 1;
    if (full_variant) {
      // models/TT_general_imagenet_v2.py:98-128: conv1 is (6,5), conv2 (5,6); at 29x29 they come
      // out 15x16 / 16x15 and are padded (bottom / right) to 16x16, out3/out4 by (0,2,0,2)
      if (w == 56) { mh.off34 = 1; ho = wo = 29; }
      else if (w == 29) { mh.off34 = 0; ho = wo = 16; }
      else if (w == 16) { mh.off34 = 0; ho = wo = 9; }
      else {
        set_error("%s: no branch-padding rule for width %d (full variant)", mh.name.c_str(), w);
        return TTNET_E_UNSUPPORTED;
      }
    } else {
    // branch padding keyed by the input width (:98-139): out3/out4 are floor(h/2) wide
    if (w == 56) mh.off34 = 1;                       // pad0 = ZeroPad2d((1,0,1,0))
    else if (w == 29 || w == 15 || w == 8 || w == 16 || w == 30 || w == 57 || w == 58) mh.off34 = 0;   // pad2 = (0,1,0,1)
    else {
      set_error("%s: no branch-padding rule for width %d", mh.name.c_str(), w);
      return TTNET_E_UNSUPPORTED;
    }
    if (h / stride + 1 != ho || w / stride + 1 != wo || h != w) {
      set_error("%s: branch shapes do not line up (%dx%d -> %dx%d)", mh.name.c_str(), h, w, ho, wo);
      return TTNET_E_UNSUPPORTED;
    }
    }
    mh.Ho = ho; mh.Wo = wo;
    if (in_planes % gsize) {
      set_error("in_channels must be divisible by groups (in_planes=%d, group size %d)", in_planes, gsize);
      return TTNET_E_INVALID;
    }
    const int kh1 = full_variant ? 6 : kh, kw1 = full_variant ? 5 : kw, kh2 = full_variant ? 5 : kh, kw2 = full_variant ? 6 : kw;
    mh.c1.g = make_geom(mh.name + ".Block_conv1", in_planes, in_planes, kh1, kw1, stride, pad, in_planes, false);
    mh.c2.g = make_geom(mh.name + ".Block_conv2", in_planes, in_planes, kh2, kw2, stride, pad, in_planes, false);
    mh.c3.g = make_geom(mh.name + ".Block_conv3", in_planes, in_planes, 1, 1, 1, 0, in_planes / gsize, false);
    const int cf_out = mh.last ? 4 * in_planes : 2 * out_planes;
    mh.cf.g = make_geom(mh.name + ".Block_convf", 4 * in_planes, cf_out, 1, 1, 1, 0, 4 * in_planes / gsize, mh.last);
    add_block_tt(pl, mh.c1.g);
    add_block_tt(pl, mh.c2.g);
    add_block_tt(pl, mh.c3.g);
    add_tensor(pl, mh.name + ".act.grad_scale", {}, TTNET_F32, false);
    add_block_tt(pl, mh.cf.g);
    // internal index orders (table variants only)
    if (!full_variant)
      for (BlockTT *b : {&mh.c1, &mh.c2, &mh.c3}) identity_perm(*b);
    // convf group = gsize/4 channels x 4 branches; reference interleave is channel 4c+branch (:144-147),
    // internal index bit = (gsize/4)*branch + channel-in-group
    const int nch = gsize / 4;
    if (!full_variant) {
      mh.cf.perm.resize(gsize);
      for (int br = 0; br < 4; ++br)
        for (int cl = 0; cl < nch; ++cl) mh.cf.perm[nch * br + cl] = (uint8_t)(4 * cl + br);
    }
    pl->blocks.push_back(mh);
    h = ho; w = wo;
    in_planes = 2 * out_planes;
  }
  if (d.variant == TTNET_SMALL && getenv("TTNET_GATE_UNFUSED") == nullptr) {
    bool fusable = true;
    for (const MultiHead &mh : pl->blocks)
      fusable = fusable && fused_block_supported(mh.C, mh.H, mh.Ho, mh.stride, mh.c1.g.pad, mh.c1.g.kh, mh.c1.g.kw);
    if (fusable) pl->path = GatePath::Fused;
  }
  const MultiHead &lb = pl->blocks.back();
  pl->featC = lb.cf.g.out_planes;
  pl->featPP = (lb.Ho / 2) * (lb.Wo / 2);
  pl->fcsize = pl->featC * pl->featPP;
  pl->head = "features." + std::to_string(4 + cfg.size() + 2);
  add_tensor(pl, pl->head + ".lin1.weight", {pl->inter, pl->fcsize}, TTNET_F32, true);
  add_bn(pl, pl->head + ".BN2", pl->inter);
  add_tensor(pl, pl->head + ".lin2.weight", {pl->n_classes, pl->inter}, TTNET_F32, true);
  add_tensor(pl, pl->head + ".lin2.bias", {pl->n_classes}, TTNET_F32, true);
  return TTNET_OK;
}

// Activation workspace of one lane.  Everything is zeroed once: the branch-padding borders, the
// k padding of lin2's A operand and the rows of the lin1 operand beyond the batch are never
// written again.
int alloc_workspace(ttnet_plan *pl, ttnet_plan::Lane &L) {
  const int nb = pl->desc.max_batch;
  size_t *ws = &pl->workspace_bytes;
  const int kpad = (pl->inter + 15) / 16 * 16;
  const GatePath path = pl->path;
  L.x_rp.assign(pl->blocks.size(), nullptr);
  L.x_cp.assign(pl->blocks.size(), nullptr);
  L.blk.assign(pl->blocks.size(), {});
  if (path == GatePath::VAlexnet) {
    TT_TRY(dev_alloc(pl, &L.x_rp[0], (size_t)nb * va::kStemRows, true, ws));
    TT_TRY(dev_alloc(pl, &L.va_y, (size_t)nb * va::kFeatRows, true, ws));
  } else {
    for (size_t i = 0; i < pl->blocks.size(); ++i) {
      const MultiHead &mh = pl->blocks[i];
      ttnet_plan::Lane::Block &bw = L.blk[i];
      if (path == GatePath::Fused) {
        // one activation layout: rows of uint64 / uint32 / uint16 words by width (the stem's output stays uint64)
        const size_t bytes = (size_t)nb * mh.C * mh.H * (i == 0 ? 8 : row_bytes(mh.W));
        TT_TRY(dev_alloc(pl, &L.x_rp[i], (bytes + 7) / 8, true, ws));
        // x_cp and the branch outputs are unused here: placeholders so that gate_args stays valid
        TT_TRY(dev_alloc(pl, &L.x_cp[i], 4, true, ws));
        for (int b = 0; b < 4; ++b) TT_TRY(dev_alloc(pl, &bw.o[b], 8, true, ws));
        if (mh.last) TT_TRY(dev_alloc(pl, &bw.idx, (size_t)nb * (mh.C / 8) * mh.Ho * mh.Wo, true, ws));
        continue;
      }
      TT_TRY(dev_alloc(pl, &L.x_rp[i], (size_t)nb * mh.C * mh.H, true, ws));
      TT_TRY(dev_alloc(pl, &L.x_cp[i], path == GatePath::Full ? 8 : (size_t)nb * mh.H * mh.W * (mh.C / 16), true, ws));
      if (path == GatePath::Full) TT_TRY(dev_alloc(pl, &bw.c3_tmp, (size_t)nb * mh.C * mh.H, true, ws));
      for (int b = 0; b < 4; ++b) {
        const size_t words16 = (size_t)nb * mh.Ho * mh.Wo * (mh.C / 16), rows64 = (size_t)nb * mh.C * mh.Ho;
        TT_TRY(dev_alloc(pl, &bw.o[b], (path == GatePath::XSmall || path == GatePath::Full) ? rows64 * 4 : words16, true, ws));
      }
    }
    if (path == GatePath::Full) {
      const MultiHead &lb = pl->blocks.back();
      TT_TRY(dev_alloc(pl, &L.last_float, (size_t)nb * lb.cf.g.out_planes * lb.Ho * lb.Wo, true, ws));
      size_t cap = 0;                                  // pixels x groups of the largest binarised 1x1 block
      for (const MultiHead &mh : pl->blocks) {
        cap = std::max(cap, part::full_fix_entries(mh.c3.g.groups, mh.H, mh.W));
        if (!mh.last) cap = std::max(cap, part::full_fix_entries(mh.cf.g.groups, mh.Ho, mh.Wo));
      }
      pl->full_fix_cap = cap * (size_t)nb;
      TT_TRY(dev_alloc(pl, &L.full_fix, 64 + pl->full_fix_cap, true, ws));
      if (!pl->full_gel) {
        TT_TRY(dev_alloc(pl, &pl->full_gel, full_gelu_tables_elems(), false, ws));
        TT_TRY(launch_full_gelu_tables(pl->full_gel, nullptr));
        TT_HIP(hipDeviceSynchronize());
      }
    }
  }
  const int nb_pad = (nb + 255) / 256 * 256;          // the lin1 GEMM walks whole 256-row tiles
  TT_TRY(dev_alloc(pl, &L.feat, frag_elems(nb_pad, pl->fcsize), true, ws));
  TT_TRY(dev_alloc(pl, &L.mid_frag, frag_elems((nb + 63) / 64 * 64, kpad), true, ws));
  size_t pe = 0;
  for (int n = 1; n <= nb; n = n < 256 ? 256 : n + 256) pe = std::max(pe, gemm_f16x2_part_elems(std::min(n, nb), pl->inter, pl->fcsize / 16));
  pe = std::max(pe, gemm_f16x2_part_elems(nb, pl->inter, pl->fcsize / 16));
  pl->part_elems = pe;
  TT_TRY(dev_alloc(pl, &L.part, pe, false, ws));
  return TTNET_OK;
}

int allocate(ttnet_plan *pl) {
  size_t *tb = &pl->table_bytes;
  TT_HIP(hipHostMalloc((void **)&pl->range_host, sizeof(uint32_t), hipHostMallocMapped));
  *pl->range_host = 0u;
  TT_HIP(hipHostGetDevicePointer((void **)&pl->range_dev, pl->range_host, 0));
  const int kpad = (pl->inter + 15) / 16 * 16;
  for (auto &kv : pl->tensors) TT_TRY(dev_alloc(pl, (uint8_t **)&kv.second.dev, kv.second.bytes, true));
  const bool valexnet = pl->path == GatePath::VAlexnet;
  if (valexnet) {
    TT_TRY(dev_alloc(pl, &pl->va_scale, 64, false));
    TT_TRY(dev_alloc(pl, &pl->va_shift, 64, false));
    TT_TRY(dev_alloc(pl, &pl->va_u8_tab, va_stem_u8_table_elems(), true));
  } else {
    TT_TRY(dev_alloc(pl, &pl->stem_wt, stem_split_weights_elems(), false));
    TT_TRY(dev_alloc(pl, &pl->stem_init, 64, false));
    TT_TRY(dev_alloc(pl, &pl->norm_tab, stem_u8_table_elems(), true));
    TT_TRY(dev_alloc(pl, &pl->stem_wt_u8, stem_split_weights_elems(), true));
    TT_TRY(dev_alloc(pl, &pl->stem_init_u8, 64, true));
    TT_TRY(dev_alloc(pl, &pl->w1p, (size_t)pl->inter * pl->fcsize, false));
  }
  for (auto &mh : pl->blocks) {
    for (BlockTT *b : {&mh.c1, &mh.c2, &mh.c3, &mh.cf}) {
      if (valexnet && b == &mh.cf) continue;          // vAlexnet has no Block_convf
      const BlockGeom &g = b->g;
      if (pl->path != GatePath::Full) {
        TT_TRY(dev_alloc(pl, (uint8_t **)&b->table, g.table_bytes(), true, tb));
        TT_TRY(dev_alloc(pl, &b->perm_dev, b->perm.size(), false));
        TT_HIP(hipMemcpy(b->perm_dev, b->perm.data(), b->perm.size(), hipMemcpyHostToDevice));
      }
      TT_TRY(dev_alloc(pl, &b->s1, (size_t)8 * g.in_planes, false));
      TT_TRY(dev_alloc(pl, &b->t1, (size_t)8 * g.in_planes, false));
      TT_TRY(dev_alloc(pl, &b->s2, g.out_planes, false));
      TT_TRY(dev_alloc(pl, &b->t2, g.out_planes, false));
      TT_TRY(dev_alloc(pl, &b->near_dev, 1, true));
    }
  }
  if (pl->path == GatePath::Fused)
    for (auto &mh : pl->blocks) {
      TT_TRY(dev_alloc(pl, (uint8_t **)&mh.img_dw, (size_t)mh.C * 16384, false, tb));
      TT_TRY(dev_alloc(pl, (uint8_t **)&mh.img_c3, (size_t)(mh.C / 8) * 65536, false, tb));
    }
  TT_TRY(dev_alloc(pl, &pl->w1f, frag_elems((pl->inter + 127) / 128 * 128, pl->fcsize), false));
  TT_TRY(dev_alloc(pl, &pl->bn_scale, pl->inter, false));
  TT_TRY(dev_alloc(pl, &pl->bn_shift, pl->inter, false));
  TT_TRY(dev_alloc(pl, &pl->w2f, frag_elems((pl->n_classes + 63) / 64 * 64, kpad), true));
  return alloc_workspace(pl, pl->lanes.emplace_back());   // lane 0
}

int fetch(const Tensor &t, std::vector<float> &host) {
  host.resize(t.bytes / 4);
  TT_HIP(hipMemcpy(host.data(), t.dev, t.bytes, hipMemcpyDeviceToHost));
  return TTNET_OK;
}

// eval-mode BatchNorm as y = x*scale + shift, folded in float64
int fold_bn(ttnet_plan *pl, const std::string &prefix, std::vector<double> &scale, std::vector<double> &shift) {
  std::vector<float> w, b, m, v;
  TT_TRY(fetch(pl->tensors[prefix + ".weight"], w));
  TT_TRY(fetch(pl->tensors[prefix + ".bias"], b));
  TT_TRY(fetch(pl->tensors[prefix + ".running_mean"], m));
  TT_TRY(fetch(pl->tensors[prefix + ".running_var"], v));
  scale.resize(w.size());
  shift.resize(w.size());
  for (size_t i = 0; i < w.size(); ++i) {
    scale[i] = (double)w[i] / sqrt((double)v[i] + kBnEps);
    shift[i] = (double)b[i] - (double)m[i] * scale[i];
  }
  return TTNET_OK;
}

// stem: BN scale folded into the weights, which are split into two prescaled fp16 planes in MFMA
// fragment order; BN shift as the weights of one more k-row (stem.hip)
int prepare_stem(ttnet_plan *pl) {
  std::vector<float> w;
  TT_TRY(fetch(pl->tensors["features.1.weight"], w));
  std::vector<uint16_t> wf(stem_split_weights_elems());
  std::vector<double> sc, sh;
  TT_TRY(fold_bn(pl, "features.2", sc, sh));
  float init[64];
  if (!stem_split_weights(w.data(), sc.data(), sh.data(), pl->p, wf.data(), init)) {
    set_error("stem: the folded BatchNorm shift of features.2 is outside the range of the split operands");
    return TTNET_E_UNSUPPORTED;
  }
  TT_HIP(hipMemcpy(pl->stem_wt, wf.data(), wf.size() * 2, hipMemcpyHostToDevice));
  TT_HIP(hipMemcpy(pl->stem_init, init, sizeof(init), hipMemcpyHostToDevice));
  return TTNET_OK;
}

// uint8 input: the stem's weights with ToTensor + Normalize folded in (stem.hip, U8).  From the loaded weights and the
// plan's mean / std: at finalize and again whenever ttnet_plan_set_input_norm changes them.
int prepare_stem_u8(ttnet_plan *pl) {
  std::vector<float> w;
  TT_TRY(fetch(pl->tensors["features.1.weight"], w));
  std::vector<uint16_t> wf(stem_split_weights_elems());
  std::vector<uint32_t> tab(stem_u8_table_elems(), 0u);
  std::vector<double> sc, sh;
  TT_TRY(fold_bn(pl, "features.2", sc, sh));
  float init[64];
  if (!stem_split_weights_u8(w.data(), sc.data(), sh.data(), pl->p, pl->in_mean, pl->in_std, wf.data(), init, tab.data())) {
    set_error("stem (uint8 input): the folded BatchNorm shift of features.2 is outside the range of the split operands");
    return TTNET_E_UNSUPPORTED;
  }
  TT_HIP(hipMemcpy(pl->stem_wt_u8, wf.data(), wf.size() * 2, hipMemcpyHostToDevice));
  TT_HIP(hipMemcpy(pl->stem_init_u8, init, sizeof(init), hipMemcpyHostToDevice));
  TT_HIP(hipMemcpy(pl->norm_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  return TTNET_OK;
}

// vAlexnet, uint8 input: the stem's weights and bias with ToTensor + Normalize folded in, one constant per border class
// (gate_va.hip).  From the loaded tensors and the plan's mean / std: at finalize and again whenever
// ttnet_plan_set_input_norm changes them.
int prepare_va_stem_u8(ttnet_plan *pl) {
  std::vector<float> w, b, tab(va_stem_u8_table_elems());
  TT_TRY(fetch(pl->tensors["features.0.weight"], w));
  TT_TRY(fetch(pl->tensors["features.0.bias"], b));
  va_stem_u8_fold(w.data(), b.data(), pl->in_mean, pl->in_std, tab.data());
  TT_HIP(hipMemcpy(pl->va_u8_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  return TTNET_OK;
}

int upload_f32(float *dst, const std::vector<double> &src) {
  std::vector<float> f(src.begin(), src.end());
  TT_HIP(hipMemcpy(dst, f.data(), f.size() * 4, hipMemcpyHostToDevice));
  return TTNET_OK;
}

int build_table(ttnet_plan *pl, BlockTT &b, hipStream_t s) {
  std::vector<double> s1, t1, s2, t2;
  TT_TRY(fold_bn(pl, b.g.name + ".bn1", s1, t1));
  TT_TRY(fold_bn(pl, b.g.name + ".bn2", s2, t2));
  TT_HIP(hipMemcpy(b.s1, s1.data(), s1.size() * 8, hipMemcpyHostToDevice));
  TT_HIP(hipMemcpy(b.t1, t1.data(), t1.size() * 8, hipMemcpyHostToDevice));
  TT_HIP(hipMemcpy(b.s2, s2.data(), s2.size() * 8, hipMemcpyHostToDevice));
  TT_HIP(hipMemcpy(b.t2, t2.data(), t2.size() * 8, hipMemcpyHostToDevice));
  if (b.user_table || pl->path == GatePath::Full) return TTNET_OK;
  TT_HIP(hipMemsetAsync(b.near_dev, 0, sizeof(unsigned), s));
  LutBuildArgs a{};
  a.w1 = (const float *)pl->tensors[b.g.name + ".conv1.weight"].dev;
  a.w2 = (const float *)pl->tensors[b.g.name + ".conv2.weight"].dev;
  a.s1 = b.s1; a.t1 = b.t1; a.s2 = b.s2; a.t2 = b.t2;
  a.perm = b.perm_dev;
  a.groups = b.g.groups; a.n = b.g.nbits(); a.mid_g = b.g.mid_g(); a.cout_g = b.g.cout_g(); a.last = b.g.last;
  a.table = b.table;
  a.near_ties = b.near_dev;
  return launch_lut_build(a, s);
}

// the near-tie counts of the tables built at finalize (after its synchronisation)
int read_near_ties(ttnet_plan *pl) {
  for (BlockTT *b : all_block_tts(pl)) {
    if (b->user_table || pl->path == GatePath::Full) continue;
    unsigned v = 0;
    TT_HIP(hipMemcpy(&v, b->near_dev, sizeof(v), hipMemcpyDeviceToHost));
    b->near_ties = v;
  }
  return TTNET_OK;
}

// (name == nullptr: not timed)
void begin_timing(ttnet_plan *pl, const char *name, hipStream_t s) {
  if (!pl->profiling || !name) return;
  if (pl->timing_used == pl->timings.size()) {
    Timing t{name, nullptr, nullptr};
    (void)hipEventCreate(&t.e0);
    (void)hipEventCreate(&t.e1);
    pl->timings.push_back(t);
  }
  pl->timings[pl->timing_used].name = name;
  (void)hipEventRecord(pl->timings[pl->timing_used].e0, s);
}
void end_timing(ttnet_plan *pl, const char *name, hipStream_t s) {
  if (!pl->profiling || !name) return;
  (void)hipEventRecord(pl->timings[pl->timing_used].e1, s);
  pl->timing_used++;
}

#define TT_TIMED(pl, name, s, expr) \
  do {                              \
    begin_timing(pl, name, s);      \
    int r__ = (expr);               \
    end_timing(pl, name, s);        \
    if (r__ != TTNET_OK) return r__; \
  } while (0)

GateBlockArgs gate_args(const ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n) {
  const MultiHead &mh = pl->blocks[i];
  uint16_t *const *o = L.blk[i].o;
  GateBlockArgs a{};
  a.n = n; a.C = mh.C; a.H = mh.H; a.W = mh.W; a.Ho = mh.Ho; a.Wo = mh.Wo; a.off34 = mh.off34;
  a.kh1 = mh.c1.g.kh; a.kw1 = mh.c1.g.kw; a.kh2 = mh.c2.g.kh; a.kw2 = mh.c2.g.kw;
  a.stride = mh.c1.g.stride; a.pad = mh.c1.g.pad;
  a.cf_bits = mh.cf.g.cout_g();
  a.x_rp = L.x_rp[i]; a.x_cp = L.x_cp[i];
  a.t_dw1 = (const uint8_t *)mh.c1.table; a.t_dw2 = (const uint8_t *)mh.c2.table;
  a.t_c3 = (const uint16_t *)mh.c3.table;
  a.o1 = o[0]; a.o2 = o[1]; a.o3 = o[2]; a.o4 = o[3];
  return a;
}

// the branch outputs of block i as uint64 rows (x-small and full variants)
std::array<uint64_t *, 4> branch_rows(const ttnet_plan::Lane &L, size_t i) {
  uint16_t *const *o = L.blk[i].o;
  return {(uint64_t *)o[0], (uint64_t *)o[1], (uint64_t *)o[2], (uint64_t *)o[3]};
}

static const char *kS1Names[] = {"gate_stage1.f4", "gate_stage1.f5", "gate_stage1.f6", "gate_stage1.f7"};
static const char *kPfNames[] = {"gate_pf.f4", "gate_pf.f5", "gate_pf.f6", "gate_pf.f7"};

// One block on the two launches of gate.hip: stage 1, then convf (or the last block's pool + flatten)
int run_two_launch_block(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, hipStream_t s) {
  const MultiHead &mh = pl->blocks[i];
  const GateBlockArgs a = gate_args(pl, L, i, n);
  TT_TIMED(pl, kS1Names[std::min<size_t>(i, 3)], s, launch_gate_stage1(a, s));
  if (!mh.last)
    TT_TIMED(pl, kPfNames[std::min<size_t>(i, 3)], s, launch_gate_pf(a, (const uint8_t *)mh.cf.table, L.x_cp[i + 1], L.x_rp[i + 1], s));
  else
    TT_TIMED(pl, "gate_last", s, launch_gate_last(a, (const float *)mh.cf.table, L.feat, pl->range_dev, s));
  return TTNET_OK;
}

// Fused block i on the lane's buffers.  idx: where its branch dwords go -- the output of a last block, an optional tap
// otherwise
FusedBlockArgs fused_args(const ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint32_t *idx) {
  const MultiHead &mh = pl->blocks[i];
  FusedBlockArgs f{};
  f.n = n; f.C = mh.C; f.H = mh.H; f.Ho = mh.Ho; f.off34 = mh.off34; f.last = mh.last ? 1 : 0;
  f.x = L.x_rp[i]; f.img_c3 = mh.img_c3; f.img_dw = mh.img_dw;
  f.t_cf = mh.last ? nullptr : (const uint8_t *)mh.cf.table;
  f.y = mh.last ? nullptr : (void *)L.x_rp[i + 1];
  f.idx = idx;
  return f;
}

// One block in one launch (gate_fused.hip); a last block adds the pool + flatten launch
int run_fused_block(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, hipStream_t s) {
  static const char *kBlkNames[] = {"gate_block.f4", "gate_block.f5", "gate_block.f6", "gate_block.f7"};
  const MultiHead &mh = pl->blocks[i];
  uint32_t *idx = mh.last ? L.blk[i].idx : nullptr;
  TT_TIMED(pl, kBlkNames[std::min<size_t>(i, 3)], s, launch_gate_block(fused_args(pl, L, i, n, idx), s));
  if (mh.last)
    TT_TIMED(pl, "gate_last", s, launch_gate_last(gate_args(pl, L, i, n), (const float *)mh.cf.table, L.feat, pl->range_dev, s, idx));
  return TTNET_OK;
}

// ---- a stage of the last forward as uint64 rows (ttnet_read_stage, ttnet_table_usage_add) ----
// Each gate path keeps its activations in its own layout; these three answer in the one layout of the C ABI.
// timing: the name the conversion launches are timed under (nullptr: not timed).

// The branch dwords of fused block i, whose branch tensors never reach HBM: a last block's are its output; any other
// block is run once more on its (still resident) input with `tap` attached -- it rewrites the next block's input with
// the same bits
int fused_branch_dwords(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint32_t *tap, const char *timing, hipStream_t s,
                        const uint32_t **dwords) {
  *dwords = pl->blocks[i].last ? L.blk[i].idx : tap;
  if (!pl->blocks[i].last) TT_TIMED(pl, timing, s, launch_gate_block(fused_args(pl, L, i, n, tap), s));
  return TTNET_OK;
}

// The input of block i as rows [n][C][H]: in place, but for the compact rows of the fused path (blocks after the
// first), which are widened into buf
int block_input_rows(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint64_t *buf, const char *timing, hipStream_t s,
                     const uint64_t **rows) {
  const MultiHead &mh = pl->blocks[i];
  *rows = L.x_rp[i];
  if (pl->path == GatePath::Fused && i > 0) {
    TT_TIMED(pl, timing, s, launch_widen_rows(L.x_rp[i], buf, (size_t)n * mh.C * mh.H, mh.W, s));
    *rows = buf;
  }
  return TTNET_OK;
}

// Branch k of block i after its padding as rows [n][C][Ho]: in place, or converted into buf (fused path: from the
// dwords of fused_branch_dwords)
int branch_as_rows(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int k, int n, const uint32_t *dwords, uint64_t *buf,
                   const char *timing, hipStream_t s, const uint64_t **rows) {
  const MultiHead &mh = pl->blocks[i];
  *rows = buf;
  switch (pl->path) {
    case GatePath::TwoLaunch: TT_TIMED(pl, timing, s, launch_cp_to_rp(L.blk[i].o[k], buf, n, mh.C, mh.Ho, mh.Wo, s)); break;
    case GatePath::Fused: TT_TIMED(pl, timing, s, launch_branch_rows(dwords, buf, n, mh.C, mh.Ho, k, s)); break;
    default: *rows = (const uint64_t *)L.blk[i].o[k]; break;      // x-small and full keep row-packed branch tensors
  }
  return TTNET_OK;
}

// One block of the x-small variant (gate_xs.hip)
int run_xs_block(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, hipStream_t s) {
  const MultiHead &mh = pl->blocks[i];
  const std::array<uint64_t *, 4> o64 = branch_rows(L, i);
  TT_TIMED(pl, kS1Names[std::min<size_t>(i, 3)], s, launch_xs_branches(gate_args(pl, L, i, n), mh.c3.table, o64.data(), s));
  if (!mh.last)
    TT_TIMED(pl, kPfNames[std::min<size_t>(i, 3)], s, launch_xs_pf(n, mh.C, mh.Ho, mh.Wo, mh.cf.g.cout_g(), o64.data(), mh.cf.table, L.x_rp[i + 1], s));
  else
    TT_TIMED(pl, "gate_last", s,
             launch_xs_last(n, mh.C, mh.Ho, mh.Wo, mh.cf.g.cout_g(), o64.data(), (const float *)mh.cf.table, L.feat, pl->range_dev, s));
  return TTNET_OK;
}

// The vAlexnet block + Flatten (gate_va.hip), from the stem bits in x_rp[0]
int run_va_block(ttnet_plan *pl, const ttnet_plan::Lane &L, int n, hipStream_t s) {
  const MultiHead &mh = pl->blocks[0];
  TT_TIMED(pl, "va.block", s, launch_va_block(L.x_rp[0], mh.c1.table, mh.c2.table, mh.c3.table, L.va_y, n, s));
  TT_TIMED(pl, "va.flatten", s, launch_va_feat(L.va_y, L.feat, n, s));
  return TTNET_OK;
}

// One block of the full variant: direct float64 evaluation (gate_full.hip)
int run_full_block(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, hipStream_t s) {
  const MultiHead &mh = pl->blocks[i];
  const std::array<uint64_t *, 4> o64 = branch_rows(L, i);
  uint64_t *const c3_tmp = L.blk[i].c3_tmp;
  auto wts = [&](const BlockTT &b, const char *leaf) { return (const float *)pl->tensors[b.g.name + leaf].dev; };
  // a grouped 1x1 block on an H x W pixel grid: everything but its sources and its output
  auto pw_args = [&](const BlockTT &b, int H, int W) {
    FullPwArgs a{};
    a.n = n; a.H = H; a.W = W;
    a.groups = b.g.groups; a.cin = b.g.cin_g(); a.mid = b.g.mid_g(); a.cout = b.g.cout_g(); a.Cout = b.g.out_planes;
    a.Csrc = mh.C;
    a.w1 = wts(b, ".conv1.weight"); a.w2 = wts(b, ".conv2.weight");
    a.s1 = b.s1; a.t1 = b.t1; a.s2 = b.s2; a.t2 = b.t2;
    a.gel = pl->full_gel ? pl->full_gel + full_gelu_tables_elems() / 2 : nullptr;
    a.fix_count = L.full_fix; a.fix_list = L.full_fix ? L.full_fix + 64 : nullptr; a.range_flag = pl->range_dev;
    return a;
  };
  for (int br = 0; br < 2; ++br) {
    const BlockTT &b = br ? mh.c2 : mh.c1;
    FullDwArgs a{};
    a.n = n; a.C = mh.C; a.H = mh.H; a.W = mh.W;
    a.kh = b.g.kh; a.kw = b.g.kw; a.stride = b.g.stride; a.pad = b.g.pad;
    a.ho = (mh.H + 2 * a.pad - a.kh) / a.stride + 1;
    a.wo = (mh.W + 2 * a.pad - a.kw) / a.stride + 1;
    a.Ho = mh.Ho; a.pad_t = 0; a.pad_l = 0;          // out1 / out2 only ever get bottom / right zero padding
    a.x_rp = L.x_rp[i];
    a.w1 = wts(b, ".conv1.weight"); a.w2 = wts(b, ".conv2.weight");
    a.s1 = b.s1; a.t1 = b.t1; a.s2 = b.s2; a.t2 = b.t2;
    a.out = o64[br];
    a.gel = pl->full_gel;
    if (L.full_fix) {                                // (the list area is shared with the 1x1 blocks: launches are ordered)
      a.fix_count = L.full_fix;
      a.fix_list = L.full_fix + 64;
      a.fix_cap = (uint32_t)std::min<size_t>(pl->full_fix_cap, 0x7FFFFFFFu);
    }
    static const char *const kDw[2][4] = {{"full.conv1.f4", "full.conv1.f5", "full.conv1.f6", "full.conv1.f7"},
                                         {"full.conv2.f4", "full.conv2.f5", "full.conv2.f6", "full.conv2.f7"}};
    TT_TIMED(pl, kDw[br][std::min<size_t>(i, 3)], s, launch_full_dw(a, s));
  }
  {
    FullPwArgs a = pw_args(mh.c3, mh.H, mh.W);
    a.interleaved = 0; a.src[0] = L.x_rp[i];
    a.out_rp = c3_tmp; a.out_float = nullptr;
    static const char *const kC3[4] = {"full.conv3.f4", "full.conv3.f5", "full.conv3.f6", "full.conv3.f7"};
    TT_TIMED(pl, kC3[std::min<size_t>(i, 3)], s, launch_full_pw(a, s));
    TT_TIMED(pl, "full.maj3", s,
             launch_rp_majority(c3_tmp, o64[2], n, mh.C, mh.H, mh.W, mh.Ho, mh.off34, mh.off34, s));
    TT_TIMED(pl, "full.maj4", s,
             launch_rp_majority(L.x_rp[i], o64[3], n, mh.C, mh.H, mh.W, mh.Ho, mh.off34, mh.off34, s));
  }
  {
    FullPwArgs a = pw_args(mh.cf, mh.Ho, mh.Wo);
    a.interleaved = 1;
    for (int k = 0; k < 4; ++k) a.src[k] = o64[k];
    if (mh.last) {
      a.out_rp = nullptr; a.out_float = L.last_float;
      TT_TIMED(pl, "full.convf_last", s, launch_full_pw(a, s));
      TT_TIMED(pl, "full.pool", s, launch_full_pool_split(L.last_float, L.feat, n, mh.cf.g.out_planes, mh.Ho, mh.Wo, pl->range_dev, s));
    } else {
      a.out_rp = L.x_rp[i + 1]; a.out_float = nullptr;
      static const char *const kCf[4] = {"full.convf.f4", "full.convf.f5", "full.convf.f6", "full.convf.f7"};
      TT_TIMED(pl, kCf[std::min<size_t>(i, 3)], s, launch_full_pw(a, s));
    }
  }
  return TTNET_OK;
}

// The classifier's operands (finalize): BatchNorm1d folded, lin1's weights permuted to the feature order of the gate
// kernels (vAlexnet's features already come in the reference's Flatten order) and split into w1f, lin2's into w2f
int prepare_head(ttnet_plan *pl, hipStream_t s) {
  const Tensor &t1 = pl->tensors[pl->head + ".lin1.weight"], &t2 = pl->tensors[pl->head + ".lin2.weight"];
  std::vector<double> sc, sh;
  TT_TRY(fold_bn(pl, pl->head + ".BN2", sc, sh));
  std::vector<float> w;
  TT_TRY(fetch(t1, w));
  const float ws1 = weight_prescale(w.data(), w.size());
  for (double &v : sc) v /= (double)ws1 * ACT_PRESCALE;      // operand prescales (powers of two) out of lin1's result
  TT_TRY(upload_f32(pl->bn_scale, sc));
  TT_TRY(upload_f32(pl->bn_shift, sh));
  const float *w1 = (const float *)t1.dev;
  if (pl->path != GatePath::VAlexnet) {
    TT_TRY(launch_permute_lin1(w1, pl->w1p, pl->inter, pl->featC / 16, pl->featPP, s));
    w1 = pl->w1p;
  }
  TT_TRY(launch_split_to_frag(w1, pl->w1f, pl->inter, pl->fcsize, (pl->inter + 127) / 128 * 128, ws1, s));
  TT_TRY(fetch(t2, w));
  const float ws2 = weight_prescale(w.data(), w.size());
  pl->lin2_inv = 1.0f / (ws2 * ACT_PRESCALE);
  const int kpad = (pl->inter + 15) / 16 * 16;
  return launch_split_to_frag((const float *)t2.dev, pl->w2f, pl->n_classes, kpad, (pl->n_classes + 63) / 64 * 64, ws2, s, pl->inter,
                              pl->inter);
}

// Classifier_scale from the features in L.feat
int run_head(ttnet_plan *pl, const ttnet_plan::Lane &L, int n, float *logits, hipStream_t s) {
  const int polynomial = pl->path == GatePath::VAlexnet ? 0 : 1;
  const int s1 = gemm_f16x2_splits(n, pl->inter, pl->fcsize / 16);
  TT_TIMED(pl, "head.lin1", s, launch_gemm_f16x2(L.feat, pl->w1f, L.part, n, pl->inter, pl->fcsize, s1, s));
  TT_TIMED(pl, polynomial ? "head.bn_poly" : "head.bn", s,
           launch_head_mid(L.part, s1, pl->bn_scale, pl->bn_shift, L.mid_frag, n, pl->inter, polynomial, pl->range_dev, s));
  TT_TIMED(pl, "head.lin2", s,
           launch_lin2_f16x2(L.mid_frag, pl->w2f, (const float *)pl->tensors[pl->head + ".lin2.bias"].dev, pl->lin2_inv, logits, n,
                             pl->n_classes, pl->inter, s));
  return TTNET_OK;
}

// Blocks + head from the stem's output in L.x_rp[0]
int run_from_blocks(ttnet_plan *pl, ttnet_plan::Lane &L, int n, float *logits, hipStream_t s) {
  for (size_t i = 0; i < pl->blocks.size(); ++i) {
    switch (pl->path) {
      case GatePath::TwoLaunch: TT_TRY(run_two_launch_block(pl, L, i, n, s)); break;
      case GatePath::Fused: TT_TRY(run_fused_block(pl, L, i, n, s)); break;
      case GatePath::XSmall: TT_TRY(run_xs_block(pl, L, i, n, s)); break;
      case GatePath::Full: TT_TRY(run_full_block(pl, L, i, n, s)); break;
      case GatePath::VAlexnet: TT_TRY(run_va_block(pl, L, n, s)); break;
    }
  }
  TT_TRY(run_head(pl, L, n, logits, s));
  L.last_n = n;
  return TTNET_OK;
}

// The range flag is raised by a kernel, i.e. asynchronously: the forward that overflowed has already
// returned TTNET_OK.  Every later call on the plan fails until the flag is read (and cleared) with
// ttnet_plan_query("range_overflow"); ttnet_read_stage checks it after its own synchronisation.
int check_range(ttnet_plan *pl) {
  if (pl->range_host && *(volatile uint32_t *)pl->range_host) {
    set_error("an earlier forward on this plan met an activation outside the range of the fp16 x 2 operand split "
              "(|input| or |feature| >= 4094, or NaN): its logits are invalid; ttnet_plan_query(\"range_overflow\") "
              "reads and clears the flag");
    return TTNET_E_RANGE;
  }
  return TTNET_OK;
}

int check_ready(ttnet_plan *pl, const void *in, int64_t n, const void *out, const char *who = "ttnet_forward") {
  if (!pl || !in || !out) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  if (!pl->finalized) {
    set_error("%s before ttnet_plan_finalize", who);
    return TTNET_E_STATE;
  }
  if (n < 1 || n > pl->desc.max_batch) {
    set_error("batch %lld outside [1, max_batch=%d]", (long long)n, pl->desc.max_batch);
    return TTNET_E_INVALID;
  }
  return check_range(pl);
}

BlockTT *find_block(ttnet_plan *pl, const char *name) {
  for (BlockTT *b : all_block_tts(pl))
    if (b->g.name == name) return b;
  return nullptr;
}

// canonical index (pattern read MSB first over (c,kh,kw), TT_FHE_SMALL.py:330-334) of an
// internal index
inline uint32_t canonical_index(const BlockTT &b, uint32_t idx) {
  const int n = b.g.nbits();
  uint32_t ci = 0;
  for (int p = 0; p < n; ++p)
    if ((idx >> p) & 1u) ci |= 1u << (n - 1 - b.perm[p]);
  return ci;
}

// The Block_TT that ttnet_plan_get_table (get) / ttnet_plan_set_table names, whose host buffer must hold the table in
// the canonical order
int table_block(ttnet_plan *pl, const char *name, const void *host, size_t bytes, bool get, BlockTT **out) {
  if (!pl || !name || !host) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  BlockTT *b = find_block(pl, name);
  if (!b) {
    set_error("no Block_TT named %s", name);
    return TTNET_E_INVALID;
  }
  if (pl->path == GatePath::Full) {
    set_error("the full variant (fan-in 30) has no truth tables: 2^30 entries per output bit");
    return TTNET_E_UNSUPPORTED;
  }
  if (get && !pl->finalized) {
    set_error("get_table before finalize");
    return TTNET_E_STATE;
  }
  if (bytes != b->g.canonical_bytes()) {
    set_error("%s(%s): %s is %zu bytes, table is %zu", get ? "get_table" : "set_table", name, get ? "destination" : "source", bytes,
              b->g.canonical_bytes());
    return TTNET_E_INVALID;
  }
  *out = b;
  return TTNET_OK;
}

// Every entry of b's table between the internal layout (raw) and the canonical order (canon); store: canon -> raw
void walk_table(const BlockTT &b, void *raw, void *canon, bool store) {
  const BlockGeom &g = b.g;
  const size_t per = (size_t)1 << g.nbits(), entry_bytes = g.canonical_bytes() / g.entries();
  for (int grp = 0; grp < g.groups; ++grp)
    for (uint32_t idx = 0; idx < per; ++idx)
      table_entry(g, raw, grp, idx, (uint8_t *)canon + ((size_t)grp * per + canonical_index(b, idx)) * entry_bytes, store);
}

// Per-lane scratch of ttnet_table_usage_add and ttnet_care_misses, sized for max_batch (a lane that has its scratch keeps it)
int alloc_usage_scratch(ttnet_plan *pl, ttnet_plan::Lane &L) {
  if (L.u_br[0] || pl->path == GatePath::XSmall) return TTNET_OK;      // (x-small keeps everything as uint64 rows already)
  const size_t nb = (size_t)pl->desc.max_batch;
  size_t rows = 0, br = 0, tap = 0;
  for (size_t i = 0; i < pl->blocks.size(); ++i) {
    const MultiHead &mh = pl->blocks[i];
    if (i > 0) rows = std::max(rows, nb * mh.C * mh.H);
    br = std::max(br, nb * mh.C * mh.Ho);
    if (!mh.last) tap = std::max(tap, nb * (mh.C / 8) * mh.Ho * mh.Wo);
  }
  size_t *acc = &pl->scratch_bytes;
  for (int k = 0; k < 4; ++k) TT_TRY(dev_alloc(pl, &L.u_br[k], br, true, acc));
  if (pl->path == GatePath::Fused) {
    TT_TRY(dev_alloc(pl, &L.u_rows, rows, true, acc));
    TT_TRY(dev_alloc(pl, &L.u_tap, tap, true, acc));
  }
  return TTNET_OK;
}

// the lanes' scratch goes once neither the usage counters nor a care set need it
void free_usage_scratch(ttnet_plan *pl) {
  if (pl->usage_on || pl->care_on) return;
  for (auto &l : pl->lanes) {
    for (auto &p : l.u_br) { dev_free(pl, p); p = nullptr; }
    dev_free(pl, l.u_rows); l.u_rows = nullptr;
    dev_free(pl, l.u_tap); l.u_tap = nullptr;
  }
  pl->scratch_bytes = 0;
}

void free_usage(ttnet_plan *pl) {
  for (BlockTT *b : all_block_tts(pl)) {
    dev_free(pl, b->usage);
    b->usage = nullptr;
  }
  pl->usage_bytes = 0;
  pl->usage_on = false;
  free_usage_scratch(pl);
}

void free_care(ttnet_plan *pl) {
  for (BlockTT *b : all_block_tts(pl)) {
    dev_free(pl, b->care);
    b->care = nullptr;
  }
  pl->care_bytes = 0;
  pl->care_on = false;
  free_usage_scratch(pl);
}

// words of b's care bitmap
size_t care_words(const BlockTT &b) {
  return (size_t)b.g.groups * std::max<size_t>(1, ((size_t)1 << b.g.nbits()) / 32);
}

// TTNET_E_UNSUPPORTED for the variants that table usage and care sets do not serve
int check_usage_served(ttnet_plan *pl, const char *what) {
  if (pl->path == GatePath::Full) {
    set_error("the full variant (fan-in 30) has no truth tables: 2^30 entries per output bit");
    return TTNET_E_UNSUPPORTED;
  }
  if (pl->path == GatePath::VAlexnet) {
    set_error("%s is not built for the vAlexnet variant", what);
    return TTNET_E_UNSUPPORTED;
  }
  return TTNET_OK;
}

// The lane whose last forward ttnet_table_usage_add / ttnet_care_misses read
int usage_lane(ttnet_plan *pl, const char *who, int lane, const ttnet_plan::Lane **out) {
  if (lane < 0 || lane >= (int)pl->lanes.size()) {
    set_error("%s: lane %d but the plan has %d (ttnet_plan_set_lanes)", who, lane, (int)pl->lanes.size());
    return TTNET_E_INVALID;
  }
  if (pl->lanes[lane].last_n < 1) {
    set_error("%s: no forward has run on lane %d", who, lane);
    return TTNET_E_STATE;
  }
  *out = &pl->lanes[lane];
  return TTNET_OK;
}

int forward_eager(ttnet_plan *pl, ttnet_plan::Lane &L, const void *x_dev, bool u8, int64_t n, float *logits_dev, hipStream_t s) {
  pl->timing_used = 0;
  if (pl->path == GatePath::VAlexnet) {
    if (u8)
      TT_TIMED(pl, "va.stem_u8", s,
               launch_va_stem_u8((const uint8_t *)x_dev, pl->va_u8_tab, pl->va_scale, pl->va_shift, L.x_rp[0], (int)n, s));
    else
      TT_TIMED(pl, "va.stem", s,
               launch_va_stem((const float *)x_dev, (const float *)pl->tensors["features.0.weight"].dev,
                              (const float *)pl->tensors["features.0.bias"].dev, pl->va_scale, pl->va_shift, L.x_rp[0],
                              (int)n, s));
  } else {
    TT_TIMED(pl, "stem", s,
             launch_stem(x_dev, u8, pl->norm_tab, u8 ? pl->stem_wt_u8 : pl->stem_wt, u8 ? pl->stem_init_u8 : pl->stem_init, L.x_rp[0],
                         pl->path == GatePath::TwoLaunch ? L.x_cp[0] : nullptr, (int)n, pl->p, pl->range_dev, s,
                         part::stem_workgroups((int)pl->lanes.size(), u8, pl->path == GatePath::Full)));      // (half the CUs for float32 input with batches in flight)
  }
  return run_from_blocks(pl, L, (int)n, logits_dev, s);
}

// The forward is a fixed chain of ~11 launches whose host cost (~20 us each) equals the device
// time at batch 256, so from the third call with a given batch size on it is replayed as a
// hipGraph captured on a private stream.  Only two pointers change between calls: the input
// (argument 0 of the first kernel) and the logits (argument 4 of lin2, the last kernel); they
// are patched into the instantiated graph when they differ from the previous call.
constexpr int kLastKernelOutArg = 4, kLastKernelBatchArg = 5;      // lin2_f16x2_kernel(A, B, bias, inv, out, M, ..)

void drop_graph(ttnet_plan::GraphEntry &e) {
  if (e.exec) (void)hipGraphExecDestroy(e.exec);
  if (e.graph) (void)hipGraphDestroy(e.graph);
  e = ttnet_plan::GraphEntry{};
}

// Captured graphs bake in by-value kernel arguments derived from the weights (lin2's 1/prescale) and
// the device addresses of tables: whenever a tensor, a table or the finalized state changes they are
// all dropped (after a device synchronisation -- a replay may still be in flight) and re-captured
// from the third forward on.
int invalidate_graphs(ttnet_plan *pl) {
  bool any = false;
  for (auto &l : pl->lanes) any = any || !l.graphs.empty();
  if (any) TT_HIP(hipDeviceSynchronize());
  for (auto &l : pl->lanes) {
    for (auto &kv : l.graphs) {
      drop_graph(kv.second);
      pl->graph_drops++;
    }
    l.graphs.clear();
    l.eager_calls.clear();
  }
  return TTNET_OK;
}

void graphs_off(ttnet_plan *pl, const char *why) {
  pl->graphs_ok = false;
  pl->graph_off_reason = why;
  (void)hipGetLastError();
}

// Copy a kernel node's launch parameters into storage we own; arg_sizes: the kernel's own export of its argument sizes.
// (The arrays returned by hipGraphKernelNodeGetParams belong to the node: they are read once,
// here, and never handed back to the runtime.)
bool own_params(hipGraphNode_t node, int (*arg_sizes)(const int **), ttnet_plan::GraphEntry::Kernel &k) {
  const int *sizes = nullptr;
  const int nargs = arg_sizes(&sizes);
  hipGraphNodeType type;
  hipKernelNodeParams q{};
  if (nargs > (int)std::size(k.argv) || hipGraphNodeGetType(node, &type) != hipSuccess || type != hipGraphNodeTypeKernel ||
      hipGraphKernelNodeGetParams(node, &q) != hipSuccess || !q.kernelParams || q.extra)
    return false;
  for (int i = 0; i < nargs; ++i) {
    if (!q.kernelParams[i]) return false;
    k.argv[i] = 0;
    memcpy(&k.argv[i], q.kernelParams[i], (size_t)sizes[i]);
  }
  k.node = node;
  k.p = q;
  k.p.kernelParams = nullptr;          // (linked to k.args when an argument is patched)
  k.p.extra = nullptr;
  return true;
}

// Re-point argument `slot` of a captured kernel in the instantiated graph
bool patch_pointer(hipGraphExec_t exec, ttnet_plan::GraphEntry::Kernel &k, int slot, const void *ptr) {
  k.argv[slot] = (uint64_t)(uintptr_t)ptr;
  k.p.kernelParams = k.args;          // (the entry may have been moved since capture)
  for (size_t i = 0; i < std::size(k.args); ++i) k.args[i] = &k.argv[i];
  return hipGraphExecKernelNodeSetParams(exec, k.node, &k.p) == hipSuccess;
}

// *status: what forward_eager returned inside the capture (a caller error -- bad argument, range flag -- is reported to
// the caller as such and does not turn graph replay off for the plan; only a failure of the capture machinery does)
bool capture_forward(ttnet_plan *pl, ttnet_plan::Lane &L, const void *x_dev, bool u8, int64_t n, float *logits_dev, ttnet_plan::GraphEntry &e, int *status) {
  *status = TTNET_OK;
  if (!pl->cap_stream && hipStreamCreateWithFlags(&pl->cap_stream, hipStreamNonBlocking) != hipSuccess) return false;
  if (hipStreamBeginCapture(pl->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
  const int r = forward_eager(pl, L, x_dev, u8, n, logits_dev, pl->cap_stream);
  hipGraph_t g = nullptr;
  const hipError_t ee = hipStreamEndCapture(pl->cap_stream, &g);
  if (r != TTNET_OK || ee != hipSuccess || !g) {
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    *status = r;
    return false;
  }
  e.graph = g;
  if (hipGraphInstantiate(&e.exec, g, nullptr, nullptr, 0) != hipSuccess) return false;
  // a single chain: walk from the root to the leaf
  hipGraphNode_t node = nullptr;
  size_t cnt = 1;
  if (hipGraphGetRootNodes(g, &node, &cnt) != hipSuccess || cnt != 1) return false;
  const hipGraphNode_t first = node;
  for (int guard = 0; guard < 1000; ++guard) {
    size_t nd = 0;
    if (hipGraphNodeGetDependentNodes(node, nullptr, &nd) != hipSuccess) return false;
    if (nd == 0) break;
    if (nd != 1) return false;
    hipGraphNode_t next = nullptr;
    if (hipGraphNodeGetDependentNodes(node, &next, &nd) != hipSuccess) return false;
    node = next;
  }
  // the first kernel of the chain, by (path, input kind): its argument 0 is the input
  int (*const first_sizes)(const int **) =
      pl->path != GatePath::VAlexnet ? stem_kernel_arg_sizes : u8 ? va_stem_u8_kernel_arg_sizes : va_stem_kernel_arg_sizes;
  if (first == node || !own_params(first, first_sizes, e.first) ||
      !own_params(node, lin2_kernel_arg_sizes, e.last))
    return false;
  // the two slots that will be patched must hold exactly the pointers this capture ran with
  if (e.first.argv[0] != (uint64_t)(uintptr_t)x_dev || e.last.argv[kLastKernelOutArg] != (uint64_t)(uintptr_t)logits_dev ||
      e.last.argv[kLastKernelBatchArg] != (uint64_t)n)
    return false;
  e.x = x_dev;
  e.out = logits_dev;
  return true;
}

int forward_impl(ttnet_plan *pl, int lane, const void *x_dev, bool u8, int64_t n, float *logits_dev, void *stream) {
  TT_TRY(check_ready(pl, x_dev, n, logits_dev));
  // The input contract of ttnet.h (16-byte aligned float32, 4-byte aligned uint8: the stem reads it with 16 / 12-byte
  // buffer loads) is checked HERE, in front of the replay, the capture and the plain path alike: a cached graph
  // only has its first argument re-pointed and would otherwise take any pointer.
  if ((pl->path != GatePath::VAlexnet || u8) && ((uintptr_t)x_dev & (u8 ? 3u : 15u)) != 0) {
    set_error("forward: the input must be %d-byte aligned", u8 ? 4 : 16);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)logits_dev & 3u) != 0) {
    set_error("forward: the logits buffer must be 4-byte aligned");
    return TTNET_E_INVALID;
  }
  if (lane < 0 || lane >= (int)pl->lanes.size()) {
    set_error("forward: lane %d but the plan has %d (ttnet_plan_set_lanes)", lane, (int)pl->lanes.size());
    return TTNET_E_INVALID;
  }
  pl->last_lane = lane;
  ttnet_plan::Lane &L = pl->lanes[lane];
  hipStream_t s = (hipStream_t)stream;
  if (pl->profiling || !pl->graphs_ok) return forward_eager(pl, L, x_dev, u8, n, logits_dev, s);
  const int64_t key = 2 * n + (u8 ? 1 : 0);               // one graph per (batch size, input kind)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (s && hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
    return forward_eager(pl, L, x_dev, u8, n, logits_dev, s);   // the caller is capturing us into a graph of their own
  auto it = L.graphs.find(key);
  if (it == L.graphs.end()) {
    if (++L.eager_calls[key] <= 2) return forward_eager(pl, L, x_dev, u8, n, logits_dev, s);   // warm: attributes, lazy module load
    ttnet_plan::GraphEntry e;
    int cap_status = TTNET_OK;
    if (!capture_forward(pl, L, x_dev, u8, n, logits_dev, e, &cap_status)) {
      drop_graph(e);
      if (cap_status != TTNET_OK) {          // the forward itself refused the call: the caller's error, graphs stay on
        --L.eager_calls[key];
        return cap_status;
      }
      graphs_off(pl, "capture or instantiation of the forward failed");   // stay on plain launches
      return forward_eager(pl, L, x_dev, u8, n, logits_dev, s);
    }
    pl->graph_captures++;
    if (L.graphs.size() >= 8) {                                // bound the cache: drop the smallest batch size
      // its last replay may still be running on a stream this call knows nothing about
      TT_HIP(hipDeviceSynchronize());
      drop_graph(L.graphs.begin()->second);
      L.graphs.erase(L.graphs.begin());
      pl->graph_drops++;
    }
    it = L.graphs.emplace(key, e).first;
  }
  ttnet_plan::GraphEntry &e = it->second;
  bool ok = true;
  if (e.x != x_dev) {
    ok = patch_pointer(e.exec, e.first, 0, x_dev);
    e.x = x_dev;
  }
  if (ok && e.out != logits_dev) {
    ok = patch_pointer(e.exec, e.last, kLastKernelOutArg, logits_dev);
    e.out = logits_dev;
  }
  if (ok) ok = hipGraphLaunch(e.exec, s) == hipSuccess;
  if (!ok) {
    drop_graph(e);
    L.graphs.erase(it);
    graphs_off(pl, "hipGraphExecKernelNodeSetParams / hipGraphLaunch failed");
    return forward_eager(pl, L, x_dev, u8, n, logits_dev, s);
  }
  L.last_n = n;
  pl->timing_used = 0;
  pl->graph_replays++;
  return TTNET_OK;
}

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

}  // namespace

extern "C" {

const char *ttnet_last_error(void) { return g_err; }
const char *ttnet_version(void) { return "ttnet-mi355x 0.1 (gfx950)"; }

int ttnet_plan_create(const ttnet_net_desc *desc, int device, ttnet_plan **out) {
  if (!desc || !out) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
    set_error("no HIP device: libttnet has no CPU path");
    return TTNET_E_HIP;
  }
  if (device < 0 || device >= count) {
    set_error("device %d out of range (%d devices)", device, count);
    return TTNET_E_INVALID;
  }
  TT_HIP(hipSetDevice(device));
  ttnet_plan *pl = new ttnet_plan();
  pl->desc = *desc;
  pl->device = device;
  int st = build_geometry(pl);
  if (st == TTNET_OK) st = allocate(pl);
  if (st != TTNET_OK) {
    ttnet_plan_destroy(pl);
    return st;
  }
  *out = pl;
  return TTNET_OK;
}

int ttnet_plan_set_tensor(ttnet_plan *pl, const char *key, const void *ptr, const int64_t *shape, int ndim,
                          int dtype, int on_device) {
  if (!pl || !key || !ptr || (ndim > 0 && !shape)) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  std::string k(key);
  if (k.rfind("module.", 0) == 0) k = k.substr(7);   // DataParallel / DDP checkpoints (main.py:181-192)
  auto it = pl->tensors.find(k);
  if (it == pl->tensors.end()) {
    set_error("unexpected key in state_dict: %s", key);
    return TTNET_E_INVALID;
  }
  Tensor &t = it->second;
  bool ok = (dtype == t.dtype) && (ndim == (int)t.shape.size());
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == t.shape[i];
  if (!ok) {
    set_error("size mismatch for %s", key);
    return TTNET_E_INVALID;
  }
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(invalidate_graphs(pl));
  TT_HIP(hipMemcpy(t.dev, ptr, t.bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  t.set = true;
  pl->finalized = false;
  drop_certify(pl);
  // new parameters for a Block_TT invalidate a table injected with ttnet_plan_set_table
  for (BlockTT *b : all_block_tts(pl))
    if (k.compare(0, b->g.name.size() + 1, b->g.name + ".") == 0) b->user_table = false;
  return TTNET_OK;
}

int ttnet_plan_finalize(ttnet_plan *pl, void *stream) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(invalidate_graphs(pl));
  for (auto &k : pl->key_order) {
    const Tensor &t = pl->tensors[k];
    if (t.required && !t.set) {
      set_error("missing key in state_dict: %s", k.c_str());
      return TTNET_E_STATE;
    }
  }
  if (pl->path == GatePath::VAlexnet) {
    std::vector<double> sc, sh;
    TT_TRY(fold_bn(pl, "features.2", sc, sh));
    TT_TRY(upload_f32(pl->va_scale, sc));
    TT_TRY(upload_f32(pl->va_shift, sh));
    TT_TRY(prepare_va_stem_u8(pl));
  } else {
    TT_TRY(prepare_stem(pl));
    TT_TRY(prepare_stem_u8(pl));
  }
  for (auto &mh : pl->blocks) {
    for (BlockTT *b : {&mh.c1, &mh.c2, &mh.c3, &mh.cf})
      if (!b->g.name.empty()) TT_TRY(build_table(pl, *b, s));
    if (pl->path == GatePath::Fused) TT_TRY(launch_fused_images(mh.c1.table, mh.c2.table, mh.c3.table, mh.C, mh.img_dw, mh.img_c3, s));
  }
  TT_TRY(prepare_head(pl, s));
  TT_HIP(hipStreamSynchronize(s));
  TT_TRY(read_near_ties(pl));
  pl->finalized = true;
  return TTNET_OK;
}

int ttnet_plan_set_lanes(ttnet_plan *pl, int lanes) {
  if (!pl || lanes < 1 || lanes > 16) {
    set_error("set_lanes: %d outside [1,16]", lanes);
    return TTNET_E_INVALID;
  }
  (void)hipSetDevice(pl->device);
  if ((int)pl->lanes.size() < lanes && pl->lanes.size() == 1) TT_TRY(invalidate_graphs(pl));      // (the stem's grid depends on lanes >= 2)
  while ((int)pl->lanes.size() < lanes) {
    const int r = alloc_workspace(pl, pl->lanes.emplace_back());
    if (r != TTNET_OK) {
      pl->lanes.pop_back();                             // (what it did allocate stays owned by the plan)
      return r;
    }
  }
  if (pl->usage_on || pl->care_on)
    for (auto &l : pl->lanes) TT_TRY(alloc_usage_scratch(pl, l));     // (lanes that have theirs keep it)
  return TTNET_OK;
}

int ttnet_plan_table_usage_enable(ttnet_plan *pl, int enabled) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  TT_TRY(check_usage_served(pl, "table usage"));
  TT_HIP(hipSetDevice(pl->device));
  if ((enabled != 0) == pl->usage_on) return TTNET_OK;
  TT_HIP(hipDeviceSynchronize());
  if (!enabled) {
    free_usage(pl);
    return TTNET_OK;
  }
  if (const char *e = getenv("TTNET_USAGE_SCHEME"))      // measurements: "plain" / "merged" for every table shape
    pl->usage_scheme_dw = pl->usage_scheme_pw = std::string(e) == "plain" ? kUsagePlain : kUsageMerged;
  int r = TTNET_OK;
  for (BlockTT *b : all_block_tts(pl)) {
    if (r == TTNET_OK) r = dev_alloc(pl, &b->usage, b->g.entries(), true, &pl->usage_bytes);
  }
  for (auto &l : pl->lanes)
    if (r == TTNET_OK) r = alloc_usage_scratch(pl, l);
  if (r != TTNET_OK) {
    free_usage(pl);
    return r;
  }
  pl->usage_on = true;
  return TTNET_OK;
}

int ttnet_plan_table_usage_reset(ttnet_plan *pl, void *stream) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  if (!pl->usage_on) {
    set_error("table_usage_reset before ttnet_plan_table_usage_enable");
    return TTNET_E_STATE;
  }
  for (BlockTT *b : all_block_tts(pl))
    TT_HIP(hipMemsetAsync(b->usage, 0, b->g.entries() * sizeof(int64_t), (hipStream_t)stream));
  return TTNET_OK;
}

int ttnet_table_usage_add(ttnet_plan *pl, int lane, void *stream) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  if (!pl->usage_on) {
    set_error("table_usage_add before ttnet_plan_table_usage_enable");
    return TTNET_E_STATE;
  }
  const ttnet_plan::Lane *lp = nullptr;
  TT_TRY(usage_lane(pl, "table_usage_add", lane, &lp));
  const ttnet_plan::Lane &L = *lp;
  const int n = (int)L.last_n;
  hipStream_t s = (hipStream_t)stream;
  for (size_t i = 0; i < pl->blocks.size(); ++i) {
    const MultiHead &mh = pl->blocks[i];
    const uint64_t *xin = nullptr;
    TT_TRY(block_input_rows(pl, L, i, n, L.u_rows, "usage.prep", s, &xin));
    for (const BlockTT *b : {&mh.c1, &mh.c2}) {
      const BlockGeom &g = b->g;
      const int ho = (mh.H + 2 * g.pad - g.kh) / g.stride + 1, wo = (mh.W + 2 * g.pad - g.kw) / g.stride + 1;
      TT_TIMED(pl, "usage.dw", s,
               launch_usage_dw(xin, n, mh.C, mh.H, mh.W, ho, wo, g.kh, g.kw, g.stride, g.pad, b->usage, pl->usage_scheme_dw, s));
    }
    TT_TIMED(pl, "usage.conv3", s,
             launch_usage_pw(&xin, 1, n, mh.C, mh.c3.g.groups, mh.c3.g.cin_g(), mh.H, mh.W, mh.c3.usage, pl->usage_scheme_pw, s));
    // the four branch tensors after their padding (a non-last fused block is run again once, not once per branch)
    const uint32_t *dwords = nullptr;
    if (pl->path == GatePath::Fused) TT_TRY(fused_branch_dwords(pl, L, i, n, L.u_tap, "usage.tap", s, &dwords));
    const uint64_t *br[4];
    for (int k = 0; k < 4; ++k) TT_TRY(branch_as_rows(pl, L, i, k, n, dwords, L.u_br[k], "usage.prep", s, &br[k]));
    TT_TIMED(pl, "usage.convf", s,
             launch_usage_pw(br, 4, n, mh.C, mh.cf.g.groups, mh.cf.g.cin_g(), mh.Ho, mh.Wo, mh.cf.usage, pl->usage_scheme_pw, s));
  }
  return TTNET_OK;
}

int ttnet_plan_get_table_usage(ttnet_plan *pl, const char *name, int64_t *dst_host, size_t dst_bytes) {
  if (!pl || !name || !dst_host) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  if (!pl->usage_on) {
    set_error("get_table_usage before ttnet_plan_table_usage_enable");
    return TTNET_E_STATE;
  }
  BlockTT *b = find_block(pl, name);
  if (!b) {
    set_error("no Block_TT named %s", name);
    return TTNET_E_INVALID;
  }
  const size_t need = b->g.entries() * sizeof(int64_t);
  if (dst_bytes != need) {
    set_error("get_table_usage(%s): destination is %zu bytes, the counters are %zu", name, dst_bytes, need);
    return TTNET_E_INVALID;
  }
  TT_HIP(hipSetDevice(pl->device));
  TT_HIP(hipDeviceSynchronize());
  TT_HIP(hipMemcpy(dst_host, b->usage, need, hipMemcpyDeviceToHost));
  return TTNET_OK;
}

int ttnet_plan_set_care(ttnet_plan *pl, const char *name, const uint32_t *bits_host, size_t bytes) {
  if (!pl || !name) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  TT_TRY(check_usage_served(pl, "the care set"));
  BlockTT *b = find_block(pl, name);
  if (!b) {
    set_error("no Block_TT named %s", name);
    return TTNET_E_INVALID;
  }
  const size_t words = care_words(*b);
  if (bits_host && bytes != words * sizeof(uint32_t)) {
    set_error("set_care(%s): source is %zu bytes, the bitmap is %zu", name, bytes, words * sizeof(uint32_t));
    return TTNET_E_INVALID;
  }
  TT_HIP(hipSetDevice(pl->device));
  TT_HIP(hipDeviceSynchronize());                      // no care_misses may be reading the bitmap that is replaced
  if (!bits_host) {
    if (b->care) pl->care_bytes -= std::max<size_t>(words * sizeof(uint32_t), 16);
    dev_free(pl, b->care);
    b->care = nullptr;
    return TTNET_OK;
  }
  const bool was_on = pl->care_on;
  pl->care_on = true;
  int r = TTNET_OK;
  for (auto &l : pl->lanes)
    if (r == TTNET_OK) r = alloc_usage_scratch(pl, l);
  if (r == TTNET_OK && !b->care) r = dev_alloc(pl, &b->care, words, false, &pl->care_bytes);
  if (r != TTNET_OK) {
    if (!was_on) free_care(pl);
    return r;
  }
  TT_HIP(hipMemcpy(b->care, bits_host, bytes, hipMemcpyHostToDevice));
  return TTNET_OK;
}

int ttnet_plan_clear_care(ttnet_plan *pl) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  if (!pl->care_on) return TTNET_OK;
  TT_HIP(hipSetDevice(pl->device));
  TT_HIP(hipDeviceSynchronize());
  free_care(pl);
  return TTNET_OK;
}

int ttnet_care_misses(ttnet_plan *pl, int lane, int32_t *rows_dev, void *stream) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  if (!pl->care_on) {
    set_error("care_misses before ttnet_plan_set_care");
    return TTNET_E_STATE;
  }
  if (!rows_dev || ((uintptr_t)rows_dev & 3)) {
    set_error("care_misses: rows_dev is null or not 4-byte aligned");
    return TTNET_E_INVALID;
  }
  const ttnet_plan::Lane *lp = nullptr;
  TT_TRY(usage_lane(pl, "care_misses", lane, &lp));
  const ttnet_plan::Lane &L = *lp;
  const int n = (int)L.last_n;
  const int nb = (int)pl->blocks.size() * 4;           // row length: the Block_TTs in the order of all_block_tts
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipMemsetAsync(rows_dev, 0, (size_t)n * nb * sizeof(int32_t), s));
  for (size_t i = 0; i < pl->blocks.size(); ++i) {
    const MultiHead &mh = pl->blocks[i];
    int32_t *rows = rows_dev + 4 * i;                  // this block's four columns
    if (mh.c1.care || mh.c2.care || mh.c3.care) {
      const uint64_t *xin = nullptr;
      TT_TRY(block_input_rows(pl, L, i, n, L.u_rows, "care.prep", s, &xin));
      int col = 0;
      for (const BlockTT *b : {&mh.c1, &mh.c2}) {
        const BlockGeom &g = b->g;
        const int ho = (mh.H + 2 * g.pad - g.kh) / g.stride + 1, wo = (mh.W + 2 * g.pad - g.kw) / g.stride + 1;
        if (b->care)
          TT_TIMED(pl, "care.dw", s,
                   launch_care_dw(xin, n, mh.C, mh.H, mh.W, ho, wo, g.kh, g.kw, g.stride, g.pad, b->care, rows + col, nb, s));
        ++col;
      }
      if (mh.c3.care)
        TT_TIMED(pl, "care.conv3", s,
                 launch_care_pw(&xin, 1, n, mh.C, mh.c3.g.groups, mh.c3.g.cin_g(), mh.H, mh.W, mh.c3.care, rows + 2, nb, s));
    }
    if (!mh.cf.care) continue;
    const uint32_t *dwords = nullptr;
    if (pl->path == GatePath::Fused) TT_TRY(fused_branch_dwords(pl, L, i, n, L.u_tap, "care.tap", s, &dwords));
    const uint64_t *br[4];
    for (int k = 0; k < 4; ++k) TT_TRY(branch_as_rows(pl, L, i, k, n, dwords, L.u_br[k], "care.prep", s, &br[k]));
    TT_TIMED(pl, "care.convf", s,
             launch_care_pw(br, 4, n, mh.C, mh.cf.g.groups, mh.cf.g.cin_g(), mh.Ho, mh.Wo, mh.cf.care, rows + 3, nb, s));
  }
  return TTNET_OK;
}

int ttnet_forward_lane(ttnet_plan *pl, int lane, const float *x_dev, int64_t n, float *logits_dev, void *stream) {
  return forward_impl(pl, lane, x_dev, false, n, logits_dev, stream);
}

int ttnet_forward(ttnet_plan *pl, const float *x_dev, int64_t n, float *logits_dev, void *stream) {
  return forward_impl(pl, 0, x_dev, false, n, logits_dev, stream);
}

int ttnet_forward_u8(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, int64_t n, float *logits_dev, void *stream) {
  return forward_impl(pl, lane, x_nhwc_dev, true, n, logits_dev, stream);
}

int ttnet_plan_set_input_norm(ttnet_plan *pl, const float *mean3, const float *std3) {
  if (!pl || !mean3 || !std3) {
    set_error("set_input_norm: null argument");
    return TTNET_E_INVALID;
  }
  for (int c = 0; c < 3; ++c)
    if (!(std3[c] > 0.f)) {                            // (refused whole: the plan keeps the constants it had)
      set_error("set_input_norm: std[%d] = %g", c, (double)std3[c]);
      return TTNET_E_INVALID;
    }
  std::copy(mean3, mean3 + 3, pl->in_mean);
  std::copy(std3, std3 + 3, pl->in_std);
  (void)hipSetDevice(pl->device);
  TT_TRY(invalidate_graphs(pl));                       // as for a new tensor: what was captured ran with the old constants
  if (pl->cert.ready) {
    TT_HIP(hipDeviceSynchronize());
    drop_certify(pl);                                  // (the slack of the stem bounds depends on the constants)
  }
  if (!pl->finalized) return TTNET_OK;                 // (finalize folds them into the uint8 stem's weights)
  TT_HIP(hipDeviceSynchronize());                      // no forward may be reading the buffers that are rewritten in place
  return pl->path == GatePath::VAlexnet ? prepare_va_stem_u8(pl) : prepare_stem_u8(pl);
}

// what the three certificate entries share: the variant, the plan's state, the arguments they all take, A / c0 / slack, the
// lane's planes; then the argument block of the stages, with the box [x, x_hi] or x +- eps
static int certify_begin(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, const uint8_t *x_hi_dev, int64_t n, const int32_t *classes_dev,
                         double eps, int enum_bits, double min_margin, void *rows_dev, const void *second_out, bool needs_second,
                         const char *bad_args, const char *who, hipStream_t s, CertifyArgs &a) {
  if (pl && pl->path != GatePath::VAlexnet) {
    set_error("certify: only the vAlexnet variant is served: the certificate needs an affine head (no polynomial, no float last "
              "block) and truth tables of at most 8 inputs");
    return TTNET_E_UNSUPPORTED;
  }
  TT_TRY(check_ready(pl, x_nhwc_dev, n, rows_dev, who));
  if (!classes_dev || (needs_second && !(x_hi_dev ? (const void *)x_hi_dev : second_out))) {   // (box: the second image; patch: the map)
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  if (bad_args) {                                      // what only one entry takes, judged by it and reported in this order
    set_error("%s", bad_args);
    return TTNET_E_INVALID;
  }
  if (!(eps >= 0.0) || !std::isfinite(eps)) {
    set_error("certify: eps = %g (finite, >= 0)", eps);
    return TTNET_E_INVALID;
  }
  if (enum_bits < 0 || enum_bits > 12 || std::isnan(min_margin)) {
    set_error("certify: enum_bits = %d (0..12), min_margin = %g", enum_bits, min_margin);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)x_nhwc_dev & 3u) || ((uintptr_t)x_hi_dev & 3u) || ((uintptr_t)classes_dev & 3u) || ((uintptr_t)rows_dev & 7u) ||
      ((uintptr_t)second_out & 7u)) {
    set_error("certify: the images and classes must be 4-byte aligned, the records and planes 8-byte aligned");
    return TTNET_E_INVALID;
  }
  if (lane < 0 || lane >= (int)pl->lanes.size()) {
    set_error("certify: lane %d but the plan has %d (ttnet_plan_set_lanes)", lane, (int)pl->lanes.size());
    return TTNET_E_INVALID;
  }
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(prepare_certify(pl, s));
  ttnet_plan::Lane &L = pl->lanes[lane];
  const size_t nb = (size_t)pl->desc.max_batch, stem_w = va::kStemRows, feat_w = va::kFeatRows;
  if (!L.cert_planes) TT_TRY(dev_alloc(pl, &L.cert_planes, nb * (2 * (stem_w + feat_w) + va::kClasses), false));
  const MultiHead &mh = pl->blocks[0];
  a = CertifyArgs{};
  a.n = (int)n;
  a.x = x_nhwc_dev;
  a.x_hi = x_hi_dev;
  a.classes = classes_dev;
  for (int c = 0; c < 3; ++c) {
    a.norm.a[c] = 1.0 / (255.0 * (double)pl->in_std[c]);
    a.norm.off[c] = 255.0 * (double)pl->in_mean[c];
  }
  a.eps = eps;
  a.min_margin = min_margin;
  a.enum_bits = enum_bits;
  a.w = (const float *)pl->tensors["features.0.weight"].dev;
  a.bias = (const float *)pl->tensors["features.0.bias"].dev;
  a.stem_bn = pl->cert.stem_bn;
  a.slack = pl->cert.slack;
  a.t1 = (const uint32_t *)mh.c1.table;
  a.t2 = (const uint32_t *)mh.c2.table;
  a.t3 = (const uint8_t *)mh.c3.table;
  a.t3w = pl->cert.t3w;
  a.A = pl->cert.A;
  a.c0 = pl->cert.c0;
  a.stem_lo = L.cert_planes;
  a.stem_hi = a.stem_lo + nb * stem_w;
  a.feat_lo = a.stem_hi + nb * stem_w;
  a.feat_hi = a.feat_lo + nb * feat_w;
  a.sums = (double *)(a.feat_hi + nb * feat_w);
  a.rows = rows_dev;
  return TTNET_OK;
}

// the four stages on `s`, then the planes [stem lo][stem hi][feature lo][feature hi], each for n images
static int certify_run(ttnet_plan *pl, const CertifyArgs &a, uint64_t *planes_dev, hipStream_t s) {
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

int ttnet_certify_u8(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, double eps,
                     int enum_bits, double min_margin, void *rows_dev, uint64_t *planes_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  CertifyArgs a;
  TT_TRY(certify_begin(pl, lane, x_nhwc_dev, nullptr, n, classes_dev, eps, enum_bits, min_margin, rows_dev, planes_dev, false, nullptr, "ttnet_certify_u8", s, a));
  return certify_run(pl, a, planes_dev, s);
}

int ttnet_certify_box_u8(ttnet_plan *pl, int lane, const uint8_t *lo_nhwc_dev, const uint8_t *hi_nhwc_dev, int64_t n,
                         const int32_t *classes_dev, int enum_bits, double min_margin, void *rows_dev, uint64_t *planes_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  CertifyArgs a;
  TT_TRY(certify_begin(pl, lane, lo_nhwc_dev, hi_nhwc_dev, n, classes_dev, 0.0, enum_bits, min_margin, rows_dev, planes_dev, true, nullptr, "ttnet_certify_box_u8", s, a));
  return certify_run(pl, a, planes_dev, s);
}

int ttnet_certify_patch_u8(ttnet_plan *pl, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, int patch_h,
                           int patch_w, int stride, int amp, int enum_bits, double min_margin, void *rows_dev, void *map_dev, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  PatchArgs p{};
  char bad[160] = "";                                 // (the variant and the plan's state are judged first, as everywhere)
  if (patch_h < 1 || patch_h > va::kPatchMax || patch_w < 1 || patch_w > va::kPatchMax || stride < 1 || stride > 32 || amp < 1 || amp > 255)
    snprintf(bad, sizeof bad, "certify_patch: patch %d x %d (1..8 each), stride %d (1..32), amp %d (1..255)", patch_h, patch_w, stride, amp);
  TT_TRY(certify_begin(pl, lane, x_nhwc_dev, nullptr, n, classes_dev, 0.0, enum_bits, min_margin, rows_dev, map_dev, true, bad[0] ? bad : nullptr,
                       "ttnet_certify_patch_u8", s, p.clean));
  ttnet_plan::Lane &L = pl->lanes[lane];
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
  p.map = map_dev;
  p.rows = rows_dev;
  pl->timing_used = 0;
  TT_TIMED(pl, "patch.base", s, launch_certify_patch(p, kPatchBase, s));
  TT_TIMED(pl, "patch.sweep", s, launch_certify_patch(p, kPatchSweep, s));
  return TTNET_OK;
}

// what the two attack entries share: the variant, the plan's state and the batch size
static int attack_ready(ttnet_plan *pl, const void *a, int64_t n, const void *b, const char *who) {
  if (pl && pl->path != GatePath::VAlexnet) {
    set_error("%s: only the vAlexnet variant is served: the search needs the certificate's stem planes, an affine head and truth "
              "tables of at most 8 inputs", who);
    return TTNET_E_UNSUPPORTED;
  }
  return check_ready(pl, a, n, b, who);
}

int ttnet_attack_propose_u8(ttnet_plan *pl, int lane, const uint8_t *x0_dev, const uint8_t *xcur_dev, int64_t n,
                            const int32_t *classes_dev, const int32_t *worst_dev, const uint64_t *stem_planes_dev, int eps_levels,
                            const int32_t *active_dev, uint8_t *cand_dev, double *gains_dev, void *stream) {
  TT_TRY(attack_ready(pl, x0_dev, n, cand_dev, "ttnet_attack_propose_u8"));
  if (!xcur_dev || !classes_dev || !worst_dev || !stem_planes_dev || !active_dev) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  if (eps_levels < 0 || eps_levels > 64) {
    set_error("attack_propose: eps_levels = %d (0..64)", eps_levels);
    return TTNET_E_INVALID;
  }
  if ((((uintptr_t)x0_dev | (uintptr_t)xcur_dev | (uintptr_t)classes_dev | (uintptr_t)worst_dev | (uintptr_t)active_dev | (uintptr_t)cand_dev) & 3u) ||
      (((uintptr_t)stem_planes_dev | (uintptr_t)gains_dev) & 7u)) {
    set_error("attack_propose: the images, classes, runner-ups, flags and candidates must be 4-byte aligned, the planes and gains 8-byte aligned");
    return TTNET_E_INVALID;
  }
  if (lane < 0 || lane >= (int)pl->lanes.size()) {
    set_error("attack_propose: lane %d but the plan has %d (ttnet_plan_set_lanes)", lane, (int)pl->lanes.size());
    return TTNET_E_INVALID;
  }
  ttnet_plan::Lane &L = pl->lanes[lane];
  if (L.last_n != n) {
    set_error("attack_propose: n=%lld but the last forward on lane %d ran %lld images", (long long)n, lane, (long long)L.last_n);
    return TTNET_E_STATE;
  }
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(prepare_certify(pl, s));
  const MultiHead &mh = pl->blocks[0];
  AttackProposeArgs a{};
  a.n = (int)n;
  a.levels = eps_levels;
  a.x0 = x0_dev;
  a.xcur = xcur_dev;
  a.classes = classes_dev;
  a.worst = worst_dev;
  a.active = active_dev;
  a.stem = L.x_rp[0];
  a.feat = L.va_y;
  a.plane_lo = stem_planes_dev;
  a.plane_hi = stem_planes_dev + (size_t)n * va::kStemRows;
  a.t1 = (const uint32_t *)mh.c1.table;
  a.t2 = (const uint32_t *)mh.c2.table;
  a.t3w = pl->cert.t3w;
  a.A = pl->cert.A;
  a.bn_scale = pl->cert.stem_bn;
  a.wsum = pl->cert.wsum;
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
  if (!classes_dev || !x0_dev || !xcur_dev || !rows_dev || !worst_dev || !active_dev) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  if (n_cand < 1 || n_cand > 8 || round < 0 || std::isnan(min_margin)) {
    set_error("attack_select: n_cand = %d (1..8), round = %d (>= 0), min_margin = %g", n_cand, round, min_margin);
    return TTNET_E_INVALID;
  }
  if ((((uintptr_t)cand_dev | (uintptr_t)logits_dev | (uintptr_t)classes_dev | (uintptr_t)x0_dev | (uintptr_t)xcur_dev | (uintptr_t)worst_dev |
        (uintptr_t)active_dev) & 3u) || ((uintptr_t)rows_dev & 7u)) {
    set_error("attack_select: the images, logits, classes, runner-ups and flags must be 4-byte aligned, the records 8-byte aligned");
    return TTNET_E_INVALID;
  }
  if (xcur_dev == cand_dev || xcur_dev == x0_dev) {
    set_error("attack_select: xcur_dev must be a buffer of its own");
    return TTNET_E_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  pl->timing_used = 0;
  TT_TIMED(pl, "attack.select", s,
           launch_attack_select(cand_dev, logits_dev, (int)n, n_cand, classes_dev, (float)min_margin, x0_dev, xcur_dev, rows_dev, worst_dev,
                                active_dev, round, s));
  return TTNET_OK;
}

int ttnet_forward_from_stem_bits(ttnet_plan *pl, const uint64_t *rows_dev, int64_t n, float *logits_dev,
                                 void *stream) {
  TT_TRY(check_ready(pl, rows_dev, n, logits_dev));
  hipStream_t s = (hipStream_t)stream;
  pl->timing_used = 0;
  ttnet_plan::Lane &L = pl->lanes[pl->last_lane];
  const MultiHead &b0 = pl->blocks[0];
  TT_HIP(hipMemcpyAsync(L.x_rp[0], rows_dev, (size_t)n * b0.C * b0.H * 8, hipMemcpyDeviceToDevice, s));
  if (pl->path == GatePath::TwoLaunch) TT_TRY(launch_rp_to_cp(L.x_rp[0], L.x_cp[0], (int)n, b0.C, b0.H, b0.W, s));
  return run_from_blocks(pl, L, (int)n, logits_dev, s);
}

int ttnet_read_stage(ttnet_plan *pl, const char *stage, int64_t n, void *dst, size_t dst_bytes, int on_device,
                     void *stream) {
  if (!pl || !stage || !dst) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  const ttnet_plan::Lane &L = pl->lanes[pl->last_lane];
  if (n < 1 || n > L.last_n) {
    set_error("read_stage: n=%lld but the last forward ran %lld images", (long long)n, (long long)L.last_n);
    return TTNET_E_STATE;
  }
  hipStream_t s = (hipStream_t)stream;
  const std::string st(stage);
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  auto copy_out = [&](const void *src, size_t bytes) -> int {
    if (dst_bytes != bytes) {
      set_error("read_stage(%s): destination is %zu bytes, stage is %zu", stage, dst_bytes, bytes);
      return TTNET_E_INVALID;
    }
    TT_HIP(hipMemcpyAsync(dst, src, bytes, kind, s));
    TT_HIP(hipStreamSynchronize(s));
    return check_range(pl);
  };
  // a stage kept in another layout is converted to the ABI's into this temporary (copy_out synchronises before it goes)
  struct Scratch {
    void *p = nullptr;
    ~Scratch() { (void)hipFree(p); }
  } tmp;
  const GatePath path = pl->path;
  if (st == "flatten") {
    const size_t bytes = (size_t)n * pl->fcsize * 4;
    TT_HIP(hipMalloc(&tmp.p, bytes));
    TT_TRY(path == GatePath::VAlexnet ? launch_va_frag_to_flat(L.feat, (float *)tmp.p, (int)n, s)
                                      : launch_frag_to_reference_order(L.feat, (float *)tmp.p, (int)n, pl->featC / 16, pl->featPP, s));
    return copy_out(tmp.p, bytes);
  }
  if (path == GatePath::VAlexnet) {
    if (st == "features.4") return copy_out(L.x_rp[0], (size_t)n * va::kStemRows * 8);
    if (st == "features.5") return copy_out(L.va_y, (size_t)n * va::kFeatRows * 8);
    set_error("unknown stage %s", stage);
    return TTNET_E_INVALID;
  }
  const uint64_t *rows = nullptr;
  for (size_t i = 0; i < pl->blocks.size(); ++i) {
    const MultiHead &mh = pl->blocks[i];
    const std::string in_name = i == 0 ? std::string("features.3") : pl->blocks[i - 1].name;
    if (st == in_name) {
      const size_t bytes = (size_t)n * mh.C * mh.H * 8;
      TT_HIP(hipMalloc(&tmp.p, bytes));
      TT_TRY(block_input_rows(pl, L, i, (int)n, (uint64_t *)tmp.p, nullptr, s, &rows));
      return copy_out(rows, bytes);
    }
    for (int b = 0; b < 4; ++b) {
      if (st != mh.name + ".out" + std::to_string(b + 1)) continue;
      const uint32_t *dwords = nullptr;
      if (path == GatePath::Fused) {
        const size_t tap_elems = (size_t)pl->desc.max_batch * (mh.C / 8) * mh.Ho * mh.Wo;
        if (!mh.last && pl->tap_elems < tap_elems) {
          uint32_t *t = nullptr;
          TT_TRY(dev_alloc(pl, &t, tap_elems, true));
          pl->tap = t;
          pl->tap_elems = tap_elems;
        }
        TT_TRY(fused_branch_dwords(pl, L, i, (int)n, pl->tap, nullptr, s, &dwords));
      }
      const size_t bytes = (size_t)n * mh.C * mh.Ho * 8;
      TT_HIP(hipMalloc(&tmp.p, bytes));
      TT_TRY(branch_as_rows(pl, L, i, b, (int)n, dwords, (uint64_t *)tmp.p, nullptr, s, &rows));
      return copy_out(rows, bytes);
    }
  }
  set_error("unknown stage %s", stage);
  return TTNET_E_INVALID;
}

int ttnet_plan_get_table(ttnet_plan *pl, const char *name, void *dst_host, size_t dst_bytes) {
  BlockTT *b = nullptr;
  TT_TRY(table_block(pl, name, dst_host, dst_bytes, true, &b));
  std::vector<uint8_t> raw(b->g.table_bytes());
  TT_HIP(hipMemcpy(raw.data(), b->table, raw.size(), hipMemcpyDeviceToHost));
  walk_table(*b, raw.data(), dst_host, false);
  return TTNET_OK;
}

int ttnet_plan_set_table(ttnet_plan *pl, const char *name, const void *src_host, size_t src_bytes) {
  BlockTT *b = nullptr;
  TT_TRY(table_block(pl, name, src_host, src_bytes, false, &b));
  std::vector<uint8_t> raw(b->g.table_bytes(), 0);
  walk_table(*b, raw.data(), const_cast<void *>(src_host), true);      // (storing only reads the canonical side)
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(invalidate_graphs(pl));
  TT_HIP(hipMemcpy(b->table, raw.data(), raw.size(), hipMemcpyHostToDevice));
  drop_certify(pl);
  b->user_table = true;
  b->near_ties = -1;
  if (pl->path == GatePath::Fused)          // the kernels read images derived from the conv1 / conv2 / conv3 tables
    for (auto &mh : pl->blocks)
      if (b == &mh.c1 || b == &mh.c2 || b == &mh.c3) {
        TT_TRY(launch_fused_images(mh.c1.table, mh.c2.table, mh.c3.table, mh.C, mh.img_dw, mh.img_c3, nullptr));
        TT_HIP(hipDeviceSynchronize());
      }
  return TTNET_OK;
}

int ttnet_plan_query(ttnet_plan *pl, const char *what, int64_t *out) {
  if (!pl || !what || !out) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  const std::string w(what);
  if (w == "fcsize") *out = pl->fcsize;
  else if (w == "n_classes") *out = pl->n_classes;
  else if (w == "n_state_tensors") *out = (int64_t)pl->key_order.size();
  else if (w == "max_batch") *out = pl->desc.max_batch;
  else if (w == "table_bytes") *out = (int64_t)pl->table_bytes;
  else if (w == "workspace_bytes") *out = (int64_t)pl->workspace_bytes;
  else if (w == "usage_bytes") *out = (int64_t)(pl->usage_bytes + pl->scratch_bytes);
  else if (w == "care_bytes") *out = (int64_t)pl->care_bytes;
  else if (w == "care_blocks") *out = (int64_t)all_block_tts(pl).size();
  else if (w.rfind("last_n:", 0) == 0) {                      // images of the forward last issued on that lane (0: none yet)
    const int lane = atoi(w.c_str() + 7);
    if (lane < 0 || lane >= (int)pl->lanes.size()) {
      set_error("last_n: lane %d but the plan has %d (ttnet_plan_set_lanes)", lane, (int)pl->lanes.size());
      return TTNET_E_INVALID;
    }
    *out = pl->lanes[lane].last_n;
  }
  else if (w == "p") *out = pl->p;
  else if (w == "graph_replays") *out = pl->graph_replays;
  else if (w == "graphs_enabled") {
    *out = pl->graphs_ok ? 1 : 0;
    if (!pl->graphs_ok)
      set_error("graphs disabled: %s", pl->graph_off_reason.empty() ? "TTNET_NO_GRAPH is set" : pl->graph_off_reason.c_str());   // readable through ttnet_last_error
  }
  else if (w == "graph_captures") *out = pl->graph_captures;
  else if (w == "graph_drops") *out = pl->graph_drops;
  else if (w == "graphs_cached") {
    int64_t c = 0;
    for (auto &l : pl->lanes) c += (int64_t)l.graphs.size();
    *out = c;
  }
  else if (w == "range_overflow") {          // read and clear (synchronises the device: the flag is raised by kernels)
    TT_HIP(hipSetDevice(pl->device));
    TT_HIP(hipDeviceSynchronize());
    *out = *(volatile uint32_t *)pl->range_host ? 1 : 0;
    *pl->range_host = 0u;
  }
  else if (w == "lanes") *out = (int64_t)pl->lanes.size();
  else if (w == "gate_path") *out = (int64_t)pl->path;       // GatePath, in the order include/ttnet.h documents
  else if (w.rfind("gate_grid:", 0) == 0) {                   // workgroups of block i's first launch at the last forward's batch size
    char *end = nullptr;
    const long i = strtol(w.c_str() + 10, &end, 10);
    const int n = (int)pl->lanes[pl->last_lane].last_n;
    if (end == w.c_str() + 10 || *end || i < 0 || (size_t)i >= pl->blocks.size() || n <= 0 ||
        (pl->path != GatePath::Fused && pl->path != GatePath::TwoLaunch)) {
      set_error("%s: needs a block index below %zu, a forward on the lane used last, and the two-launch or fused path", what,
                pl->blocks.size());
      return TTNET_E_INVALID;
    }
    const int C = pl->blocks[(size_t)i].C;
    *out = pl->path == GatePath::Fused ? (int64_t)(C / 8) * part::fused_block_slices(C, n) : (int64_t)part::stage1_grid(C, n).blocks();
  }
  else if (w == "full_listed_pw" || w == "full_listed_dw") {      // full variant: (pixel, group) pairs / outputs sent to float64 so far (lane used last)
    uint32_t v[2] = {0, 0};
    const uint32_t *fix = pl->lanes[pl->last_lane].full_fix;
    if (fix) {
      TT_HIP(hipSetDevice(pl->device));
      TT_HIP(hipDeviceSynchronize());
      TT_HIP(hipMemcpy(v, fix + 62, sizeof(v), hipMemcpyDeviceToHost));
    }
    *out = v[w == "full_listed_dw" ? 1 : 0];
  }
  else if (w.rfind("near_ties:", 0) == 0) {
    BlockTT *b = find_block(pl, w.c_str() + 10);
    if (!b) {
      set_error("no Block_TT named %s", w.c_str() + 10);
      return TTNET_E_INVALID;
    }
    *out = b->near_ties;
  } else {
    set_error("unknown query %s", what);
    return TTNET_E_INVALID;
  }
  return TTNET_OK;
}

int ttnet_plan_set_profiling(ttnet_plan *pl, int enabled) {
  if (!pl) {
    set_error("null plan");
    return TTNET_E_INVALID;
  }
  pl->profiling = enabled != 0;
  pl->timing_used = 0;
  return TTNET_OK;
}

int ttnet_plan_last_timings(ttnet_plan *pl, const char **names, float *ms, int cap) {
  if (!pl || !names || !ms) {
    set_error("null argument");
    return TTNET_E_INVALID;
  }
  int k = 0;
  for (size_t i = 0; i < pl->timing_used && k < cap; ++i, ++k) {
    if (hipEventSynchronize(pl->timings[i].e1) != hipSuccess) {
      set_error("hipEventSynchronize failed");
      return TTNET_E_HIP;
    }
    float t = 0.f;
    (void)hipEventElapsedTime(&t, pl->timings[i].e0, pl->timings[i].e1);
    names[k] = pl->timings[i].name;
    ms[k] = t;
  }
  return k;
}

void ttnet_plan_destroy(ttnet_plan *pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  for (auto &t : pl->timings) {
    (void)hipEventDestroy(t.e0);
    (void)hipEventDestroy(t.e1);
  }
  for (auto &l : pl->lanes)
    for (auto &kv : l.graphs) drop_graph(kv.second);
  if (pl->cap_stream) (void)hipStreamDestroy(pl->cap_stream);
  if (pl->range_host) (void)hipHostFree(pl->range_host);
  for (void *ptr : pl->owned) (void)hipFree(ptr);
  delete pl;
}

}  // extern "C"
