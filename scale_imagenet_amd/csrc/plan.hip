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
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
#include <mutex>
#include <unordered_map>

#include "plan.h"

namespace ttnet {

static thread_local char g_err[1024] = "";

static void vset_error(const char *fmt, va_list ap) { vsnprintf(g_err, sizeof(g_err), fmt, ap); }

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vset_error(fmt, ap);
  va_end(ap);
}

int refused(int status, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vset_error(fmt, ap);
  va_end(ap);
  return status;
}

}  // namespace ttnet

using namespace ttnet;

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

constexpr double kBnEps = 1e-5;   // nn.BatchNorm2d / BatchNorm1d default

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
  if (d.image_h != 32 || d.image_w != 32) return refused(TTNET_E_UNSUPPORTED, "vAlexnet takes 32x32 inputs (got %dx%d)", d.image_h, d.image_w);
  if (d.max_batch < 1) return refused(TTNET_E_INVALID, "max_batch must be positive");
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
    return refused(TTNET_E_INVALID, "unknown variant %d", d.variant);
  }
  if (d.image_h != 224 || d.image_w != 224)
    return refused(TTNET_E_UNSUPPORTED, "only 224x224 inputs are supported (got %dx%d)", d.image_h, d.image_w);
  if (d.nfilter < 1 || d.tfilter < 1 || d.max_batch < 1) return refused(TTNET_E_INVALID, "nfilter, tfilter and max_batch must be positive");
  const bool full_variant = pl->path == GatePath::Full;
  const int p = d.nfilter * d.tfilter;
  pl->p = p;
  // The reference constructs any p whose group counts divide its channel counts (TT_general_imagenet_v2_small.py:
  // 165-167, :28-76); a fan-in of 16 (the truth tables of the small variant) needs p % 16 == 0, and the depthwise
  // tables of both table variants are striped by 16 channels.  Built: p in {16, 32, .., 128} for the table variants
  // (one, two or four 32-channel M-tiles in the stem kernel), p <= 64 for the full variant; anything else is refused here.
  if (p > 128 || (full_variant && p > 64) || (!full_variant && p % 16 != 0))
    return refused(TTNET_E_UNSUPPORTED,
                   "p = nfilter*tfilter = %d: built for p <= 128 with p %% 16 == 0 (fan-in 16 / tables striped by 16 channels; full variant: p <= 64)", p);
  if (d.layers >= 3 && p != 64)
    return refused(TTNET_E_UNSUPPORTED, "--layers %d at p = %d: the stride-1 blocks (two-launch gate kernels, channel-word layout) are built for p = 64", d.layers, p);
  std::vector<int> cfg, strides;
  switch (d.layers) {   // TT_general_imagenet_v2_small.py:172-181; a bare entry is a stride-1 block
    case 0: cfg = {p, 2 * p}; strides = {2, 2}; break;
    case 1: cfg = {p, 2 * p, 4 * p}; strides = {2, 2, 2}; break;
    case 2: cfg = {p, 2 * p, 4 * p, 8 * p}; strides = {2, 2, 2, 2}; break;
    case 3: cfg = {p, 2 * p, 4 * p, 8 * p}; strides = {1, 2, 2, 2}; break;
    case 4: cfg = {p, 2 * p, 2 * p, 4 * p, 8 * p}; strides = {1, 2, 1, 2, 2}; break;
    default:
      return refused(TTNET_E_UNSUPPORTED, "--layers %d: the reference defines 0..4", d.layers);
  }
  if (d.layers >= 3 && d.variant != TTNET_SMALL)
    return refused(TTNET_E_UNSUPPORTED, "--layers %d (stride-1 blocks) is built for the small variant only", d.layers);
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
        return refused(TTNET_E_UNSUPPORTED, "%s: no branch-padding rule for width %d (full variant)", mh.name.c_str(), w);
      }
    } else {
    // branch padding keyed by the input width (:98-139): out3/out4 are floor(h/2) wide
    if (w == 56) mh.off34 = 1;                       // pad0 = ZeroPad2d((1,0,1,0))
    else if (w == 29 || w == 15 || w == 8 || w == 16 || w == 30 || w == 57 || w == 58) mh.off34 = 0;   // pad2 = (0,1,0,1)
    else {
      return refused(TTNET_E_UNSUPPORTED, "%s: no branch-padding rule for width %d", mh.name.c_str(), w);
    }
    if (h / stride + 1 != ho || w / stride + 1 != wo || h != w)
      return refused(TTNET_E_UNSUPPORTED, "%s: branch shapes do not line up (%dx%d -> %dx%d)", mh.name.c_str(), h, w, ho, wo);
    }
    mh.Ho = ho; mh.Wo = wo;
    if (in_planes % gsize) return refused(TTNET_E_INVALID, "in_channels must be divisible by groups (in_planes=%d, group size %d)", in_planes, gsize);
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

// stem: BN scale folded into the weights, which are split into two prescaled fp16 planes in MFMA
// fragment order; BN shift as the weights of one more k-row (stem.hip)
int prepare_stem(ttnet_plan *pl) {
  std::vector<float> w;
  TT_TRY(fetch(pl->tensors["features.1.weight"], w));
  std::vector<uint16_t> wf(stem_split_weights_elems());
  std::vector<double> sc, sh;
  TT_TRY(fold_bn(pl, "features.2", sc, sh));
  float init[64];
  if (!stem_split_weights(w.data(), sc.data(), sh.data(), pl->p, wf.data(), init))
    return refused(TTNET_E_UNSUPPORTED, "stem: the folded BatchNorm shift of features.2 is outside the range of the split operands");
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
  if (!stem_split_weights_u8(w.data(), sc.data(), sh.data(), pl->p, pl->in_mean, pl->in_std, wf.data(), init, tab.data()))
    return refused(TTNET_E_UNSUPPORTED, "stem (uint8 input): the folded BatchNorm shift of features.2 is outside the range of the split operands");
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
  ttnet_plan::Lane *lp = nullptr;
  TT_TRY(lane_of(pl, "forward", lane, &lp));
  pl->last_lane = lane;
  ttnet_plan::Lane &L = *lp;
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

}  // namespace

// ---- helpers that plan_tables.hip and plan_certify.hip use too (plan.h) ----

void ttnet::dev_free(ttnet_plan *pl, void *ptr) {
  if (!ptr) return;
  auto it = std::find(pl->owned.begin(), pl->owned.end(), ptr);
  if (it != pl->owned.end()) pl->owned.erase(it);
  (void)hipFree(ptr);
}

// every Block_TT of the plan (vAlexnet's block has no convf: its entry keeps an empty name)
std::vector<BlockTT *> ttnet::all_block_tts(ttnet_plan *pl) {
  std::vector<BlockTT *> v;
  for (auto &mh : pl->blocks)
    for (BlockTT *b : {&mh.c1, &mh.c2, &mh.c3, &mh.cf})
      if (!b->g.name.empty()) v.push_back(b);
  return v;
}

BlockTT *ttnet::find_block(ttnet_plan *pl, const char *name) {
  for (BlockTT *b : all_block_tts(pl))
    if (b->g.name == name) return b;
  return nullptr;
}

int ttnet::fetch(const Tensor &t, std::vector<float> &host) {
  host.resize(t.bytes / 4);
  TT_HIP(hipMemcpy(host.data(), t.dev, t.bytes, hipMemcpyDeviceToHost));
  return TTNET_OK;
}

// eval-mode BatchNorm as y = x*scale + shift, folded in float64
int ttnet::fold_bn(ttnet_plan *pl, const std::string &prefix, std::vector<double> &scale, std::vector<double> &shift) {
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

void ttnet::begin_timing(ttnet_plan *pl, const char *name, hipStream_t s) {
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
void ttnet::end_timing(ttnet_plan *pl, const char *name, hipStream_t s) {
  if (!pl->profiling || !name) return;
  (void)hipEventRecord(pl->timings[pl->timing_used].e1, s);
  pl->timing_used++;
}

// Each gate path keeps its activations in its own layout; these three answer in the one layout of the C ABI
// (ttnet_read_stage, ttnet_table_usage_add, ttnet_care_misses).  timing: the name the conversion launches are timed
// under (nullptr: not timed).

// The branch dwords of fused block i, whose branch tensors never reach HBM: a last block's are its output; any other
// block is run once more on its (still resident) input with `tap` attached -- it rewrites the next block's input with
// the same bits
int ttnet::fused_branch_dwords(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint32_t *tap, const char *timing, hipStream_t s,
                               const uint32_t **dwords) {
  *dwords = pl->blocks[i].last ? L.blk[i].idx : tap;
  if (!pl->blocks[i].last) TT_TIMED(pl, timing, s, launch_gate_block(fused_args(pl, L, i, n, tap), s));
  return TTNET_OK;
}

// The input of block i as rows [n][C][H]: in place, but for the compact rows of the fused path (blocks after the
// first), which are widened into buf
int ttnet::block_input_rows(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint64_t *buf, const char *timing, hipStream_t s,
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
int ttnet::branch_as_rows(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int k, int n, const uint32_t *dwords, uint64_t *buf,
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

// The range flag is raised by a kernel, i.e. asynchronously: the forward that overflowed has already
// returned TTNET_OK.  Every later call on the plan fails until the flag is read (and cleared) with
// ttnet_plan_query("range_overflow"); ttnet_read_stage checks it after its own synchronisation.
int ttnet::check_range(ttnet_plan *pl) {
  if (pl->range_host && *(volatile uint32_t *)pl->range_host)
    return refused(TTNET_E_RANGE, "an earlier forward on this plan met an activation outside the range of the fp16 x 2 operand split "
                                  "(|input| or |feature| >= 4094, or NaN): its logits are invalid; ttnet_plan_query(\"range_overflow\") "
                                  "reads and clears the flag");
  return TTNET_OK;
}

int ttnet::check_ready(ttnet_plan *pl, const void *in, int64_t n, const void *out, const char *who) {
  if (!pl || !in || !out) return refused(TTNET_E_INVALID, "null argument");
  if (!pl->finalized) return refused(TTNET_E_STATE, "%s before ttnet_plan_finalize", who);
  if (n < 1 || n > pl->desc.max_batch) return refused(TTNET_E_INVALID, "batch %lld outside [1, max_batch=%d]", (long long)n, pl->desc.max_batch);
  return check_range(pl);
}

int ttnet::lane_of(ttnet_plan *pl, const char *who, int lane, ttnet_plan::Lane **out) {
  if (lane < 0 || lane >= (int)pl->lanes.size())
    return refused(TTNET_E_INVALID, "%s: lane %d but the plan has %d (ttnet_plan_set_lanes)", who, lane, (int)pl->lanes.size());
  *out = &pl->lanes[lane];
  return TTNET_OK;
}

// Captured graphs bake in by-value kernel arguments derived from the weights (lin2's 1/prescale) and
// the device addresses of tables: whenever a tensor, a table or the finalized state changes they are
// all dropped (after a device synchronisation -- a replay may still be in flight) and re-captured
// from the third forward on.
int ttnet::invalidate_graphs(ttnet_plan *pl) {
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

extern "C" {

const char *ttnet_last_error(void) { return g_err; }
const char *ttnet_version(void) { return "ttnet-mi355x 0.1 (gfx950)"; }

int ttnet_plan_create(const ttnet_net_desc *desc, int device, ttnet_plan **out) {
  if (!desc || !out) return refused(TTNET_E_INVALID, "null argument");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return refused(TTNET_E_HIP, "no HIP device: libttnet has no CPU path");
  if (device < 0 || device >= count) return refused(TTNET_E_INVALID, "device %d out of range (%d devices)", device, count);
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
  if (!pl || !key || !ptr || (ndim > 0 && !shape)) return refused(TTNET_E_INVALID, "null argument");
  std::string k(key);
  if (k.rfind("module.", 0) == 0) k = k.substr(7);   // DataParallel / DDP checkpoints (main.py:181-192)
  auto it = pl->tensors.find(k);
  if (it == pl->tensors.end())
    return refused(TTNET_E_INVALID, "unexpected key in state_dict: %s", key);
  Tensor &t = it->second;
  bool ok = (dtype == t.dtype) && (ndim == (int)t.shape.size());
  for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == t.shape[i];
  if (!ok) return refused(TTNET_E_INVALID, "size mismatch for %s", key);
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
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipSetDevice(pl->device));
  TT_TRY(invalidate_graphs(pl));
  for (auto &k : pl->key_order) {
    const Tensor &t = pl->tensors[k];
    if (t.required && !t.set) return refused(TTNET_E_STATE, "missing key in state_dict: %s", k.c_str());
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
  if (!pl || lanes < 1 || lanes > 16) return refused(TTNET_E_INVALID, "set_lanes: %d outside [1,16]", lanes);
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
  if (!pl || !mean3 || !std3) return refused(TTNET_E_INVALID, "set_input_norm: null argument");
  for (int c = 0; c < 3; ++c)
    if (!(std3[c] > 0.f)) {                            // (refused whole: the plan keeps the constants it had)
      return refused(TTNET_E_INVALID, "set_input_norm: std[%d] = %g", c, (double)std3[c]);
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

int ttnet_plan_query(ttnet_plan *pl, const char *what, int64_t *out) {
  if (!pl || !what || !out) return refused(TTNET_E_INVALID, "null argument");
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
    ttnet_plan::Lane *L = nullptr;
    TT_TRY(lane_of(pl, "last_n", atoi(w.c_str() + 7), &L));
    *out = L->last_n;
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
        (pl->path != GatePath::Fused && pl->path != GatePath::TwoLaunch))
      return refused(TTNET_E_INVALID, "%s: needs a block index below %zu, a forward on the lane used last, and the two-launch or fused path", what,
                pl->blocks.size());
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
    if (!b) return refused(TTNET_E_INVALID, "no Block_TT named %s", w.c_str() + 10);
    *out = b->near_ties;
  } else {
    return refused(TTNET_E_INVALID, "unknown query %s", what);
  }
  return TTNET_OK;
}

int ttnet_plan_set_profiling(ttnet_plan *pl, int enabled) {
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
  pl->profiling = enabled != 0;
  pl->timing_used = 0;
  return TTNET_OK;
}

int ttnet_plan_last_timings(ttnet_plan *pl, const char **names, float *ms, int cap) {
  if (!pl || !names || !ms) return refused(TTNET_E_INVALID, "null argument");
  int k = 0;
  for (size_t i = 0; i < pl->timing_used && k < cap; ++i, ++k) {
    if (hipEventSynchronize(pl->timings[i].e1) != hipSuccess) return refused(TTNET_E_HIP, "hipEventSynchronize failed");
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
