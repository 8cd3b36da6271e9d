// libttnet.so -- what reads or rewrites the plan's truth tables and stage views: ttnet_plan_get_table / _set_table,
// ttnet_read_stage, the usage counts (ttnet_plan_table_usage_*, ttnet_table_usage_add) and the care sets
// (ttnet_plan_set_care / _clear_care, ttnet_care_misses) of include/ttnet.h.
//
// Host code only: the kernels are usage.hip's, the stage conversions gate.hip's and gate_fused.hip's.

#include <stdlib.h>

#include "plan.h"

using namespace ttnet;

namespace {

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
  if (!pl || !name || !host) return refused(TTNET_E_INVALID, "null argument");
  BlockTT *b = find_block(pl, name);
  if (!b) return refused(TTNET_E_INVALID, "no Block_TT named %s", name);
  if (pl->path == GatePath::Full)
    return refused(TTNET_E_UNSUPPORTED, "the full variant (fan-in 30) has no truth tables: 2^30 entries per output bit");
  if (get && !pl->finalized) return refused(TTNET_E_STATE, "get_table before finalize");
  if (bytes != b->g.canonical_bytes())
    return refused(TTNET_E_INVALID, "%s(%s): %s is %zu bytes, table is %zu", get ? "get_table" : "set_table", name, get ? "destination" : "source", bytes,
                   b->g.canonical_bytes());
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
  if (pl->path == GatePath::Full)
    return refused(TTNET_E_UNSUPPORTED, "the full variant (fan-in 30) has no truth tables: 2^30 entries per output bit");
  if (pl->path == GatePath::VAlexnet) return refused(TTNET_E_UNSUPPORTED, "%s is not built for the vAlexnet variant", what);
  return TTNET_OK;
}

// The lane whose last forward ttnet_table_usage_add / ttnet_care_misses read
int usage_lane(ttnet_plan *pl, const char *who, int lane, const ttnet_plan::Lane **out) {
  ttnet_plan::Lane *L = nullptr;
  TT_TRY(lane_of(pl, who, lane, &L));
  if (L->last_n < 1) return refused(TTNET_E_STATE, "%s: no forward has run on lane %d", who, lane);
  *out = L;
  return TTNET_OK;
}

// One table's lookups of a forward: the operand rows src[0..nsrc) ([n][C][H] each), the ho x wo grid of outputs and
// where the table stands: block `block`, column `col` (0..3 = conv1, conv2, conv3, convf; all_block_tts order)
struct Lookups {
  const MultiHead *mh;
  const BlockTT *b;
  const uint64_t *const *src;
  int nsrc, n, ho, wo;
  size_t block;
  int col;
};

// the timing names of a walk's launches
struct WalkNames {
  const char *prep, *dw, *conv3, *tap, *convf;
};

// Every table lookup of the forward last issued on lane L, block by block: the two depthwise tables and conv3 on the
// block's input rows, then convf on the four branch tensors after their padding (a non-last fused block is run again
// once, not once per branch).  A table that is not wanted(b) is passed over, and so is a conversion that only unwanted
// tables would read.  dw / pw launch what is done with a depthwise / grouped 1x1 table's lookups.
template <typename Wanted, typename Dw, typename Pw>
int walk_lookups(ttnet_plan *pl, const ttnet_plan::Lane &L, const WalkNames &names, hipStream_t s, Wanted wanted, Dw dw, Pw pw) {
  const int n = (int)L.last_n;
  for (size_t i = 0; i < pl->blocks.size(); ++i) {
    const MultiHead &mh = pl->blocks[i];
    if (wanted(mh.c1) || wanted(mh.c2) || wanted(mh.c3)) {
      const uint64_t *xin = nullptr;
      TT_TRY(block_input_rows(pl, L, i, n, L.u_rows, names.prep, s, &xin));
      int col = 0;
      for (const BlockTT *b : {&mh.c1, &mh.c2}) {
        const BlockGeom &g = b->g;
        const int ho = (mh.H + 2 * g.pad - g.kh) / g.stride + 1, wo = (mh.W + 2 * g.pad - g.kw) / g.stride + 1;
        if (wanted(*b)) TT_TIMED(pl, names.dw, s, dw(Lookups{&mh, b, &xin, 1, n, ho, wo, i, col}));
        ++col;
      }
      if (wanted(mh.c3)) TT_TIMED(pl, names.conv3, s, pw(Lookups{&mh, &mh.c3, &xin, 1, n, mh.H, mh.W, i, 2}));
    }
    if (!wanted(mh.cf)) continue;
    const uint32_t *dwords = nullptr;
    if (pl->path == GatePath::Fused) TT_TRY(fused_branch_dwords(pl, L, i, n, L.u_tap, names.tap, s, &dwords));
    const uint64_t *br[4];
    for (int k = 0; k < 4; ++k) TT_TRY(branch_as_rows(pl, L, i, k, n, dwords, L.u_br[k], names.prep, s, &br[k]));
    TT_TIMED(pl, names.convf, s, pw(Lookups{&mh, &mh.cf, br, 4, n, mh.Ho, mh.Wo, i, 3}));
  }
  return TTNET_OK;
}

}  // namespace

// Per-lane scratch of ttnet_table_usage_add and ttnet_care_misses, sized for max_batch (a lane that has its scratch keeps it)
int ttnet::alloc_usage_scratch(ttnet_plan *pl, ttnet_plan::Lane &L) {
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

extern "C" {

int ttnet_plan_table_usage_enable(ttnet_plan *pl, int enabled) {
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
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
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
  if (!pl->usage_on) return refused(TTNET_E_STATE, "table_usage_reset before ttnet_plan_table_usage_enable");
  for (BlockTT *b : all_block_tts(pl))
    TT_HIP(hipMemsetAsync(b->usage, 0, b->g.entries() * sizeof(int64_t), (hipStream_t)stream));
  return TTNET_OK;
}

int ttnet_table_usage_add(ttnet_plan *pl, int lane, void *stream) {
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
  if (!pl->usage_on) return refused(TTNET_E_STATE, "table_usage_add before ttnet_plan_table_usage_enable");
  const ttnet_plan::Lane *L = nullptr;
  TT_TRY(usage_lane(pl, "table_usage_add", lane, &L));
  hipStream_t s = (hipStream_t)stream;
  return walk_lookups(
      pl, *L, {"usage.prep", "usage.dw", "usage.conv3", "usage.tap", "usage.convf"}, s, [](const BlockTT &) { return true; },
      [&](const Lookups &k) {
        const BlockGeom &g = k.b->g;
        return launch_usage_dw(k.src[0], k.n, k.mh->C, k.mh->H, k.mh->W, k.ho, k.wo, g.kh, g.kw, g.stride, g.pad, k.b->usage, pl->usage_scheme_dw, s);
      },
      [&](const Lookups &k) {
        return launch_usage_pw(k.src, k.nsrc, k.n, k.mh->C, k.b->g.groups, k.b->g.cin_g(), k.ho, k.wo, k.b->usage, pl->usage_scheme_pw, s);
      });
}

int ttnet_plan_get_table_usage(ttnet_plan *pl, const char *name, int64_t *dst_host, size_t dst_bytes) {
  if (!pl || !name || !dst_host) return refused(TTNET_E_INVALID, "null argument");
  if (!pl->usage_on) return refused(TTNET_E_STATE, "get_table_usage before ttnet_plan_table_usage_enable");
  BlockTT *b = find_block(pl, name);
  if (!b) return refused(TTNET_E_INVALID, "no Block_TT named %s", name);
  const size_t need = b->g.entries() * sizeof(int64_t);
  if (dst_bytes != need)
    return refused(TTNET_E_INVALID, "get_table_usage(%s): destination is %zu bytes, the counters are %zu", name, dst_bytes, need);
  TT_HIP(hipSetDevice(pl->device));
  TT_HIP(hipDeviceSynchronize());
  TT_HIP(hipMemcpy(dst_host, b->usage, need, hipMemcpyDeviceToHost));
  return TTNET_OK;
}

int ttnet_plan_set_care(ttnet_plan *pl, const char *name, const uint32_t *bits_host, size_t bytes) {
  if (!pl || !name) return refused(TTNET_E_INVALID, "null argument");
  TT_TRY(check_usage_served(pl, "the care set"));
  BlockTT *b = find_block(pl, name);
  if (!b) return refused(TTNET_E_INVALID, "no Block_TT named %s", name);
  const size_t words = care_words(*b);
  if (bits_host && bytes != words * sizeof(uint32_t))
    return refused(TTNET_E_INVALID, "set_care(%s): source is %zu bytes, the bitmap is %zu", name, bytes, words * sizeof(uint32_t));
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
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
  if (!pl->care_on) return TTNET_OK;
  TT_HIP(hipSetDevice(pl->device));
  TT_HIP(hipDeviceSynchronize());
  free_care(pl);
  return TTNET_OK;
}

int ttnet_care_misses(ttnet_plan *pl, int lane, int32_t *rows_dev, void *stream) {
  if (!pl) return refused(TTNET_E_INVALID, "null plan");
  if (!pl->care_on) return refused(TTNET_E_STATE, "care_misses before ttnet_plan_set_care");
  if (!rows_dev || ((uintptr_t)rows_dev & 3)) return refused(TTNET_E_INVALID, "care_misses: rows_dev is null or not 4-byte aligned");
  const ttnet_plan::Lane *L = nullptr;
  TT_TRY(usage_lane(pl, "care_misses", lane, &L));
  const int nb = (int)pl->blocks.size() * 4;           // row length: the Block_TTs in the order of all_block_tts
  hipStream_t s = (hipStream_t)stream;
  TT_HIP(hipMemsetAsync(rows_dev, 0, (size_t)L->last_n * nb * sizeof(int32_t), s));
  return walk_lookups(
      pl, *L, {"care.prep", "care.dw", "care.conv3", "care.tap", "care.convf"}, s, [](const BlockTT &b) { return b.care != nullptr; },
      [&](const Lookups &k) {
        const BlockGeom &g = k.b->g;
        return launch_care_dw(k.src[0], k.n, k.mh->C, k.mh->H, k.mh->W, k.ho, k.wo, g.kh, g.kw, g.stride, g.pad, k.b->care,
                              rows_dev + 4 * k.block + k.col, nb, s);
      },
      [&](const Lookups &k) {
        return launch_care_pw(k.src, k.nsrc, k.n, k.mh->C, k.b->g.groups, k.b->g.cin_g(), k.ho, k.wo, k.b->care, rows_dev + 4 * k.block + k.col, nb, s);
      });
}

int ttnet_read_stage(ttnet_plan *pl, const char *stage, int64_t n, void *dst, size_t dst_bytes, int on_device,
                     void *stream) {
  if (!pl || !stage || !dst) return refused(TTNET_E_INVALID, "null argument");
  const ttnet_plan::Lane &L = pl->lanes[pl->last_lane];
  if (n < 1 || n > L.last_n)
    return refused(TTNET_E_STATE, "read_stage: n=%lld but the last forward ran %lld images", (long long)n, (long long)L.last_n);
  hipStream_t s = (hipStream_t)stream;
  const std::string st(stage);
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  auto copy_out = [&](const void *src, size_t bytes) -> int {
    if (dst_bytes != bytes) return refused(TTNET_E_INVALID, "read_stage(%s): destination is %zu bytes, stage is %zu", stage, dst_bytes, bytes);
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
    return refused(TTNET_E_INVALID, "unknown stage %s", stage);
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
  return refused(TTNET_E_INVALID, "unknown stage %s", stage);
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

}  // extern "C"
