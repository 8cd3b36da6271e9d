// The plan object and the host helpers that plan.hip, plan_tables.hip and plan_certify.hip share.  Host only, private to
// those three files: the C ABI is include/ttnet.h.
//
//   plan.hip          geometry, allocation, finalize, the forward (eager, captured, replayed), query, profiling, destroy
//   plan_tables.hip   tables and stage views: get / set table, ttnet_read_stage, usage counts, care sets
//   plan_certify.hip  vAlexnet: the three certificate entries and the two attack entries
#pragma once

#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "partition.h"
#include "ttnet_common.h"
#include "va_block.h"

namespace ttnet {

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

}  // namespace ttnet

struct ttnet_plan {
  ttnet_net_desc desc{};
  int device = 0;
  int p = 0;
  int n_classes = 1000, inter = 1000, fcsize = 0;
  int featC = 0, featPP = 0;        // last block: channels, pooled pixels per channel
  std::string head;
  std::vector<ttnet::MultiHead> blocks;
  std::map<std::string, ttnet::Tensor> tensors;
  std::vector<std::string> key_order;
  bool finalized = false;
  ttnet::GatePath path = ttnet::GatePath::TwoLaunch;
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
  int usage_scheme_dw = ttnet::kUsageMerged, usage_scheme_pw = ttnet::kUsageMerged;   // per table shape: depthwise / grouped 1x1 (DESIGN: table usage)
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
  std::vector<ttnet::Timing> timings;
  size_t timing_used = 0;

  std::vector<void *> owned;        // everything hipMalloc'ed, freed in destroy
};

namespace ttnet {

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

// ---- plan.hip ----
int refused(int status, const char *fmt, ...);      // set_error(fmt, ..), then the status: `return refused(TTNET_E_INVALID, "..", ..);`
void dev_free(ttnet_plan *pl, void *ptr);
std::vector<BlockTT *> all_block_tts(ttnet_plan *pl);      // every Block_TT of the plan, in the column order of ttnet_care_misses
BlockTT *find_block(ttnet_plan *pl, const char *name);
int fetch(const Tensor &t, std::vector<float> &host);
int fold_bn(ttnet_plan *pl, const std::string &prefix, std::vector<double> &scale, std::vector<double> &shift);
int check_range(ttnet_plan *pl);
int check_ready(ttnet_plan *pl, const void *in, int64_t n, const void *out, const char *who = "ttnet_forward");
// The lane a call names: "<who>: lane %d but the plan has %d (ttnet_plan_set_lanes)" and TTNET_E_INVALID when there is none
int lane_of(ttnet_plan *pl, const char *who, int lane, ttnet_plan::Lane **out);
int invalidate_graphs(ttnet_plan *pl);
void begin_timing(ttnet_plan *pl, const char *name, hipStream_t s);      // (name == nullptr: not timed)
void end_timing(ttnet_plan *pl, const char *name, hipStream_t s);
// a stage of the last forward as uint64 rows, whatever layout the gate path keeps it in
int fused_branch_dwords(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint32_t *tap, const char *timing, hipStream_t s,
                        const uint32_t **dwords);
int block_input_rows(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int n, uint64_t *buf, const char *timing, hipStream_t s,
                     const uint64_t **rows);
int branch_as_rows(ttnet_plan *pl, const ttnet_plan::Lane &L, size_t i, int k, int n, const uint32_t *dwords, uint64_t *buf,
                   const char *timing, hipStream_t s, const uint64_t **rows);
// ---- plan_tables.hip ----
int alloc_usage_scratch(ttnet_plan *pl, ttnet_plan::Lane &L);
// ---- plan_certify.hip ----
void drop_certify(ttnet_plan *pl);

#define TT_TIMED(pl, name, s, expr) \
  do {                              \
    begin_timing(pl, name, s);      \
    int r__ = (expr);               \
    end_timing(pl, name, s);        \
    if (r__ != TTNET_OK) return r__; \
  } while (0)

}  // namespace ttnet
