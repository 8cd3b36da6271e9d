// ttnet_launch_partition: csrc/partition.h read out by name.  No plan, no device, no HIP call: the tests derive their
// batch sizes and edge images from the arithmetic the launchers and kernels themselves use.

#include <string.h>

#include <string>

#include "partition.h"
#include "ttnet_common.h"

namespace {

using namespace ttnet::part;
typedef int64_t I;

// What an argument may be, by kind: 'n' a batch size in [1, 2^20]; 'C' input planes, a multiple of 8 in [8, 8192]
// ('D': of 16); 'd' a side length in [1, 512]; 'c' a count in [1, 65536]; 'i' an index in [0, 2^31); 'u' a 32-bit
// count; 'f' 0 or 1.  The bounds keep every product of the header inside an int.
struct Arg { const char *name; char kind; };
struct Key {
  const char *name;
  int n_args;
  Arg args[5];
  int n_out;
  int (*fn)(const I *a, I *o);           // 0, or a negative status with the message set
};

int fail(const char *key, const char *fmt, I v, I bound) {
  ttnet::set_error((std::string("launch_partition ") + key + ": " + fmt).c_str(), (long long)v, (long long)bound);
  return TTNET_E_INVALID;
}

int check_arg(const char *key, const Arg &g, I v) {
  I lo = 0, hi = 0, mult = 1;
  switch (g.kind) {
    case 'n': lo = 1; hi = 1 << 20; break;
    case 'C': lo = 8; hi = 8192; mult = 8; break;
    case 'D': lo = 16; hi = 8192; mult = 16; break;
    case 'd': lo = 1; hi = 512; break;
    case 'c': lo = 1; hi = 65536; break;
    case 'i': lo = 0; hi = 0x7FFFFFFF; break;
    case 'u': lo = 0; hi = 0xFFFFFFFFll; break;
    default: lo = 0; hi = 1; break;
  }
  if (v < lo || v > hi || v % mult) {
    ttnet::set_error("launch_partition %s: %s=%lld must be a multiple of %lld in [%lld, %lld]", key, g.name, (long long)v,
                     (long long)mult, (long long)lo, (long long)hi);
    return TTNET_E_INVALID;
  }
  return 0;
}

int flat(const FlatGrid &g, I *o) {
  o[0] = g.per_image;
  o[1] = g.threads;
  return 0;
}

// the cut of n * P workgroups that the patch sweep and the patch search share; `key` names the caller in a refusal
int patch_cut(const char *key, const I *a, I *o) {
  if (a[1] > ttnet::va::kPatchMax || a[2] > ttnet::va::kPatchMax) return fail(key, "a patch side of %lld is above %lld", a[1] > a[2] ? a[1] : a[2], ttnet::va::kPatchMax);
  if (a[3] > 32) return fail(key, "stride=%lld is above %lld", a[3], 32);
  o[0] = patch_positions((int)a[1], (int)a[3]); o[1] = patch_positions((int)a[2], (int)a[3]);
  const long long tasks = a[0] * o[0] * o[1];
  o[2] = patch_launches(tasks); o[3] = patch_launch_size(tasks, 0); o[4] = patch_launch_size(tasks, o[2] - 1); o[5] = kPatchGrid;
  return 0;
}

const Key kKeys[] = {
    // ---- common
    {"slices_for", 3, {{"n", 'n'}, {"units", 'c'}, {"target", 'c'}}, 1, [](const I *a, I *o) {
       o[0] = slices_for((int)a[0], (int)a[1], (int)a[2]);
       return 0;
     }},
    {"slice", 3, {{"sl", 'i'}, {"n", 'n'}, {"slices", 'c'}}, 2, [](const I *a, I *o) {     // -> n0, n1
       if (a[0] >= a[2]) return fail("slice", "sl=%lld but there are %lld slices", a[0], a[2]);
       o[0] = slice_begin((int)a[0], (int)a[1], (int)a[2]);
       o[1] = slice_begin((int)a[0] + 1, (int)a[1], (int)a[2]);
       return 0;
     }},
    // ---- fused path
    {"fused.const", 0, {}, 4, [](const I *, I *o) {     // -> threads, bytes of a table buffer, bytes left for a round, workgroups at most
       o[0] = kFT; o[1] = kFBuf; o[2] = kFMaxScratch; o[3] = kFusedTarget;
       return 0;
     }},
    {"fused.round", 1, {{"HO", 'd'}}, 1, [](const I *a, I *o) {
       o[0] = fused_round((int)a[0]);
       return 0;
     }},
    {"fused.launch", 3, {{"C", 'C'}, {"HO", 'd'}, {"n", 'n'}}, 4, [](const I *a, I *o) {     // -> grid, slices, R, placement (FusedPlacement)
       const int strands = (int)a[0] / 8, slices = fused_block_slices((int)a[0], (int)a[2]);
       o[0] = (I)strands * slices; o[1] = slices; o[2] = fused_launch_round((int)a[1], (int)a[2], slices); o[3] = fused_placement(strands, slices);
       return 0;
     }},
    {"fused.owner", 3, {{"b", 'i'}, {"C", 'C'}, {"n", 'n'}}, 2, [](const I *a, I *o) {       // -> strand, slice
       const int strands = (int)a[1] / 8, slices = fused_block_slices((int)a[1], (int)a[2]);
       if (a[0] >= (I)strands * slices) return fail("fused.owner", "b=%lld but the grid is %lld", a[0], (I)strands * slices);
       const FusedOwner w = fused_owner((int)a[0], strands, slices);
       o[0] = w.strand; o[1] = w.slice;
       return 0;
     }},
    // ---- two-launch path
    {"two_launch.const", 0, {}, 3, [](const I *, I *o) {
       o[0] = kDwTarget; o[1] = kPwTarget; o[2] = kPfTarget;
       return 0;
     }},
    {"two_launch.stage1", 2, {{"C", 'D'}, {"n", 'n'}}, 5, [](const I *a, I *o) {             // -> grid, depthwise units, their slices, conv3 units, their slices
       const Stage1Grid g = stage1_grid((int)a[0], (int)a[1]);
       o[0] = g.blocks(); o[1] = g.n_dw; o[2] = g.sl_dw; o[3] = g.n_pw; o[4] = g.sl_pw;
       return 0;
     }},
    {"two_launch.pf", 2, {{"C", 'C'}, {"n", 'n'}}, 2, [](const I *a, I *o) {                 // -> units, slices
       o[0] = pf_units((int)a[0]); o[1] = pf_slices((int)a[0], (int)a[1]);
       return 0;
     }},
    // ---- flat grids -> tasks per image, threads per workgroup
    {"flat.xs_branches", 2, {{"C", 'C'}, {"Ho", 'd'}}, 2, [](const I *a, I *o) { return flat(xs_branches_grid((int)a[0], (int)a[1]), o); }},
    {"flat.xs_pf", 2, {{"C", 'C'}, {"Ho", 'd'}}, 2, [](const I *a, I *o) { return flat(xs_pf_grid((int)a[0], (int)a[1]), o); }},
    {"flat.xs_last", 3, {{"C", 'C'}, {"Ho", 'd'}, {"Wo", 'd'}}, 2, [](const I *a, I *o) { return flat(xs_last_grid((int)a[0], (int)a[1], (int)a[2]), o); }},
    {"flat.va_dw", 0, {}, 2, [](const I *, I *o) { return flat(va_dw_grid(), o); }},
    {"flat.va_c3", 0, {}, 2, [](const I *, I *o) { return flat(va_c3_grid(), o); }},
    {"flat.va_feat", 0, {}, 2, [](const I *, I *o) { return flat(va_feat_grid(), o); }},
    // ---- full variant
    {"full.const", 0, {}, 8, [](const I *, I *o) {
       o[0] = kFullDwRows; o[1] = kFullDwGrid; o[2] = kFullDwFixGrid; o[3] = kFullPwWaves; o[4] = kFullPwGrid;
       o[5] = kFullFixGrid; o[6] = kFullFixPixels; o[7] = kFullFixShare;
       return 0;
     }},
    {"full.row_bundle", 2, {{"H", 'd'}, {"W", 'd'}}, 2, [](const I *a, I *o) {               // -> rows per wave task, wave tasks per image
       if (a[1] > 64) return fail("full.row_bundle", "W=%lld but a wave task has %lld lanes", a[1], 64);
       const RowBundle rb((int)a[0], (int)a[1]);
       o[0] = rb.rpw; o[1] = rb.bundles;
       return 0;
     }},
    {"full.dw", 3, {{"n", 'n'}, {"C", 'c'}, {"ho", 'd'}}, 2, [](const I *a, I *o) {           // -> chunks, chunks at most
       o[0] = full_dw_chunks((int)a[0], (int)a[1], (int)a[2]); o[1] = full_cap((int)a[1], kFullDwGrid);
       return 0;
     }},
    {"full.pw", 4, {{"n", 'n'}, {"groups", 'c'}, {"H", 'd'}, {"W", 'd'}}, 4, [](const I *a, I *o) {     // -> wave tasks, chunks, chunks at most, chunks of the list pass
       if (a[3] > 64) return fail("full.pw", "W=%lld but a wave task has %lld lanes", a[3], 64);
       const int tasks = full_pw_tasks((int)a[0], (int)a[2], (int)a[3]);
       o[0] = tasks; o[1] = full_pw_chunks(tasks, (int)a[1]); o[2] = full_cap((int)a[1], kFullPwGrid); o[3] = full_fix_xchunks(tasks, (int)a[1]);
       return 0;
     }},
    {"full.fix", 5, {{"n", 'n'}, {"groups", 'c'}, {"H", 'd'}, {"W", 'd'}, {"listed", 'u'}}, 2, [](const I *a, I *o) {   // -> wave tasks of a group's list, chunks
       if (a[3] > 64) return fail("full.fix", "W=%lld but a wave task has %lld lanes", a[3], 64);
       const I pixels = a[0] * a[2] * a[3];                                                 // (a list never holds more than every pixel)
       if (pixels > 0xFFFFFFFFll) return fail("full.fix", "%lld pixels do not fit the 32-bit list of %lld", pixels, a[0]);
       o[0] = full_fix_tasks((uint32_t)std::min(a[4], pixels));
       o[1] = full_fix_xchunks(full_pw_tasks((int)a[0], (int)a[2], (int)a[3]), (int)a[1]);
       return 0;
     }},
    {"full.fix_entries", 3, {{"groups", 'c'}, {"H", 'd'}, {"W", 'd'}}, 1, [](const I *a, I *o) {
       o[0] = (I)full_fix_entries((int)a[0], (int)a[1], (int)a[2]);
       return 0;
     }},
    // ---- stem
    {"stem.const", 0, {}, 4, [](const I *, I *o) {      // -> items per image, stage buffers, workgroups on the whole chip, on half of it
       o[0] = NBLK; o[1] = NSTAGE; o[2] = kStemGrid; o[3] = kStemHalfGrid;
       return 0;
     }},
    {"stem.workgroups", 3, {{"lanes", 'c'}, {"u8", 'f'}, {"full", 'f'}}, 1, [](const I *a, I *o) {
       o[0] = stem_workgroups((int)a[0], a[1] != 0, a[2] != 0);
       return 0;
     }},
    {"stem.grid", 2, {{"n", 'n'}, {"G", 'c'}}, 1, [](const I *a, I *o) {
       o[0] = stem_grid((int)a[0], (int)a[1]);
       return 0;
     }},
    {"stem.run", 3, {{"bid", 'i'}, {"n", 'n'}, {"G", 'c'}}, 2, [](const I *a, I *o) {        // -> first item, items
       const int grid = stem_grid((int)a[1], (int)a[2]);
       if (a[0] >= grid) return fail("stem.run", "bid=%lld but the grid is %lld", a[0], grid);
       o[0] = stem_first_item((int)a[0], (int)a[1], grid); o[1] = stem_my_items((int)a[0], (int)a[1], grid);
       return 0;
     }},
    {"stem.continues", 2, {{"first", 'i'}, {"j", 'i'}}, 1, [](const I *a, I *o) {
       if (a[0] + a[1] > 0x7FFFFFFF) return fail("stem.continues", "item %lld + %lld is out of range", a[0], a[1]);
       o[0] = stem_continues((int)a[0], (int)a[1]) ? 1 : 0;
       return 0;
     }},
    // ---- patch sweep and patch search: the same cut
    {"patch.sweep", 4, {{"n", 'n'}, {"patch_h", 'd'}, {"patch_w", 'd'}, {"stride", 'd'}}, 6, [](const I *a, I *o) { return patch_cut("patch.sweep", a, o); }},   // -> positions down, across, launches, workgroups of the first, of the last, at most
    {"patch.attack", 4, {{"n", 'n'}, {"patch_h", 'd'}, {"patch_w", 'd'}, {"stride", 'd'}}, 6, [](const I *a, I *o) { return patch_cut("patch.attack", a, o); }},
};

}  // namespace

extern "C" int ttnet_launch_partition(const char *what, const int64_t *args, int n_args, int64_t *out, int out_cap) {
  if (!what || n_args < 0 || (n_args > 0 && !args) || out_cap < 0 || (out_cap > 0 && !out)) {
    ttnet::set_error("launch_partition: null argument or negative count");
    return TTNET_E_INVALID;
  }
  for (const Key &k : kKeys) {
    if (strcmp(k.name, what)) continue;
    if (n_args != k.n_args) {
      std::string names;
      for (int i = 0; i < k.n_args; ++i) names += std::string(i ? ", " : "") + k.args[i].name;
      ttnet::set_error("launch_partition %s takes %d arguments (%s), got %d", what, k.n_args, names.c_str(), n_args);
      return TTNET_E_INVALID;
    }
    if (out_cap < k.n_out) {
      ttnet::set_error("launch_partition %s writes %d values, out_cap is %d", what, k.n_out, out_cap);
      return TTNET_E_INVALID;
    }
    for (int i = 0; i < k.n_args; ++i) TT_TRY(check_arg(what, k.args[i], args[i]));
    I tmp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    TT_TRY(k.fn(args, tmp));
    for (int i = 0; i < k.n_out; ++i) out[i] = tmp[i];
    return k.n_out;
  }
  ttnet::set_error("launch_partition: unknown key %s", what);
  return TTNET_E_INVALID;
}
