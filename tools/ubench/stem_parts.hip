// Additive decomposition of stem_pc_kernel (stem.hip): the same kernel built with parts switched off
// (TT_STEM_SKIP) and, with -DTT_STEM_STAMP, s_memtime stamps of every period of both roles; random
// input, timed with HIP events.
//   stem_parts_<name> [images [launches [1 = all-zero input]]]      (TTNET_STEM_GRID=128: the half-chip launch)
//   hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fno-slp-vectorize -DTT_STEM_SKIP=<mask> [-DTT_STEM_STAMP] -o stem_parts_<mask> stem_parts.hip
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#include "../../scale_imagenet_amd/csrc/stem.hip"

namespace ttnet {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
float weight_prescale(const float *w, size_t n) {
  float amax = 0.f;
  for (size_t i = 0; i < n; ++i) amax = fmaxf(amax, fabsf(w[i]));
  int e;
  frexpf(amax, &e);
  return ldexpf(1.0f, 14 - e);
}
int ensure_dynamic_lds(const void *kernel, size_t bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess ? 0 : -3;
}
}  // namespace ttnet

int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 256;

  const size_t xe = (size_t)n * 3 * 224 * 224;
  float *x;
  uint64_t *rp;
  uint16_t *wf;
  float *init;
  uint32_t *flag;
  hipMalloc(&x, xe * 4); hipMalloc(&rp, (size_t)n * 64 * 56 * 8); hipMalloc(&wf, ttnet::stem_split_weights_elems() * 2);
  hipMalloc(&init, 256); hipMalloc(&flag, 4);
  hipMemset(flag, 0, 4);
  std::vector<float> h(xe);
  uint64_t s = 88172645463325252ull;
  for (auto &v : h) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = ((float)(s & 0xFFFF) / 65536.f - 0.5f) * 4.f; }
  if (argc > 3 && atoi(argv[3]) == 1) std::fill(h.begin(), h.end(), 0.f);      // zero input: what the clock does without operand toggling
  hipMemcpy(x, h.data(), xe * 4, hipMemcpyHostToDevice);
  std::vector<float> w(64 * 147);
  std::vector<double> sc(64, 1.0), sh(64, 0.01);
  for (auto &v : w) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = ((float)(s & 0xFFFF) / 65536.f - 0.5f) * 0.16f; }
  std::vector<uint16_t> wfh(ttnet::stem_split_weights_elems());
  std::vector<float> inith(64);
  ttnet::stem_split_weights(w.data(), sc.data(), sh.data(), 64, wfh.data(), inith.data());
  hipMemcpy(wf, wfh.data(), wfh.size() * 2, hipMemcpyHostToDevice);
  hipMemcpy(init, inith.data(), 256, hipMemcpyHostToDevice);
  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  for (int i = 0; i < 5; ++i) ttnet::launch_stem(x, false, nullptr, wf, init, rp, nullptr, n, 64, flag, 0);
  hipDeviceSynchronize();
  const int reps = argc > 2 && atoi(argv[2]) > 0 ? atoi(argv[2]) : 50;      // (long runs: the clock settles only after a second or two of load)
  hipEventRecord(e0, 0);
  for (int i = 0; i < reps; ++i) ttnet::launch_stem(x, false, nullptr, wf, init, rp, nullptr, n, 64, flag, 0);
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  printf("skip=%d n=%d: %.2f us per launch\n", TT_STEM_SKIP, n, 1e3 * ms / reps);
#ifdef TT_STEM_STAMP
  // TTNET_STEM_GRID=<g> forces the grid (launch_stem reads it): the half-chip regime of the plan with two batches in flight is g = 128
  const int grid = std::min(n * 7, getenv("TTNET_STEM_GRID") && atoi(getenv("TTNET_STEM_GRID")) > 0 ? atoi(getenv("TTNET_STEM_GRID")) : 256);
  const int items = (int)(1ll * n * 7 / grid);                                    // of block 0
  static unsigned long long st[256][2][ttnet::STAMP_SLOTS], dt[256][2][ttnet::STAMP_ITEMS][4];
  hipMemcpyFromSymbol(st, HIP_SYMBOL(ttnet::g_stem_stamps), sizeof(st));
  hipMemcpyFromSymbol(dt, HIP_SYMBOL(ttnet::g_stem_detail), sizeof(dt));
  const int slots = std::min(ttnet::STAMP_SLOTS, 3 + items + 1), its = std::min(ttnet::STAMP_ITEMS, items);
  for (int b : {0, 1, grid / 2, grid - 1}) {
    for (int role = 0; role < 2; ++role) {
      // slot 0: start, 1 / 2: after barrier 1 / end of the prologue pass (producers), 2: after barrier 2 (consumers), 3 + j: arrival at the barrier of period j
      printf("block %3d %s:", b, role ? "prod" : "cons");
      for (int j = 1; j < slots; ++j) printf(" %6lld", st[b][role][j] ? (long long)(st[b][role][j] - st[b][1][0]) : -1ll);
      printf("\n");
    }
    // per item and consumer wave (0: four units, 4: three units of the same SIMD): released -> first fragment landed, -> unit loop done,
    // -> at the barrier; then how long the wave waited there (release of the next item - arrival)
    for (int w = 0; w < 2; ++w) {
      printf("block %3d wave %d [first mfma, loop, arrive, wait]:", b, 4 * w);
      for (int j = 0; j < its; ++j) {
        const unsigned long long *d = dt[b][w][j];
        const long long wait = j + 1 < its ? (long long)(dt[b][w][j + 1][0] - d[3]) : -1;
        printf(" [%lld %lld %lld %lld]", (long long)(d[1] - d[0]), (long long)(d[2] - d[0]), (long long)(d[3] - d[0]), wait);
      }
      printf("\n");
    }
  }
  // medians over the workgroups: period of a steady item (release to release, wave 0), and its parts
  {
    std::vector<long long> per, first, loop, arr, wait0, wait4, prodlead;
    for (int b = 0; b < grid; ++b)
      for (int j = 1; j + 1 < its; ++j) {
        per.push_back((long long)(dt[b][0][j + 1][0] - dt[b][0][j][0]));
        first.push_back((long long)(dt[b][0][j][1] - dt[b][0][j][0]));
        loop.push_back((long long)(dt[b][0][j][2] - dt[b][0][j][0]));
        arr.push_back((long long)(dt[b][0][j][3] - dt[b][0][j][0]));
        wait0.push_back((long long)(dt[b][0][j + 1][0] - dt[b][0][j][3]));
        wait4.push_back((long long)(dt[b][1][j + 1][0] - dt[b][1][j][3]));
        // producers' arrival at the barrier of period j before (+) or after (-) consumer wave 0's
        if (3 + j < ttnet::STAMP_SLOTS) prodlead.push_back((long long)(st[b][0][3 + j] - st[b][1][3 + j]));
      }
    auto med = [](std::vector<long long> &v) -> long long {
      if (v.empty()) return -1;
      std::sort(v.begin(), v.end());
      return v[v.size() / 2];
    };
    printf("median over %d workgroups, steady items: period %lld | wave 0: first mfma %lld, loop %lld, arrive %lld, wait %lld | wave 4 wait %lld | "
           "producers ahead of wave 0 at the barrier %lld\n",
           grid, med(per), med(first), med(loop), med(arr), med(wait0), med(wait4), med(prodlead));
  }
#endif
  return 0;
}
