"""Measurements of the rule support pass (scale_imagenet_amd.rules, csrc/rules.hip); the text goes to profiles/rules_bench.txt.

  python tools/rules_bench.py [--images N] [--sample K]
      one MI355X, TT-small p = 64 --layers 1, synthetic weights, the table usage of N (256) synthetic images.  Per binarised
      block, for the DNF + CNF covers of every filter (minimised with the entries never read as don't-cares):
        minimise ms      host time around minimise_device for those functions, in the same run (as tools/minimise_bench.py)
        support ms       device time of ttnet_cover_support, HIP events, median of 5: every cube kept and no lost_bits; with
                         lost_bits; and pruned (keep flags from --share, lost_bits given), where every pattern is walked
        twin s           cover_support_cpu on a fixed sample of K (8) functions of the block, extrapolated to all of them
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from minimise_bench import small_p64  # noqa: E402
from scale_imagenet_amd import _lib  # noqa: E402
from scale_imagenet_amd import minimise as M  # noqa: E402
from scale_imagenet_amd import rules as R  # noqa: E402


def device_ms(call, repeats: int = 5) -> float:
    import torch
    call()                                                           # warm
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main(images: int, sample: int, share: float):
    import torch
    dev, spec, m, usage = small_p64(images)
    lib = _lib.load()
    print(f"{'block':<24}{'functions':>10}{'cubes':>9}{'max cover':>10}{'used patterns':>14}{'minimise ms':>12}{'support ms':>11}"
          f"{'+ lost_bits':>12}{'pruned':>9}{'cubes kept':>11}{'twin s (all)':>13}{'twin functions':>15}")
    total = dict(minimise=0.0, plain=0.0, bits=0.0, pruned=0.0, twin=0.0)
    for b in spec.block_tts():
        if b.last:
            continue
        n = b.fan_in_bits
        on, dc = M.pack_functions(m.get_table(b.name), usage[b.name])
        both_on, both_dc = np.concatenate([on, M.complement(on, dc, n)]), np.concatenate([dc, dc])
        on_t, dc_t = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (both_on, both_dc))
        M.minimise_device(on_t[:2], dc_t[:2], n, dev)                # library and allocator warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        covers = M.minimise_device(on_t, dc_t, n, dev)
        t_min = (time.perf_counter() - t0) * 1e3
        f = len(covers)
        rows = np.tile(np.repeat(np.arange(b.groups, dtype=np.int32), b.cout_g), 2)
        plain = R.cover_support(covers, usage[b.name], rows, n, device=dev)
        keep = R.keep_by_support(plain, min_share=share)
        counts = np.array([len(c) for c in covers], dtype=np.int32)
        cap = max(int(counts.max()), 1)
        packed, flags = np.zeros((f, cap), dtype=np.uint32), np.zeros((f, cap), dtype=np.uint8)
        for i, (c, k) in enumerate(zip(covers, keep)):
            packed[i, : len(c)], flags[i, : len(c)] = c, k
        t = lambda a: torch.from_numpy(a).to(dev)                    # noqa: E731
        cubes_t, counts_t, keep_t, usage_t, rows_t = t(packed.view(np.int32)), t(counts), t(flags), t(usage[b.name]), t(rows)
        out = torch.empty((3, f, cap), dtype=torch.int64, device=dev)
        totals_t = torch.empty((f, 4), dtype=torch.int64, device=dev)
        lost_t = torch.empty((f, M.n_words(n)), dtype=torch.int32, device=dev)
        work = torch.empty(_lib.check(lib.ttnet_cover_support_workspace(n, f)), dtype=torch.uint8, device=dev)
        run = lambda kp, lost: R.launch_cover_support(cubes_t, counts_t, kp, usage_t, rows_t, n, out[0], out[1], out[2], totals_t,  # noqa: E731
                                                      lost, work)
        ms = [device_ms(lambda: run(None, None)), device_ms(lambda: run(None, lost_t)), device_ms(lambda: run(keep_t, lost_t))]
        pick = np.linspace(0, f - 1, min(sample, f)).astype(int)
        t0 = time.perf_counter()
        twin = R.cover_support_cpu([covers[i] for i in pick], usage[b.name], rows[pick], n)
        t_twin = (time.perf_counter() - t0) / len(pick) * f
        for key in ("hits", "first", "sole"):
            assert all(np.array_equal(twin[key][j], plain[key][i]) for j, i in enumerate(pick)), "the twin and the device disagree"
        used = int(np.count_nonzero(usage[b.name]) / b.groups)
        print(f"{b.name:<24}{f:>10}{int(counts.sum()):>9}{cap:>10}{used:>14}{t_min:>12.1f}{ms[0]:>11.3f}{ms[1]:>12.3f}{ms[2]:>9.3f}"
              f"{int(sum(k.sum() for k in keep)):>11}{t_twin:>13.1f}{len(pick):>15}", flush=True)
        for key, v in zip(("minimise", "plain", "bits", "pruned", "twin"), (t_min, *ms, t_twin)):
            total[key] += v
    print(f"all blocks: minimise {total['minimise']:.0f} ms (host time around minimise_device); support {total['plain']:.1f} ms, "
          f"{total['bits']:.1f} ms with lost_bits, {total['pruned']:.1f} ms pruned at share {share:g} (device time); numpy twin "
          f"{total['twin']:.0f} s extrapolated from {sample} functions per block (one process)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--share", type=float, default=1e-4, help="the pruning share of the third support column")
    a = ap.parse_args()
    main(a.images, a.sample, a.share)
