"""Measurements of the truth-table minimiser (scale_imagenet_amd.minimise); the text goes to profiles/minimise_bench.txt.

  python tools/minimise_bench.py --quality           CPU only: literal counts against sympy's SOPform / POSform on the
                                                     x-small tables (n = 4) and seeded random functions of n = 6 and 8
  python tools/minimise_bench.py --device [--images N] [--sample K]
                                                     MI355X: device time to minimise every binarised table of TT-small
                                                     p = 64 --layers 1 (DNF and CNF, synthetic weights), with and without
                                                     the don't-cares of N synthetic images; cubes and literals per block;
                                                     the CPU twin on K functions per block in 16 processes beside it
  python tools/minimise_bench.py --rounds 0,1,2,4 [--quality] [--device] [--images N] [--repeats K]
                                                     the same two measurements per number of reduce / expand rounds (the text
                                                     goes to profiles/minimise_rounds_bench.txt): the literal ratios of
                                                     --quality for every round count; the time of the --device job (all
                                                     blocks, K alternating passes after a warm one, the best and the worst
                                                     pass) and its gate totals.  Rounds 0 is ttnet_minimise_covers itself.
"""
import argparse
import os
import sys
import time
from argparse import Namespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scale_imagenet_amd import export as E  # noqa: E402
from scale_imagenet_amd import minimise as M  # noqa: E402


def _twin_job(job):
    on, dc, n = job
    return len(M.minimise_cpu(on, dc, n))


def quality():
    def ratios(functions, n):
        out = []
        for on_b, dc_b in functions:
            if not on_b.any() or (on_b | dc_b).all() or not (~on_b & ~dc_b).any():
                continue
            on, dc = M.pack_bits(on_b), M.pack_bits(dc_b)
            ours = M.literal_total(M.minimise_cpu(on, dc, n)) + M.literal_total(M.minimise_cpu(M.complement(on, dc, n), dc, n))
            dnf, cnf = E.minimal_forms(np.flatnonzero(on_b).tolist(), n, np.flatnonzero(dc_b).tolist())
            out.append(ours / (E.literal_count(str(dnf)) + E.literal_count(str(cnf))))
        return np.array(out)

    for tag, n, fns in quality_sets():
        r = ratios(fns, n)
        print(f"{tag:<46} functions {len(r):4d}  literals ours / sympy: mean {r.mean():.3f}  median {np.median(r):.3f}  "
              f"min {r.min():.3f}  max {r.max():.3f}  p90 {np.quantile(r, 0.9):.3f}")


def quality_sets():
    """``[(tag, n, [(on flags, dc flags)])]``: the x-small tables and the seeded random functions of --quality."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from _util import spec_and_state
    from oracle import ttnet_bits as OB
    spec, st = spec_and_state("xsmall")
    fns = []
    for blk in spec.blocks:
        for b in (blk.conv1, blk.conv2, blk.conv3, blk.convf):
            if b.last or b.fan_in_bits != 4:
                continue
            table, _ = OB.build_lut(st, b)
            for g in range(table.shape[0]):
                for o in range(table.shape[2]):
                    fns.append((table[g, :, o] == 1, np.zeros(16, dtype=bool)))
    sets = [("x-small tables (n = 4, synthetic weights)", 4, fns)]
    for n, count in ((6, 200), (8, 40)):
        for p_on, p_dc in ((0.5, 0.0), (0.3, 0.4)):
            rng = np.random.default_rng(1000 * n + int(100 * p_dc))
            fns = []
            for _ in range(count):
                r = rng.random(1 << n)
                fns.append((r < p_on, (r >= p_on) & (r < p_on + p_dc)))
            sets.append((f"random n = {n}, ON {p_on:.0%}, don't-care {p_dc:.0%}", n, fns))
    return sets


def quality_rounds(rounds):
    """The ratios of ``quality`` for every round count: sympy minimises each function once."""
    for tag, n, fns in quality_sets():
        ours = {r: [] for r in rounds}
        theirs = []
        for on_b, dc_b in fns:
            if not on_b.any() or (on_b | dc_b).all() or not (~on_b & ~dc_b).any():
                continue
            on, dc = M.pack_bits(on_b), M.pack_bits(dc_b)
            dnf, cnf = E.minimal_forms(np.flatnonzero(on_b).tolist(), n, np.flatnonzero(dc_b).tolist())
            theirs.append(E.literal_count(str(dnf)) + E.literal_count(str(cnf)))
            for r in rounds:
                ours[r].append(M.literal_total(M.minimise_cpu(on, dc, n, r))
                               + M.literal_total(M.minimise_cpu(M.complement(on, dc, n), dc, n, r)))
        for r in rounds:
            q = np.array(ours[r]) / np.array(theirs)
            print(f"{tag:<46} rounds {r}  functions {len(q):4d}  literals ours / sympy: mean {q.mean():.3f}  median {np.median(q):.3f}  "
                  f"min {q.min():.3f}  max {q.max():.3f}  p90 {np.quantile(q, 0.9):.3f}  total {sum(ours[r])} / {sum(theirs)} = "
                  f"{sum(ours[r]) / sum(theirs):.3f}", flush=True)


def small_p64(images: int):
    """TT-small p = 64 --layers 1 on device 0 with synthetic weights and the table usage of ``images`` synthetic images."""
    import torch

    from scale_imagenet_amd import synth, ttnet
    from scale_imagenet_amd.spec import make_spec
    dev = torch.device("cuda", 0)
    spec = make_spec("small", 8, 8, 1)
    m = ttnet.TT_vf_19lv3_imgnet_small(Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(spec).items()}, strict=True)
    m = m.to(dev).eval().reserve(100)
    m.count_table_usage(True)
    with torch.no_grad():
        for first in range(0, images, 100):
            m(torch.from_numpy(synth.synth_images(min(100, images - first), first=first)).to(dev))
            m.add_table_usage(0)
    torch.cuda.synchronize()
    usage = m.table_usage()
    m.count_table_usage(False)
    print(f"TT-small p = 64 --layers 1, synthetic weights; don't-cares: entries not read by {images} synthetic images")
    return dev, spec, m, usage


def device_rounds(rounds, images: int, repeats: int):
    """Per round count: the time of the whole job (every binarised block, DNF + CNF of every filter, host time around
    ``minimise_device``, which ends in the copy back), on the whole tables and with don't-cares, and its gate totals.  One warm
    pass over every round count, then ``repeats`` passes that alternate the round counts."""
    import torch
    dev, spec, m, usage = small_p64(images)
    jobs = []
    for b in spec.block_tts():
        if b.last:
            continue
        table = m.get_table(b.name)
        for with_dc in (False, True):
            on, dc = M.pack_functions(table, usage[b.name] if with_dc else None)
            both_on, both_dc = np.concatenate([on, M.complement(on, dc, b.fan_in_bits)]), np.concatenate([dc, dc])
            jobs.append((with_dc, b.fan_in_bits, len(on), torch.from_numpy(both_on.view(np.int32)).to(dev),
                         torch.from_numpy(both_dc.view(np.int32)).to(dev)))
    times = {(r, d): [] for r in rounds for d in (False, True)}
    totals = {}
    for rep in range(repeats + 1):
        for r in rounds:
            spent = {False: 0.0, True: 0.0}
            row = {d: dict(functions=0, constant=0, cubes=0, literals=0) for d in (False, True)}
            for with_dc, n, f, on_t, dc_t in jobs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                covers = M.minimise_device(on_t, dc_t, n, dev, rounds=r)
                spent[with_dc] += (time.perf_counter() - t0) * 1e3
                if rep:
                    continue                                                    # the totals are the same in every pass
                for d, c in zip(covers[:f], covers[f:]):
                    row[with_dc]["functions"] += 2
                    if M.literal_total(d) == 0 or M.literal_total(c) == 0:
                        row[with_dc]["constant"] += 1
                        continue
                    row[with_dc]["cubes"] += len(d) + len(c)
                    row[with_dc]["literals"] += M.literal_total(d) + M.literal_total(c)
            print(f"pass {rep} rounds {r}: {spent[False]:.0f} ms whole tables, {spent[True]:.0f} ms with don't-cares", file=sys.stderr,
                  flush=True)
            if rep:
                for d in (False, True):
                    times[r, d].append(spent[d])
            else:
                totals[r] = row
    print(f"{'rounds':<8}{'dc':>4}{'functions':>10}{'constant':>9}{'cubes':>10}{'literals':>11}{'lits / rounds 0':>17}"
          f"{'best ms':>10}{'worst ms':>10}{'best / rounds 0':>17}   ({repeats} passes after a warm one, DNF + CNF, all blocks)")
    for d in (False, True):
        for r in rounds:
            t, base = totals[r][d], totals[rounds[0]][d]
            print(f"{r:<8}{'yes' if d else 'no':>4}{t['functions']:>10}{t['constant']:>9}{t['cubes']:>10}{t['literals']:>11}"
                  f"{t['literals'] / base['literals']:>17.4f}{min(times[r, d]):>10.0f}{max(times[r, d]):>10.0f}"
                  f"{min(times[r, d]) / min(times[rounds[0], d]):>17.2f}", flush=True)


def device(images: int, sample: int):
    import multiprocessing as mp

    import torch
    dev, spec, m, usage = small_p64(images)
    print(f"{'block':<24}{'dc':>3}{'functions':>10}{'device ms':>11}{'dnf cubes':>11}{'dnf lits':>11}{'cnf cubes':>11}{'cnf lits':>11}"
          f"{'constant':>9}{'twin s/function':>17}{'twin functions':>15}")
    pool = mp.get_context("spawn").Pool(16)
    total = {False: 0.0, True: 0.0}
    for b in spec.block_tts():
        if b.last:
            continue
        table = m.get_table(b.name)
        n = b.fan_in_bits
        for with_dc in (False, True):
            on, dc = M.pack_functions(table, usage[b.name] if with_dc else None)
            both_on, both_dc = np.concatenate([on, M.complement(on, dc, n)]), np.concatenate([dc, dc])
            on_t = torch.from_numpy(both_on.view(np.int32)).to(dev)
            dc_t = torch.from_numpy(both_dc.view(np.int32)).to(dev)
            M.minimise_device(on_t[:2], dc_t[:2], n, dev)                           # library and allocator warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            covers = M.minimise_device(on_t, dc_t, n, dev)                           # launches, the cap retry and the copy back
            ms = (time.perf_counter() - t0) * 1e3
            total[with_dc] += ms
            f = len(on)
            row = dict(constant=0, dnf_cubes=0, dnf_literals=0, cnf_cubes=0, cnf_literals=0)
            for d, c in zip(covers[:f], covers[f:]):
                if M.literal_total(d) == 0 or M.literal_total(c) == 0:
                    row["constant"] += 1
                    continue
                row["dnf_cubes"] += len(d)
                row["dnf_literals"] += M.literal_total(d)
                row["cnf_cubes"] += len(c)
                row["cnf_literals"] += M.literal_total(c)
            pick = np.linspace(0, 2 * f - 1, min(sample, 2 * f)).astype(int)
            t0 = time.perf_counter()
            sizes = pool.map(_twin_job, [(both_on[i], both_dc[i], n) for i in pick])
            twin = (time.perf_counter() - t0) / len(pick)                             # wall time per function with 16 at work
            assert sizes == [len(covers[i]) for i in pick], "the twin and the device disagree"
            print(f"{b.name:<24}{'yes' if with_dc else 'no':>3}{2 * f:>10}{ms:>11.1f}{row['dnf_cubes']:>11}{row['dnf_literals']:>11}"
                  f"{row['cnf_cubes']:>11}{row['cnf_literals']:>11}{row['constant']:>9}{twin:>17.4f}{len(pick):>15}", flush=True)
    pool.close()
    print(f"device, all blocks: {total[False]:.0f} ms on the whole tables, {total[True]:.0f} ms with don't-cares "
          "(host time around minimise_device: its launches, the second launch for covers above the first cap, the copies)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--rounds", type=str, default=None, metavar="R,R,..", help="report per number of reduce / expand rounds")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    rounds = None if a.rounds is None else [int(r) for r in a.rounds.split(",")]
    if a.quality:
        quality() if rounds is None else quality_rounds(rounds)
    if a.device:
        device(a.images, a.sample) if rounds is None else device_rounds(rounds, a.images, a.repeats)
