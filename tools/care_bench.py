"""What asking for the care-set misses costs: ttnet_care_misses behind a batch-256 forward, against the merged usage add
measured in the same run, on uniform and on skewed input, and evaluate() with the option off and on.

    python tools/care_bench.py [--batch 256] [--calls 20] [--windows 5] [--batches 40] [--inflight 2]
                               [--parent DIR] [--bench-runs 5] [--out profiles/care_bench.txt]

Legs (medians over the windows after a warm-up of each):
  1. forward alone, forward + care_misses and forward + the (merged) usage add, between HIP events around --calls
     back-to-back calls, the three alternated inside every window, on two inputs: the bench's synthetic images and a batch
     of constant images (every pixel of an image equal).  The care set is what the forward of a DIFFERENT synthetic batch
     reads, so most lookups of the synthetic images miss, and the constant images hit a handful of entries;
  2. the per-kernel split of one care_misses call (HIP events of the plan's profiling mode, plain launches);
  3. evaluate() on device-resident float batches, device metrics, --inflight lanes: care off against on;
  4. with --parent DIR (a checkout of the parent commit with its library built): `python bench.py --gpus 1 --steps 300
     --warmup 30` in DIR and in this tree, alternating (who goes first swaps with every pair), --bench-runs times each, care
     never enabled.
No number is promised: the output file records what was measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scale_imagenet_amd import minimise, synth  # noqa: E402
from scale_imagenet_amd.evaluate import evaluate  # noqa: E402
from table_usage_bench import _Quiet, constant_images, split_of_last_call  # noqa: E402  (tools/ is on the path of a script in it)


def bench_line(tree: str) -> dict:
    """The JSON line of one `python bench.py` run in ``tree`` (a fresh process: bench.py starts its own rank)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "300", "--warmup", "30"], cwd=tree,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    from _util import args_for, spec_and_state
    from scale_imagenet_amd import ttnet
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built (leg 4)")
    ap.add_argument("--bench-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "care_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"care_bench: TT-small p = 64 --layers 1, synthetic weights, batch {a.batch}, {a.calls} calls x {a.windows} windows, "
             f"{torch.cuda.get_device_name(dev)}", "command: python tools/care_bench.py " + " ".join(sys.argv[1:])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    inputs = {"synthetic images": torch.from_numpy(synth.synth_images(a.batch)).to(dev),
              "constant images": constant_images(a.batch).to(dev)}

    def forward(x):
        with torch.no_grad():
            model(x)

    # the care set: what another synthetic batch reads (counted once by the usage add, which then goes)
    model.count_table_usage(True)
    forward(torch.from_numpy(synth.synth_images(a.batch, first=10 * a.batch)).to(dev))
    model.add_table_usage(0)
    usage = model.table_usage()
    masks = minimise.care_masks(usage)
    model.set_care(masks)
    plan = model._any_plan()
    kept = sum(int((u > 0).sum()) for u in usage.values()) / sum(u.size for u in usage.values())
    say(f"   care set: the entries one other synthetic batch reads, {100 * kept:.2f} % of all entries; bitmaps "
        f"{plan.query('care_bytes') / 1e6:.1f} MB, counters + scratch {plan.query('usage_bytes') / 1e6:.0f} MB")

    def forward_care(x):
        forward(x)
        model.care_misses(0)

    def forward_add(x):
        forward(x)
        model.add_table_usage(0)

    legs = {"forward alone": forward, "forward + care_misses": forward_care, "forward + usage add (merged)": forward_add}

    def window(fn, x):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn(x)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    say("1. us per call (back-to-back between HIP events, launch gaps included); the three legs alternate inside every window: "
        "median (fastest .. slowest)")
    for tag, x in inputs.items():
        per = {k: [] for k in legs}
        for rep in range(a.windows + 1):
            for k, fn in legs.items():
                t = window(fn, x)
                if rep:                                     # (the first pass warms every leg)
                    per[k].append(t)
        med = {k: statistics.median(v) for k, v in per.items()}
        for k, v in per.items():
            extra = "" if k == "forward alone" else f"   extra = {med[k] - med['forward alone']:8.1f}"
            say(f"   {tag:<17} {k:<29} {med[k]:9.1f}   ({min(v):.1f} .. {max(v):.1f}){extra}")
        rows = model.care_misses(0).cpu()
        say(f"   {tag:<17} covered images {int((~rows.bool().any(dim=1)).sum())}/{a.batch}, lookups that miss "
            f"{100.0 * rows.sum().item() / (a.batch * sum(model.care_lookups().values())):.2f} %")
    model.count_table_usage(False)

    say("2. one care_misses call by kernel, ms (plain launches, HIP events per launch; care.tap = the fused blocks run again for "
        "their branch tensors, care.prep = layout conversions, care.dw = Block_conv1 + Block_conv2)")
    for tag, x in inputs.items():
        model.set_profiling(True)
        forward_care(x)
        torch.cuda.synchronize()
        sp = split_of_last_call(model)
        model.set_profiling(False)
        parts = "  ".join(f"{k} {v:.3f}" for k, v in sp.items() if k.startswith("care."))
        say(f"   {tag:<17} {parts}   | care total {sum(v for k, v in sp.items() if k.startswith('care.')):.3f}"
            f"   | forward {sum(v for k, v in sp.items() if not k.startswith('care.')):.3f}")

    pool = [torch.from_numpy(synth.synth_images(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    tpool = [torch.from_numpy(synth.synth_targets(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    batches = [(pool[i % 2], tpool[i % 2]) for i in range(a.batches)]
    images = a.batch * a.batches
    model.clear_care()
    cases = {"care off": {}, "care on": dict(care=masks)}
    times = {k: [] for k in cases}
    for rep in range(a.windows + 1):
        for k, kw in cases.items():
            t0 = time.perf_counter()
            with _Quiet():
                evaluate(model, batches, dev, inflight=a.inflight, metrics="device", **kw)
            if rep:
                times[k].append(time.perf_counter() - t0)
            model.clear_care()
    say(f"3. evaluate(), float batches on the device, metrics=device, inflight {a.inflight}, {a.batches} batches per window: median "
        "(slowest .. fastest) images/s; 'on' includes installing the bitmaps, a top-5 per image and the rows' copy to the host")
    for k, v in times.items():
        say(f"   {k:<16} {images / statistics.median(v):10.0f}   ({images / max(v):.0f} .. {images / min(v):.0f})")

    if a.parent:
        del model
        torch.cuda.empty_cache()
        say("4. python bench.py --gpus 1 --steps 300 --warmup 30, care never enabled, parent commit and this tree alternating in "
            "one session on the same box (images/s, ms per step):")
        got = {"parent": [], "this tree": []}
        trees = [("parent", a.parent), ("this tree", ROOT)]
        for i in range(a.bench_runs):
            for k, tree in trees[::-1] if i % 2 == 0 else trees:      # (the order swaps with every pair)
                d = bench_line(tree)
                got[k].append(d["value"])
                say(f"   {k:<10} {d['value']:12.0f}   {d.get('ms_per_step')}")
        p, t = got["parent"], got["this tree"]
        say(f"   this tree / parent = {statistics.mean(t) / statistics.mean(p):.4f} (means of {a.bench_runs} runs each); parent's own "
            f"spread (max - min) / mean = {(max(p) - min(p)) / statistics.mean(p):.4f}, this tree's {(max(t) - min(t)) / statistics.mean(t):.4f}")
    else:
        say("4. not run (--parent DIR was not given)")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
