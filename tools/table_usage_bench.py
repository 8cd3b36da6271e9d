"""What counting truth-table lookups costs: ttnet_table_usage_add behind a batch-256 forward, per histogram scheme, on
uniform and on skewed input, and evaluate() with the option off and on.

    python tools/table_usage_bench.py [--batch 256] [--calls 20] [--windows 5] [--batches 40] [--inflight 2]
                                      [--out profiles/table_usage_bench.txt]

Legs (medians over the windows after a warm-up of each):
  1. forward alone, then forward + add, between HIP events around --calls back-to-back pairs, for both histogram schemes
     (TTNET_USAGE_SCHEME=plain / merged, read when the counters are enabled) on two inputs: the bench's synthetic images
     (lookups spread over the tables) and a batch of constant images (every pixel of an image equal: whole rows of lookups
     on one counter);
  2. the per-kernel split of one add (HIP events of the plan's profiling mode, plain launches), same four cases;
  3. evaluate() on device-resident float batches, device metrics, --inflight lanes: table_usage off against on (the
     shipped scheme per table shape).
No number is promised: the output file records what was measured.  bench.py's own line, with counting never enabled, is
compared with the parent commit's by running both on the same box (appended to the file by hand).
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scale_imagenet_amd import _lib, synth  # noqa: E402
from scale_imagenet_amd.evaluate import evaluate  # noqa: E402


class _Quiet:
    def __enter__(self):
        self.out, sys.stdout = sys.stdout, open(os.devnull, "w")

    def __exit__(self, *exc):
        sys.stdout.close()
        sys.stdout = self.out


def constant_images(n: int) -> torch.Tensor:
    """Every pixel of an image equal; the grey levels walk the normalised range."""
    levels = torch.linspace(-2.1, 2.6, n)
    return levels.reshape(-1, 1, 1, 1).expand(-1, 3, 224, 224).contiguous()


def split_of_last_call(model):
    """{kernel name: ms} of the plan's last profiled forward + add, equal names summed."""
    plan = model._any_plan()
    cap = 128
    names, ms = (C.c_char_p * cap)(), (C.c_float * cap)()
    k = _lib.check(plan.lib.ttnet_plan_last_timings(plan.handle, names, ms, cap))
    out = {}
    for i in range(k):
        out[names[i].decode()] = out.get(names[i].decode(), 0.0) + float(ms[i])
    return out


def main():
    from _util import args_for, spec_and_state
    from scale_imagenet_amd import ttnet
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_usage_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"table_usage_bench: TT-small p = 64 --layers 1, synthetic weights, batch {a.batch}, {a.calls} calls x {a.windows} windows, "
             f"{torch.cuda.get_device_name(dev)}", "command: python tools/table_usage_bench.py " + " ".join(sys.argv[1:])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    inputs = {"synthetic images": torch.from_numpy(synth.synth_images(a.batch)).to(dev),
              "constant images": constant_images(a.batch).to(dev)}

    def timed(fn):
        for _ in range(4):
            fn()
        per = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        return statistics.median(per)

    def forward(x):
        with torch.no_grad():
            model(x)

    def forward_add(x):
        forward(x)
        model.add_table_usage(0)

    say("1. forward and forward + add, us per call (back-to-back between HIP events, launch gaps included)")
    alone = {tag: timed(lambda x=x: forward(x)) for tag, x in inputs.items()}
    for tag, t in alone.items():
        say(f"   forward alone, {tag:<17}            {t:9.1f}")
    splits = {}
    for scheme in ("plain", "merged"):
        os.environ["TTNET_USAGE_SCHEME"] = scheme
        model.count_table_usage(True)
        if scheme == "plain":
            say(f"   (counters + scratch: {model._any_plan().query('usage_bytes') / 1e6:.0f} MB)")
        for tag, x in inputs.items():
            t = timed(lambda x=x: forward_add(x))
            say(f"   forward + add, {tag:<17} {scheme:<7}    {t:9.1f}   add = {t - alone[tag]:9.1f}")
            model.set_profiling(True)
            forward_add(x)
            torch.cuda.synchronize()
            splits[(scheme, tag)] = split_of_last_call(model)
            model.set_profiling(False)
        model.count_table_usage(False)
    del os.environ["TTNET_USAGE_SCHEME"]
    say("2. one add by kernel, ms (plain launches, HIP events per launch; usage.tap = the fused blocks run again for their "
        "branch tensors, usage.prep = layout conversions, usage.dw = Block_conv1 + Block_conv2)")
    for (scheme, tag), sp in splits.items():
        parts = "  ".join(f"{k} {v:.3f}" for k, v in sp.items() if k.startswith("usage."))
        say(f"   {scheme:<7} {tag:<17} {parts}   | forward {sum(v for k, v in sp.items() if not k.startswith('usage.')):.3f}")

    # 3. evaluate() with and without the option (shipped schemes)
    pool = [torch.from_numpy(synth.synth_images(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    tpool = [torch.from_numpy(synth.synth_targets(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    batches = [(pool[i % 2], tpool[i % 2]) for i in range(a.batches)]
    images = a.batch * a.batches
    legs = {"table_usage off": {}, "table_usage on": dict(table_usage=True)}
    times = {k: [] for k in legs}
    for rep in range(a.windows + 1):
        for k, kw in legs.items():
            t0 = time.perf_counter()
            with _Quiet():
                evaluate(model, batches, dev, inflight=a.inflight, metrics="device", **kw)
            if rep:                                         # (the first pass warms plans, graphs and counters)
                times[k].append(time.perf_counter() - t0)
    say(f"3. evaluate(), float batches on the device, metrics=device, inflight {a.inflight}, {a.batches} batches per window: median "
        "(slowest .. fastest) images/s; 'on' includes reading 543 MB of counters back at the end of every window")
    for k, v in times.items():
        say(f"   {k:<16} {images / statistics.median(v):10.0f}   ({images / max(v):.0f} .. {images / min(v):.0f})")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
