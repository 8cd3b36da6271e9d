"""The CIFAR path of TT_FHE_XSMALL_vAlexnet on one MI355X: the uint8 stem against the float32 stem, both forwards, and a
whole 10,000-image evaluation from bytes on the device.

    python tools/cifar_bench.py [--batch 256] [--calls 200] [--window 0.5] [--windows 5] [--images 10000] [--repeats 5]
                                [--out profiles/cifar_bench.txt]

Legs, all in one process:
  1. device time of va.stem (float32 input) and va.stem_u8 (uint8 input) from ttnet_plan_last_timings with profiling on
     (plain launches, HIP events around each kernel), the two alternated call by call, --calls each after a warm-up:
     median and quartiles.  The float32 kernel is the yardstick: the uint8 stem is expected to be no slower than the
     float32 stem's median plus its own interquartile range in this run; the file says whether it was;
  2. forward and forward_u8 from device-resident inputs, graphs on, images/s over windows of at least --window seconds,
     the two alternated window by window;
  3. wall time of evaluate(metrics="device") over cifar.device_batches of --images synthetic images with labels, the one
     upload included, and that upload timed on its own.
Synthetic weights and images: no accuracy is measured here.  No number is promised: the file records what was measured.
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scale_imagenet_amd import cifar, synth, ttnet  # noqa: E402
from scale_imagenet_amd.evaluate import evaluate  # noqa: E402
from scale_imagenet_amd.spec import VAlexSpec  # noqa: E402


def quartiles(v):
    q1, q2, q3 = statistics.quantiles(v, n=4)
    return q1, q2, q3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cifar_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from argparse import Namespace
    model = ttnet.TT_FHE_XSMALL_vAlexnet(Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(VAlexSpec()).items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"cifar_bench: TT_FHE_XSMALL_vAlexnet, synthetic weights and images, batch {a.batch}, {torch.cuda.get_device_name(dev)}",
             "command: python tools/cifar_bench.py " + " ".join(sys.argv[1:])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    u8 = synth.synth_images_u8(a.batch, hw=(32, 32))
    mean, std = (np.asarray(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (cifar.CIFAR_MEAN, cifar.CIFAR_STD))
    xf = torch.from_numpy(((u8.astype(np.float32) / np.float32(255.0) - mean) / std).astype(np.float32)).to(dev)
    x8 = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 2, 3, 1))).to(dev)

    # 1. the two stem kernels, profiling on
    with torch.no_grad():
        model(xf)
        model.set_profiling(True)
        per = {"va.stem": [], "va.stem_u8": []}
        for i in range(a.calls + 20):
            for name, fn, x in (("va.stem", model, xf), ("va.stem_u8", model.forward_u8, x8)):
                fn(x)
                t = model.last_timings()[name] * 1e3
                if i >= 20:                                   # (warm-up)
                    per[name].append(t)
        split = model.last_timings()
        model.set_profiling(False)
    say(f"1. stem kernels, us of device time between HIP events, profiling on, alternated, {a.calls} calls each after 20 of warm-up: "
        "median (first quartile .. third quartile)")
    q = {k: quartiles(v) for k, v in per.items()}
    for k, (q1, q2, q3) in q.items():
        say(f"   {k:<11} {q2:8.2f}   ({q1:.2f} .. {q3:.2f})   min {min(per[k]):.2f}")
    f1, f2, f3 = q["va.stem"]
    bound = f2 + (f3 - f1)
    say(f"   expectation: va.stem_u8 median <= va.stem median + va.stem interquartile range = {f2:.2f} + {f3 - f1:.2f} = {bound:.2f}: "
        f"{'met' if q['va.stem_u8'][1] <= bound else 'NOT met'} ({q['va.stem_u8'][1]:.2f})")
    say("   one forward_u8 by kernel, us: " + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in split.items()))

    # 2. whole forwards, graphs on
    def window(fn, x):
        calls, t0 = 0, time.perf_counter()
        while True:
            for _ in range(50):
                fn(x)
            calls += 50
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            if dt >= a.window:
                return calls * a.batch / dt

    rates = {"forward (float32 input)": [], "forward_u8 (uint8 input)": []}
    with torch.no_grad():
        for rep in range(a.windows + 1):
            for (k, v), (fn, x) in zip(rates.items(), ((model, xf), (model.forward_u8, x8))):
                r = window(fn, x)
                if rep:                                       # (the first pass warms up and captures the graphs)
                    v.append(r)
    plan = model._any_plan()
    say(f"2. images/s from device-resident inputs, one lane, graphs on (graphs_enabled {plan.query('graphs_enabled')}, "
        f"{plan.query('graph_replays')} replays), windows of >= {a.window} s alternated, {a.windows} each: median (slowest .. fastest)")
    for k, v in rates.items():
        say(f"   {k:<26} {statistics.median(v):12.0f}   ({min(v):.0f} .. {max(v):.0f})")

    # 3. a whole evaluation from the bytes
    images = np.ascontiguousarray(synth.synth_images_u8(a.images, hw=(32, 32)).transpose(0, 2, 3, 1))
    targets = synth.synth_targets(a.images, n_classes=10)
    walls, uploads = [], []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        up = torch.from_numpy(images).to(dev)
        torch.cuda.synchronize(dev)
        t_up = time.perf_counter() - t0
        del up
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            res = evaluate(model, cifar.device_batches(images, targets, a.batch, dev), dev, inflight=a.inflight, metrics="device")
        t_all = time.perf_counter() - t0
        if rep:
            walls.append(t_all * 1e3)
            uploads.append(t_up * 1e3)
    assert res.images == a.images
    say(f"3. evaluate(metrics=device, inflight {a.inflight}) over cifar.device_batches, {a.images} images ({images.nbytes / 1e6:.1f} MB of "
        f"bytes) in batches of {a.batch}, wall ms with the one upload included, {a.repeats} runs after one of warm-up: median "
        f"{statistics.median(walls):.2f} ({min(walls):.2f} .. {max(walls):.2f}) = {a.images / statistics.median(walls) * 1e3:.0f} images/s")
    say(f"   the upload alone (pageable host memory, timed separately in the same runs): median {statistics.median(uploads):.2f} ms "
        f"({min(uploads):.2f} .. {max(uploads):.2f})")
    say("   accuracy on real CIFAR-10 is not measured: there is no trained checkpoint and no dataset on these machines")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
