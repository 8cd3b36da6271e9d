"""What the robustness certificate of TT_FHE_XSMALL_vAlexnet costs on one MI355X, next to the forward of the same run.

    python tools/certify_bench.py [--batch 256] [--calls 100] [--images 10000] [--repeats 5] [--out profiles/certify_bench.txt]

Legs, all in one process:
  1. device time of the four steps of ttnet_certify_u8 (stem planes, block planes, interval margin, enumeration) at --batch
     for eps in {0.03, 1, 2}, from ttnet_plan_last_timings with profiling on (plain launches, HIP events around each step),
     and the kernels of forward_u8 measured the same way in the same loop: medians over --calls after a warm-up;
  2. wall time of certify_batches over --images device-resident synthetic images at the three eps (one pass), next to
     evaluate(metrics="device") over the same bytes, alternated.
No speed threshold is set in advance: the file records what was measured.  Synthetic weights and images: the certified shares
say nothing about a trained network.
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scale_imagenet_amd import certify, cifar, synth, ttnet  # noqa: E402
from scale_imagenet_amd.evaluate import evaluate  # noqa: E402
from scale_imagenet_amd.spec import VAlexSpec  # noqa: E402

EPS = (0.03, 1.0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = ttnet.TT_FHE_XSMALL_vAlexnet(Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(VAlexSpec()).items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"certify_bench: TT_FHE_XSMALL_vAlexnet, SYNTHETIC weights and images, batch {a.batch}, {torch.cuda.get_device_name(dev)}",
             "command: python tools/certify_bench.py " + " ".join(sys.argv[1:]),
             "the certified shares below come from synthetic weights: they say nothing about a trained network (no checkpoint, no dataset here)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    x8 = torch.from_numpy(np.ascontiguousarray(synth.synth_images_u8(a.batch, hw=(32, 32)).transpose(0, 2, 3, 1))).to(dev)
    with torch.no_grad():
        cls = model.forward_u8(x8).argmax(dim=1).to(torch.int32)          # certify the device's own top-1

    # 1. per step, profiling on
    per = {eps: {} for eps in EPS}
    fwd = {}
    with torch.no_grad():
        model.set_profiling(True)
        for i in range(a.calls + 10):
            model.forward_u8(x8)
            for k, v in model.last_timings().items():
                if i >= 10:
                    fwd.setdefault(k, []).append(v * 1e3)
            for eps in EPS:
                model.certify_u8(x8, cls, eps)
                for k, v in model.last_timings().items():
                    if i >= 10:
                        per[eps].setdefault(k, []).append(v * 1e3)
        model.set_profiling(False)
        shares = {eps: certify.summarise(eps, model.certify_u8(x8, cls, eps).numpy()) for eps in EPS}
    say(f"1. device time per step, us between HIP events, profiling on, batch {a.batch}, median of {a.calls} calls after 10 of warm-up "
        "(forward_u8 and the three eps alternated call by call)")
    med = {k: statistics.median(v) for k, v in fwd.items()}
    say("   forward_u8      " + "  ".join(f"{k} {v:.1f}" for k, v in med.items()) + f"   sum {sum(med.values()):.1f}")
    for eps in EPS:
        med = {k: statistics.median(v) for k, v in per[eps].items()}
        s = shares[eps]
        say(f"   certify eps={eps:<5g}" + "  ".join(f"{k} {v:.1f}" for k, v in med.items()) + f"   sum {sum(med.values()):.1f}"
            f"   [certified {s['certified']}/{s['images']}: interval {s['interval']}, enumeration {s['enumeration']}; unknown stem bits "
            f"median {s['unknown_stem_median']:g} max {s['unknown_stem_max']}]")

    # 2. a whole pass from device-resident bytes
    images = np.ascontiguousarray(synth.synth_images_u8(a.images, hw=(32, 32)).transpose(0, 2, 3, 1))
    xd = torch.from_numpy(images).to(dev)
    with torch.no_grad():
        labels = torch.cat([model.forward_u8(xd[i:i + a.batch]).argmax(dim=1) for i in range(0, a.images, a.batch)])
    batches = [(xd[i:i + a.batch], labels[i:i + a.batch]) for i in range(0, a.images, a.batch)]
    t_cert, t_eval = [], []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sums = certify.certify_batches(model, batches, EPS)               # (ends in the copy of the records to the host)
        t1 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            evaluate(model, batches, dev, inflight=1, metrics="device")
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if rep:
            t_cert.append((t1 - t0) * 1e3)
            t_eval.append((t2 - t1) * 1e3)
    mc, me = statistics.median(t_cert), statistics.median(t_eval)
    say(f"2. {a.images} device-resident images in batches of {a.batch}, wall ms, {a.repeats} runs after one of warm-up, alternated: median "
        "(fastest .. slowest)")
    say(f"   certify_batches at eps {', '.join(f'{e:g}' for e in EPS)} (three certificates per image, records copied to the host): "
        f"{mc:.2f} ({min(t_cert):.2f} .. {max(t_cert):.2f}) = {len(EPS) * a.images / mc * 1e3:.0f} certificates/s")
    say(f"   evaluate(metrics=device, inflight 1) over the same batches: {me:.2f} ({min(t_eval):.2f} .. {max(t_eval):.2f}) = "
        f"{a.images / me * 1e3:.0f} images/s; one certificate costs {mc / len(EPS) / me:.2f} forwards")
    for s in sums:
        say("   " + certify.verified_line(s) + "   [synthetic weights, the device's own top-1 as the class]")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
