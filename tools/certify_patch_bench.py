"""What the patch sweep of TT_FHE_XSMALL_vAlexnet costs on one MI355X: ttnet_certify_patch_u8 next to the same boxes pushed through
ttnet_certify_box_u8 (the non-incremental way), to one ttnet_certify_u8 and to the forward, all in one process.

    python tools/certify_patch_bench.py [--batch 256] [--calls 100] [--box_passes 3] [--images 10000] [--out profiles/certify_patch_bench.txt]

Legs:
  1. device time of "patch.base" and "patch.sweep" at --batch for 1x1, 2x2, 4x4 (stride 1, amp 255) and 4x4 / amp 1, from
     ttnet_plan_last_timings with profiling on (HIP events around each step), with forward_u8 and certify_u8 (eps 1) in the same
     loop: medians over --calls after a warm-up;
  2. the same --batch x P boxes through certify_box_u8, one call of --batch boxes per position (the boxes are built on the device
     outside the timed steps): sum of the steps' device time over a whole pass, median of --box_passes passes;
  3. wall time of certify_patch_batches (1x1, amp 255) over --images device-resident synthetic images.
No speed threshold is set in advance: the file records what was measured.  Synthetic weights and images: the certified shares
say nothing about a trained network.
"""
import argparse
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scale_imagenet_amd import certify, synth, ttnet  # noqa: E402
from scale_imagenet_amd.spec import VAlexSpec  # noqa: E402

SWEEPS = (((1, 1), 255), ((2, 2), 255), ((4, 4), 255), ((4, 4), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--box_passes", type=int, default=3)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certify_patch_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = ttnet.TT_FHE_XSMALL_vAlexnet(Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(VAlexSpec()).items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"certify_patch_bench: TT_FHE_XSMALL_vAlexnet, SYNTHETIC weights and images, batch {a.batch}, {torch.cuda.get_device_name(dev)}",
             "command: python tools/certify_patch_bench.py " + " ".join(sys.argv[1:]),
             "the certified shares below come from synthetic weights: they say nothing about a trained network (no checkpoint, no dataset here)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    x8 = torch.from_numpy(np.ascontiguousarray(synth.synth_images_u8(a.batch, hw=(32, 32)).transpose(0, 2, 3, 1))).to(dev)
    with torch.no_grad():
        cls = model.forward_u8(x8).argmax(dim=1).to(torch.int32)          # certify the device's own top-1

    # 1. the sweep per step, profiling on
    per = {k: {} for k in SWEEPS}
    fwd, cert = {}, {}
    with torch.no_grad():
        model.set_profiling(True)
        for i in range(a.calls + 5):
            for fn, into in ((lambda: model.forward_u8(x8), fwd), (lambda: model.certify_u8(x8, cls, 1.0), cert)):
                fn()
                for k, v in model.last_timings().items():
                    if i >= 5:
                        into.setdefault(k, []).append(v * 1e3)
            for key in SWEEPS:
                model.certify_patch_u8(x8, cls, key[0], 1, key[1])
                for k, v in model.last_timings().items():
                    if i >= 5:
                        per[key].setdefault(k, []).append(v * 1e3)
    t_fwd = sum(statistics.median(v) for v in fwd.values())
    t_cert = sum(statistics.median(v) for v in cert.values())
    say(f"1. device time, us between HIP events, profiling on, batch {a.batch}, median of {a.calls} calls after 5 of warm-up (forward_u8, "
        "certify_u8 and the four sweeps alternated call by call)")
    say(f"   forward_u8 {t_fwd:.1f}   certify_u8 eps=1 " + "  ".join(f"{k} {statistics.median(v):.1f}" for k, v in cert.items()) + f"   sum {t_cert:.1f}")
    sweep_us = {}
    for key in SWEEPS:
        (h, w), amp = key
        med = {k: statistics.median(v) for k, v in per[key].items()}
        rows, maps = model.certify_patch_u8(x8, cls, key[0], 1, amp).numpy()
        s = certify.summarise_patch(key[0], 1, amp, rows, maps)
        P = maps[0].size
        sweep_us[key] = med["patch.sweep"]
        say(f"   sweep {h}x{w} amp {amp:<3d} P={P:<4d} " + "  ".join(f"{k} {v:.1f}" for k, v in med.items()) +
            f"   = {1e3 * med['patch.sweep'] / (a.batch * P):.1f} ns per (image, position); one certify_u8 per image costs {1e3 * t_cert / a.batch:.0f} ns"
            f"   [{s['certified']}/{s['images']} images patch-certified, positions {s['positions_certified']}/{s['positions']}: interval "
            f"{s['interval']}, enumeration {s['enumeration']}; unknown stem bits median {s['unknown_stem_median']:g} max {s['unknown_stem_max']}]")

    # 2. the same boxes through the box certificate, a call per position
    say(f"2. the same {a.batch} x P boxes through certify_box_u8, one call of {a.batch} boxes per position, boxes built on the device outside "
        f"the timed steps: sum of certify.* device time over a pass, median of {a.box_passes} passes")
    xi = x8.to(torch.int16)
    with torch.no_grad():
        for key in SWEEPS:
            (h, w), amp = key
            org = certify.patch_origins(key[0], 1)
            totals = []
            agree = True
            for rep in range(a.box_passes):
                total = 0.0
                for p, (y0, x0) in enumerate(org):
                    lo, hi = x8.clone(), x8.clone()
                    lo[:, y0:y0 + h, x0:x0 + w] = (xi[:, y0:y0 + h, x0:x0 + w] - amp).clamp(0, 255).to(torch.uint8)
                    hi[:, y0:y0 + h, x0:x0 + w] = (xi[:, y0:y0 + h, x0:x0 + w] + amp).clamp(0, 255).to(torch.uint8)
                    res = certify.certify_box_u8(model, lo, hi, cls, check_order=False)
                    total += sum(model.last_timings().values()) * 1e3
                    if rep == 0 and p % 97 == 0:                          # a spot check that both ways speak of the same boxes
                        maps = model.certify_patch_u8(x8, cls, key[0], 1, amp).numpy()[1].reshape(a.batch, -1)
                        agree &= bool(np.array_equal(res.numpy()["stage"], maps[:, p]["stage"]))
                totals.append(total)
            t_box = statistics.median(totals)
            say(f"   boxes {h}x{w} amp {amp:<3d} P={len(org):<4d} {t_box:.0f} us a pass = {1e3 * t_box / (a.batch * len(org)):.1f} ns per (image, position); "
                f"the sweep takes {sweep_us[key]:.0f} us: {t_box / sweep_us[key]:.1f} x less   [stages agree on the positions compared: {agree}]")
        model.set_profiling(False)

    # 3. a whole pass from device-resident bytes
    images = np.ascontiguousarray(synth.synth_images_u8(a.images, hw=(32, 32)).transpose(0, 2, 3, 1))
    xd = torch.from_numpy(images).to(dev)
    with torch.no_grad():
        labels = torch.cat([model.forward_u8(xd[i:i + a.batch]).argmax(dim=1) for i in range(0, a.images, a.batch)])
    batches = [(xd[i:i + a.batch], labels[i:i + a.batch]) for i in range(0, a.images, a.batch)]
    walls = []
    for rep in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        sums = certify.certify_patch_batches(model, batches, [(1, 1)], 1, 255)    # (ends in the copy of the records to the host)
        walls.append((time.perf_counter() - t0) * 1e3)
    say(f"3. {a.images} device-resident images in batches of {a.batch}, 1x1 / amp 255 / stride 1 (1,024 positions each), records and maps "
        f"copied to the host: wall ms of three passes {', '.join(f'{t:.1f}' for t in walls)} = {a.images * 1024 / min(walls) * 1e3 / 1e6:.1f} M "
        "(image, position) certificates/s in the fastest")
    say("   " + certify.patch_line(sums[0]) + "   [synthetic weights, the device's own top-1 as the class]")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
