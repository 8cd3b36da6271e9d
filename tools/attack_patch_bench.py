"""What the patch search of TT_FHE_XSMALL_vAlexnet costs on one MI355X: ttnet_attack_patch_u8 next to the certified sweep
(ttnet_certify_patch_u8) and the forward, all in one process.

    python tools/attack_patch_bench.py [--batch 256] [--calls 10] [--images 10000] [--out profiles/attack_patch_bench.txt]

Legs:
  1. device time of "patch.attack" at --batch for 1x1, 2x2, 4x4 (stride 1, amp 255) and 4x4 / amp 1 at two rounds, from
     ttnet_plan_last_timings with profiling on (HIP events around each step), with "patch.sweep" and forward_u8 in the same loop:
     medians over --calls after a warm-up; the same search at one and four rounds, and how many positions were searched at all;
  2. the confirm forwards: wall time of attack_patch_u8 with confirm = none, best and all at --batch, and how many forwards ran;
  3. wall time of attack_patch_batches and certify_patch_batches over --images device-resident synthetic images, and the bracket.
No speed threshold is set in advance: the file records what was measured.  Synthetic weights and images: the counts say nothing
about a trained network.
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

from scale_imagenet_amd import attack, certify, synth, ttnet  # noqa: E402
from scale_imagenet_amd.spec import VAlexSpec  # noqa: E402

SEARCHES = (((1, 1), 255), ((2, 2), 255), ((4, 4), 255), ((4, 4), 1))
MIN_MARGIN = 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attack_patch_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = ttnet.TT_FHE_XSMALL_vAlexnet(Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(VAlexSpec()).items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"attack_patch_bench: TT_FHE_XSMALL_vAlexnet, SYNTHETIC weights and images, batch {a.batch}, {torch.cuda.get_device_name(dev)}",
             "command: python tools/attack_patch_bench.py " + " ".join(sys.argv[1:]),
             "the counts below come from synthetic weights: they say nothing about a trained network (no checkpoint, no dataset here)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    x8 = torch.from_numpy(np.ascontiguousarray(synth.synth_images_u8(a.batch, hw=(32, 32)).transpose(0, 2, 3, 1))).to(dev)
    with torch.no_grad():
        cls = model.forward_u8(x8).argmax(dim=1).to(torch.int32)          # the device's own top-1 as the class

    # 1. the search per step, profiling on
    per = {(k, r): {} for k in SEARCHES for r in (1, 2, 4)}
    sweep = {k: {} for k in SEARCHES}
    fwd = {}
    with torch.no_grad():
        model.set_profiling(True)
        for i in range(a.calls + 2):
            model.forward_u8(x8)
            for k, v in model.last_timings().items():
                if i >= 2:
                    fwd.setdefault(k, []).append(v * 1e3)
            for key in SEARCHES:
                model.certify_patch_u8(x8, cls, key[0], 1, key[1], min_margin=MIN_MARGIN)
                for k, v in model.last_timings().items():
                    if i >= 2:
                        sweep[key].setdefault(k, []).append(v * 1e3)
                for r in (2,) if i < a.calls else (1, 2, 4):              # (one and four rounds: the last two calls only)
                    attack.patch_search_u8(model, x8, cls, key[0], 1, key[1], r, MIN_MARGIN)
                    for k, v in model.last_timings().items():
                        if i >= 2:
                            per[(key, r)].setdefault(k, []).append(v * 1e3)
        model.set_profiling(False)
    t_fwd = sum(statistics.median(v) for v in fwd.values())
    say(f"1. device time, us between HIP events, profiling on, batch {a.batch}, stride 1, min_margin {MIN_MARGIN:g}, median of {a.calls} calls "
        f"after 2 of warm-up (forward_u8, the sweep and the search alternated call by call); forward_u8 {t_fwd:.1f} us")
    for key in SEARCHES:
        (h, w), amp = key
        med = {r: statistics.median(per[(key, r)]["patch.attack"]) for r in (1, 2, 4)}
        t_sweep = statistics.median(sweep[key]["patch.sweep"])
        rec = attack.patch_search_u8(model, x8, cls, key[0], 1, amp, 2, MIN_MARGIN)[0].cpu().numpy().view(attack.PATCH_RECORD).reshape(a.batch, -1)
        P = rec.shape[1]
        say(f"   {h}x{w} amp {amp:<3d} P={P:<4d} patch.base {statistics.median(per[(key, 2)]['patch.base']):.1f}  patch.attack {med[2]:.0f} us = "
            f"{1e3 * med[2] / (a.batch * P):.0f} ns per (image, position); patch.sweep {t_sweep:.0f} us = {1e3 * t_sweep / (a.batch * P):.0f} ns: "
            f"ratio {med[2] / t_sweep:.1f}; the search costs {med[2] / t_fwd:.0f} forwards of {a.batch}; rounds 1 / 4 (median of 2 calls): {med[1]:.0f} / "
            f"{med[4]:.0f} us   [positions kept from round 0 / 1 / 2: {(rec['round'] == 0).sum()} / {(rec['round'] == 1).sum()} / "
            f"{(rec['round'] == 2).sum()}; predicted m_pred < -min_margin: {(rec['m_pred'] < -MIN_MARGIN).sum()} of {rec.size}; with a cell "
            f"within the slack: {(rec['unknown'] > 0).sum()}]")

    # 2. the confirm forwards
    say(f"2. attack_patch_u8 at batch {a.batch}, two rounds, wall ms with the records read back (median of 3 calls): what the forwards add")
    for key in (((4, 4), 255), ((1, 1), 255)):
        (h, w), amp = key
        parts = []
        for mode in ("none", "best", "all"):
            walls = []
            for rep in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                res = attack.attack_patch_u8(model, x8, cls, key[0], 1, amp, 2, MIN_MARGIN, mode)
                walls.append((time.perf_counter() - t0) * 1e3)
            judged = int((~np.isnan(res.map["margin"])).sum())
            parts.append(f"{mode} {statistics.median(walls):.1f} ms ({judged} witnesses forwarded, {int((res.map['status'] == attack.FALSIFIED).sum())} "
                         f"falsified)")
        say(f"   {h}x{w} amp {amp}: " + ";  ".join(parts))

    # 3. a whole pass from device-resident bytes
    images = np.ascontiguousarray(synth.synth_images_u8(a.images, hw=(32, 32)).transpose(0, 2, 3, 1))
    xd = torch.from_numpy(images).to(dev)
    with torch.no_grad():
        labels = torch.cat([model.forward_u8(xd[i:i + a.batch]).argmax(dim=1) for i in range(0, a.images, a.batch)])
    batches = [(xd[i:i + a.batch], labels[i:i + a.batch]) for i in range(0, a.images, a.batch)]
    say(f"3. {a.images} device-resident images in batches of {a.batch}, two rounds, min_margin {MIN_MARGIN:g} on both sides, records, maps and fills "
        "copied to the host: wall ms of one pass")
    for patch, stride, mode in (((1, 1), 1, "best"), ((4, 4), 4, "all")):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        found = attack.attack_patch_batches(model, batches, [patch], stride, 255, 2, MIN_MARGIN, mode)
        t_att = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        certs = certify.certify_patch_batches(model, batches, [patch], stride, 255, min_margin=MIN_MARGIN)
        t_cert = (time.perf_counter() - t0) * 1e3
        say(f"   {patch[0]}x{patch[1]} / 255 / stride {stride}, confirm {mode}: attack_patch_batches {t_att:.0f} ms = "
            f"{found[0]['positions'] / t_att * 1e3 / 1e6:.2f} M (image, position) searches/s; certify_patch_batches {t_cert:.0f} ms")
        say("   " + certify.patch_line(certs[0]))
        say("   " + attack.patch_robust_line(certs[0], found[0]) + "   [synthetic weights, the device's own top-1 as the class]")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
