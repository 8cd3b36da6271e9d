"""What the witness search of TT_FHE_XSMALL_vAlexnet costs on one MI355X, next to the forward and the certificate of the same run.

    python tools/attack_bench.py [--batch 256] [--calls 100] [--images 10000] [--rounds 3] [--out profiles/attack_bench.txt]

Legs, all in one process, at CIFAR mean / std and at the wide std (16, 16, 16), eps 1 and 2:
  1. device time of one round at --batch -- "attack.propose", the eight candidate forwards, "attack.select" -- from
     ttnet_plan_last_timings with profiling on (plain launches, HIP events around each step), and forward_u8 and
     ttnet_certify_u8 measured the same way in the same loop: medians over --calls after a warm-up.  The round measured is
     round 1 from the state round 0 leaves, re-initialised before every call;
  2. one pass over --images device-resident synthetic images: certify_batches + attack_batches, wall time, the `Robust..`
     line and the share falsified by round.
No speed threshold is set in advance: the file records what was measured.  Synthetic weights and images: the counts say
nothing about a trained network.
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

from scale_imagenet_amd import attack, certify, cifar, synth, ttnet  # noqa: E402
from scale_imagenet_amd.spec import VAlexSpec  # noqa: E402

NORMS = (("CIFAR std", cifar.CIFAR_STD), ("std 16", (16.0, 16.0, 16.0)))
EPS = (1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attack_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = ttnet.TT_FHE_XSMALL_vAlexnet(Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None]))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(VAlexSpec()).items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"attack_bench: TT_FHE_XSMALL_vAlexnet, SYNTHETIC weights and images, batch {a.batch}, {torch.cuda.get_device_name(dev)}",
             "command: python tools/attack_bench.py " + " ".join(sys.argv[1:]),
             "the counts below come from synthetic weights: they say nothing about a trained network (not measured: a trained checkpoint)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.batch
    x8 = torch.from_numpy(np.ascontiguousarray(synth.synth_images_u8(n, hw=(32, 32)).transpose(0, 2, 3, 1))).to(dev)
    images = np.ascontiguousarray(synth.synth_images_u8(a.images, hw=(32, 32)).transpose(0, 2, 3, 1))
    xd = torch.from_numpy(images).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    med = lambda d: {k: statistics.median(v) for k, v in d.items()}
    fmt = lambda d: "  ".join(f"{k} {v:.1f}" for k, v in d.items()) + f"   sum {sum(d.values()):.1f}"
    say(f"1. device time, us between HIP events, profiling on, batch {n}, median of {a.calls} calls after 10 of warm-up (forward_u8, the "
        "certificate and one round of the search alternated call by call; the round is round 1, re-initialised by round 0 before each call)")
    passes = []
    for name, std in NORMS:
        model.set_input_norm(cifar.CIFAR_MEAN, std)
        with torch.no_grad():
            cls = model.forward_u8(x8).argmax(dim=1).to(torch.int32)      # the device's own top-1 as the class
        plan = model._plan_for(dev, n)
        rows = torch.empty((n, 8), dtype=torch.int32, device=dev)
        xcur = torch.empty_like(x8)
        worst = torch.empty(n, dtype=torch.int32, device=dev)
        active = torch.empty(n, dtype=torch.int32, device=dev)
        logits = torch.empty((8 * n, 10), dtype=torch.float32, device=dev)
        fwd, cert = {}, {e: {} for e in EPS}
        rnd = {e: {"attack.propose": [], "candidate forwards (8)": [], "attack.select": []} for e in EPS}
        planes = {}
        for e in EPS:
            p = model.certify_u8(x8, cls, float(e), 0, return_planes=True).planes
            planes[e] = torch.stack([p["stem_lo"], p["stem_hi"]]).contiguous()
        model.set_profiling(True)
        with torch.no_grad():
            for i in range(a.calls + 10):
                keep = i >= 10
                for e in EPS:
                    model.certify_u8(x8, cls, float(e))
                    for k, v in model.last_timings().items():
                        if keep:
                            cert[e].setdefault(k, []).append(v * 1e3)
                    attack._forward_into(plan, 0, x8, logits[:n], stream)
                    for k, v in model.last_timings().items():
                        if keep and e == EPS[0]:
                            fwd.setdefault(k, []).append(v * 1e3)
                    attack.select_u8(model, x8, logits, n, 1, cls, 0.0, x8, xcur, rows, worst, active, 0)
                    cand = attack.propose_u8(model, x8, xcur, cls, worst, planes[e], e, active, 0)
                    t_prop = sum(model.last_timings().values()) * 1e3
                    flat, t_fwd = cand.view(8 * n, 32, 32, 3), 0.0
                    for b in range(0, 8 * n, n):
                        attack._forward_into(plan, 0, flat[b:b + n], logits[b:b + n], stream)
                        t_fwd += sum(model.last_timings().values()) * 1e3
                    attack.select_u8(model, cand, logits, n, 8, cls, 0.0, x8, xcur, rows, worst, active, 1)
                    t_sel = sum(model.last_timings().values()) * 1e3
                    if keep:
                        for k, v in zip(rnd[e], (t_prop, t_fwd, t_sel)):
                            rnd[e][k].append(v)
        model.set_profiling(False)
        say(f"   {name}: forward_u8      " + fmt(med(fwd)))
        for e in EPS:
            say(f"   {name}: certify eps={e}   " + fmt(med(cert[e])))
            r = med(rnd[e])
            say(f"   {name}: one round eps={e} " + fmt(r) + f"   = {sum(r.values()) / sum(med(fwd).values()):.1f} forward_u8 of {n} images")
        # 2. a whole pass from device-resident bytes
        with torch.no_grad():
            labels = torch.cat([model.forward_u8(xd[i:i + n]).argmax(dim=1) for i in range(0, a.images, n)])
        batches = [(xd[i:i + n], labels[i:i + n]) for i in range(0, a.images, n)]
        for rep in range(2):                                              # (the first pass warms up: graphs, first-use builds)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            certs = certify.certify_batches(model, batches, [float(e) for e in EPS])
            t1 = time.perf_counter()
            found = attack.attack_batches(model, batches, [float(e) for e in EPS], a.rounds)
            t2 = time.perf_counter()
        passes.append((name, certs, found, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    say(f"2. {a.images} device-resident images in batches of {n}, eps {', '.join(str(e) for e in EPS)} in one pass each, {a.rounds} rounds, wall ms of "
        "the second pass (records copied to the host at the end); classes: the device's own top-1")
    for name, certs, found, tc, ta in passes:
        say(f"   {name}: certify_batches {tc:.1f} ms, attack_batches {ta:.1f} ms (its own certificate for the planes included) = "
            f"{len(EPS) * a.images / ta * 1e3:.0f} searches/s")
        for c, f in zip(certs, found):
            say("   " + certify.verified_line(c))
            say("   " + attack.robust_line(c["eps"], c["rows"], f["rows"]))
            open_after = f["images"] - f["wrong"]
            say(f"      falsified by round {f['by_round']} of {open_after} images right at x0; changed bytes of a witness: median "
                f"{float(np.median(f['rows']['changed'][f['rows']['status'] == 2])) if f['search'] else 0:g} of 3072")
    say(f"3. cost in forwards per image: 1 (x0) + per round 8 (candidates) + 1 (x_cur, from round 2 on) = {1 + 9 * a.rounds - 1} for "
        f"{a.rounds} rounds, whether the image is still open or not (the open images of a round are not compacted)")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
