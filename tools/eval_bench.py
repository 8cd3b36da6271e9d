"""What the device metrics (ttnet_eval_metrics) buy the evaluation loop: evaluate() timed with metrics="torch" and with
metrics="device", one process, the legs alternated window by window so that drift hits both alike.

    python tools/eval_bench.py [--batch 256] [--batches 200] [--windows 7] [--inflight 2] [--workers 16]
                               [--out profiles/eval_metrics_bench.txt]

Legs (medians over the windows after one warm-up pass of each):
  1. device-resident float batches of --batch images, TT-small with synthetic weights: images/s of both metric paths;
  2. the per-call device time of ttnet_eval_metrics on [--batch, 1000] logits from HIP events around 200 back-to-back
     calls, next to the stock sequence it replaces (cross_entropy + topk + eq / any / float / mean);
  3. the same two metric paths behind a JPEG loader over the committed fixtures, the batch built as
     tools/jpeg_bench.py builds its own (spawned workers, pin_memory, collate_jpeg).
No number is promised: whether the fused metrics buy anything measurable is what the output file records.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from scale_imagenet_amd import jpeg as J, synth, ttnet  # noqa: E402
from scale_imagenet_amd.evaluate import DeviceMetrics, evaluate  # noqa: E402


class _Quiet:
    """evaluate() prints its Acc.. line per call; keep the report readable."""

    def __enter__(self):
        self.out, sys.stdout = sys.stdout, open(os.devnull, "w")

    def __exit__(self, *exc):
        sys.stdout.close()
        sys.stdout = self.out


def alternate(legs, windows, images):
    """{name: median images/s}: every window runs each leg once, in turn."""
    times = {k: [] for k in legs}
    for k, fn in legs.items():
        fn()                                               # warm-up: plans, graphs, workspaces, loader start
    for _ in range(windows):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    return {k: (images / statistics.median(v), images / max(v), images / min(v)) for k, v in times.items()}


def main():
    from _util import args_for, spec_and_state
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loader-batches", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    lines = [f"eval_bench: TT-small, synthetic weights, batch {a.batch}, inflight {a.inflight}, {a.windows} windows, "
             f"{torch.cuda.get_device_name(dev)}"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # 1. device-resident float batches
    pool = [torch.from_numpy(synth.synth_images(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    tpool = [torch.from_numpy(synth.synth_targets(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    batches = [(pool[i % 2], tpool[i % 2]) for i in range(a.batches)]

    def leg(metrics, data):
        def run():
            with _Quiet():
                evaluate(model, data, dev, inflight=a.inflight, metrics=metrics)
        return run

    r = alternate({"torch": leg("torch", batches), "device": leg("device", batches)}, a.windows, a.batch * a.batches)
    say(f"1. float batches on the device, {a.batches} batches per window (median, slowest .. fastest window)")
    for k, (med, lo, hi) in r.items():
        say(f"   metrics={k:<7} {med:12.0f} images/s   ({lo:.0f} .. {hi:.0f})")
    say(f"   device / torch = {r['device'][0] / r['torch'][0]:.3f}")

    # 2. the metrics alone, HIP events around back-to-back calls
    with torch.no_grad():
        logits = model(pool[0])
    dm = DeviceMetrics(dev, 1)

    def stock():
        loss = torch.nn.functional.cross_entropy(logits, tpool[0])
        hits = logits.topk(5, dim=1).indices.eq(tpool[0].reshape(-1, 1))
        return loss, hits[:, :1].any(dim=1).float().mean(), hits[:, :5].any(dim=1).float().mean()

    def timed(fn, calls=200):
        for _ in range(20):
            fn()
        per = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / calls)
        return statistics.median(per)

    t_dev = timed(lambda: dm.update(logits, tpool[0], 0))
    t_stock = timed(stock)
    say(f"2. metrics of one [{a.batch}, 1000] batch, back-to-back calls between HIP events (includes their launch gaps)")
    say(f"   ttnet_eval_metrics (2 launches)      {t_dev:8.2f} us per call")
    say(f"   cross_entropy + topk + eq/any/mean   {t_stock:8.2f} us per call")

    # 3. behind a JPEG loader over the committed fixtures
    import jpeg_bench
    files = jpeg_bench.fixture_files()
    n_img = a.batch * a.loader_batches
    loader = torch.utils.data.DataLoader(
        jpeg_bench.Files(files, n_img), batch_size=a.batch, num_workers=a.workers, collate_fn=J.collate_jpeg, pin_memory=True,
        multiprocessing_context="spawn", persistent_workers=True, prefetch_factor=2)
    r = alternate({"torch": leg("torch", loader), "device": leg("device", loader)}, max(3, a.windows // 2), n_img)
    say(f"3. JPEG loader ({a.workers} workers, collate_jpeg), {a.loader_batches} batches per window")
    for k, (med, lo, hi) in r.items():
        say(f"   metrics={k:<7} {med:12.0f} images/s   ({lo:.0f} .. {hi:.0f})")
    say(f"   device / torch = {r['device'][0] / r['torch'][0]:.3f}")
    del loader
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
