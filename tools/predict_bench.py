"""What the per-image predictions and per-class counters cost: ttnet_topk_rows next to the stock sequence it replaces,
and evaluate() with the options off (against the parent commit) and on.

    python tools/predict_bench.py [--batch 256] [--batches 200] [--windows 9] [--inflight 2] [--k 5]
                                  [--parent DIR] [--out profiles/predict_bench.txt]

Legs (medians over the windows after one warm-up pass of each; the legs of a comparison alternate window by window, in
one process, so that drift hits them alike):
  1. one [--batch, 1000] batch: ttnet_topk_rows (k = --k) between HIP events around 200 back-to-back calls, next to
     torch.topk + log_softmax + gather on the same tensor (the method of leg 2 of tools/eval_bench.py); then
     ttnet_class_counts alone;
  2. evaluate() on device-resident float batches, device metrics, options off: this tree against the package under
     --parent (a checkout of the parent commit with its library built), which is loaded twice (A, B) so that the
     parent's own A/A spread is on the page.  Skipped without --parent;
  3. the same leg on this tree with topk = --k, per_class = True against the options off: what a user pays.
No number is promised: the output file records what was measured.
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scale_imagenet_amd import synth  # noqa: E402
from scale_imagenet_amd.evaluate import DeviceMetrics, topk_rows  # noqa: E402


class _Quiet:
    """evaluate() prints its Acc.. line per call; keep the report readable."""

    def __enter__(self):
        self.out, sys.stdout = sys.stdout, open(os.devnull, "w")

    def __exit__(self, *exc):
        sys.stdout.close()
        sys.stdout = self.out


def load_package(name: str, root: str):
    """The package scale_imagenet_amd of the tree at ``root`` under another name (its own libttnet.so beside it)."""
    path = os.path.join(root, "scale_imagenet_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def alternate(legs, windows, images):
    """{name: (median, slowest, fastest) images/s}: every window runs each leg once, in turn."""
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()                                               # warm-up: plans, graphs, workspaces
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
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, library built (leg 2)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    _, st = spec_and_state("small")
    state = {k: torch.from_numpy(v.copy()) for k, v in st.items()}
    lines = [f"predict_bench: TT-small, synthetic weights, batch {a.batch}, inflight {a.inflight}, k {a.k}, {a.windows} windows, "
             f"{torch.cuda.get_device_name(dev)}", "command: python tools/predict_bench.py " + " ".join(sys.argv[1:])]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def model_of(pkg):
        ttnet = importlib.import_module(pkg + ".ttnet")
        m = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
        m.load_state_dict(state, strict=True)
        return m.to(dev).eval().reserve(a.batch)

    def leg(pkg, model, data, **kw):
        evaluate = importlib.import_module(pkg + ".evaluate").evaluate

        def run():
            with _Quiet():
                evaluate(model, data, dev, inflight=a.inflight, metrics="device", **kw)
        return run

    model = model_of("scale_imagenet_amd")
    pool = [torch.from_numpy(synth.synth_images(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    tpool = [torch.from_numpy(synth.synth_targets(a.batch, first=a.batch * i)).to(dev) for i in range(2)]
    batches = [(pool[i % 2], tpool[i % 2]) for i in range(a.batches)]
    images = a.batch * a.batches

    # 1. the kernels alone, HIP events around back-to-back calls
    with torch.no_grad():
        logits = model(pool[0]).clone()
    rec = torch.empty((a.batch, a.k, 2), dtype=torch.int64, device=dev)
    dm = DeviceMetrics(dev, 1)

    def stock():
        top = logits.topk(a.k, dim=1)
        return top.indices, top.values, torch.log_softmax(logits, dim=1).gather(1, top.indices)

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

    t_topk = timed(lambda: topk_rows(logits, a.k, out=rec))
    t_stock = timed(stock)
    t_metrics = timed(lambda: dm.update(logits, tpool[0], 0))
    t_counts = timed(lambda: dm.update(logits, tpool[0], 0, topk=rec, per_class=True))
    say(f"1. one [{a.batch}, {logits.shape[1]}] batch, back-to-back calls between HIP events (includes their launch gaps)")
    say(f"   ttnet_topk_rows, k = {a.k} (1 launch)            {t_topk:8.2f} us per call")
    say(f"   torch.topk + log_softmax + gather (float32)   {t_stock:8.2f} us per call")
    say(f"   ttnet_eval_metrics (2 launches)               {t_metrics:8.2f} us per call")
    say(f"   ttnet_eval_metrics + ttnet_class_counts       {t_counts:8.2f} us per call")

    # 2. options off against the parent commit
    if a.parent:
        names = {"parent A": "ttnet_parent_a", "branch": "scale_imagenet_amd", "parent B": "ttnet_parent_b"}
        for tag in ("parent A", "parent B"):
            load_package(names[tag], a.parent)
        models = {tag: model if tag == "branch" else model_of(pkg) for tag, pkg in names.items()}
        r = alternate({tag: leg(pkg, models[tag], batches) for tag, pkg in names.items()}, a.windows, images)
        say(f"2. evaluate(), float batches on the device, metrics=device, options off, {a.batches} batches per window: "
            "median (slowest .. fastest) images/s")
        for tag, (med, lo, hi) in r.items():
            say(f"   {tag:<9} {med:12.0f}   ({lo:.0f} .. {hi:.0f})")
        lo, hi = sorted((r["parent A"][0], r["parent B"][0]))
        say(f"   branch / mean of the parent's two = {2 * r['branch'][0] / (lo + hi):.4f}; the parent's A/A medians differ by "
            f"{100 * (hi - lo) / lo:.2f} %")
        del models
    else:
        say("2. (no --parent: the comparison with the parent commit was not run)")

    # 3. what the options cost
    legs = {"options off": leg("scale_imagenet_amd", model, batches),
            f"topk={a.k}": leg("scale_imagenet_amd", model, batches, topk=a.k),
            f"topk={a.k}, per_class": leg("scale_imagenet_amd", model, batches, topk=a.k, per_class=True)}
    r = alternate(legs, a.windows, images)
    say(f"3. the same leg on this tree, {a.batches} batches per window: median (slowest .. fastest) images/s")
    for tag, (med, lo, hi) in r.items():
        say(f"   {tag:<22} {med:12.0f}   ({lo:.0f} .. {hi:.0f})   {med / r['options off'][0]:.3f} of options off")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
