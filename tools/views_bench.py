"""What views cost on the device (ttnet_resize_views_u8_ragged, ttnet_make_eval_views, ttnet_mean_views), one process,
the legs of a comparison alternated:

  (a) the existing ragged call, ttnet_resize_center_crop_u8_ragged, from THIS tree's library and from the PARENT commit's
      (--parent-lib, a libttnet.so built from the parent checkout) on the same buffers: 256 images of 375 x 500 and the
      seeded 121-size mix of ragged_bench.py.  Three runs each, alternated; the tree/parent ratio of the best runs is
      set beside the spread the parent shows against itself (its slowest run / its fastest).
  (b) the views resize (generator + resize) at V = 1, 2, 5, 10 on both workloads: time per call and per view.
  (c) images/s of the JPEG pipeline through a DataLoader of --workers spawned workers, two batches in flight, with
      views None (jpeg_eval_forward, the existing path), "flip" and "ten" (jpeg_views_forward), alternated.
  (d) --parent-tree DIR: bench.py's headline in this tree and in the parent checkout, alternated, one fresh process each.

    python tools/views_bench.py [--parent-lib FILE] [--parent-tree DIR] [--reps 50] [--workers 16] [--loader-batches 24]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scale_imagenet_amd import _lib, jpeg as J, preprocess, synth, ttnet  # noqa: E402

B = 256
dev = torch.device("cuda", 0)


def ev_time(fn, reps):
    """us per call, by events around `reps` calls after 5 warm-up calls."""
    for i in range(5):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def raw_center_crop(lib, r, out):
    """ttnet_resize_center_crop_u8_ragged of `lib` (a CDLL) on a RaggedU8: the call alone, no wrapper around it."""
    fn = lib.ttnet_resize_center_crop_u8_ragged
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    args = (r.data.data_ptr(), r.data.numel(), r.desc.data_ptr(), len(r), r.max_h, r.max_w, 256, 224, out.data_ptr(), None)

    def call(_):
        st = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
        assert st == 0, st
    return call


def fmt(runs):
    return ", ".join(f"{t:.1f}" for t in runs)


def leg_a(a, workloads):
    if not a.parent_lib:
        print("(a) no --parent-lib: the tree's ragged call alone")
    tree = _lib.load()
    parent = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    for name, r in workloads:
        out_t = torch.empty((len(r), 224, 224, 3), dtype=torch.uint8, device=dev)
        out_p = torch.empty_like(out_t)
        call_t = raw_center_crop(tree, r, out_t)
        ts, ps = [], []
        if parent is not None:
            call_p = raw_center_crop(parent, r, out_p)
            call_t(0), call_p(0)
            torch.cuda.synchronize()
            assert torch.equal(out_t, out_p), "the tree's ragged crops differ from the parent's"
        for _ in range(3):                       # alternated
            if parent is not None:
                ps.append(ev_time(call_p, a.reps))
            ts.append(ev_time(call_t, a.reps))
        line = f"(a) ragged centre crop, {name}: tree {min(ts):.1f} us (runs {fmt(ts)})"
        if parent is not None:
            ratio, spread = min(ts) / min(ps), max(ps) / min(ps)
            verdict = "inside" if 1.0 / spread <= ratio <= spread else "OUTSIDE"
            line += (f"; parent {min(ps):.1f} us (runs {fmt(ps)}); same bytes; tree / parent {ratio:.3f}, {verdict} the parent's "
                     f"own spread [{1.0 / spread:.3f}, {spread:.3f}]")
        print(line, flush=True)


def leg_b(a, workloads):
    for name, r in workloads:
        base = ev_time(lambda i: preprocess.resize_center_crop_u8_ragged(r), a.reps)
        print(f"(b) {name}: resize_center_crop_u8_ragged (wrapper) {base:.1f} us per call", flush=True)
        for family, V in (("center", 1), ("flip", 2), ("five", 5), ("ten", 10)):
            views = preprocess.eval_views(r, family)
            t_gen = ev_time(lambda i: preprocess.eval_views(r, family), a.reps)
            t_res = ev_time(lambda i: preprocess.resize_views_u8_ragged(r, views), a.reps)
            t_both = ev_time(lambda i: preprocess.resize_views_u8_ragged(r, preprocess.eval_views(r, family)), a.reps)
            print(f"(b) {name}, V = {V:2d} ({family}): generator {t_gen:.1f} us, views resize {t_res:.1f} us per call = "
                  f"{t_res / (len(r) * V):.3f} us per view ({t_res / base:.2f} x the centre-crop call), both {t_both:.1f} us",
                  flush=True)
        logits = torch.randn((len(r) * 10, 1000), device=dev)
        print(f"(b) mean_views [{len(r)} x 10, 1000]: {ev_time(lambda i: preprocess.mean_views(logits, 10), a.reps):.1f} us", flush=True)
    preprocess.check_ragged(dev)


class Files(torch.utils.data.Dataset):
    def __init__(self, files, n):
        self.files, self.n = files, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.files[i % len(self.files)], 0


def fixture_files():
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "ref_jpeg.json")) as f:
        ents = [e for e in json.load(f)["images"] if e["device"]]
    big = [e for e in ents if e["h"] * e["w"] >= 375 * 500]
    out = []
    for e in big * 3 + [e for e in ents if e not in big]:      # (the batch composition of tools/jpeg_bench.py)
        with open(os.path.join(gold, "jpeg", e["name"] + ".jpg"), "rb") as f:
            out.append(f.read())
    return out


def leg_c(a):
    from _util import args_for, spec_and_state
    _, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(dev).eval().reserve(B * 10)
    model.set_lanes(2)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    files = fixture_files()
    n = B * a.loader_batches
    loader = torch.utils.data.DataLoader(Files(files, n), batch_size=B, num_workers=a.workers, collate_fn=J.collate_jpeg,
                                         pin_memory=True, multiprocessing_context="spawn", persistent_workers=True, prefetch_factor=2)

    def one_pass(views):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i, (b, _) in enumerate(loader):
            with torch.cuda.stream(streams[i & 1]), torch.no_grad():
                b = b.to(dev, non_blocking=True)
                if views is None:
                    J.jpeg_eval_forward(model, b, lane=i & 1)
                else:
                    J.jpeg_views_forward(model, b, views, lane=i & 1)
        torch.cuda.synchronize(dev)
        return n / (time.perf_counter() - t0)

    # from a packed, pinned batch already on the host (no loader): device time per batch
    rj = J.pack_jpeg([files[i % len(files)] for i in range(B)]).pin_memory()
    k = [0]

    def step(views):
        lane = k[0] & 1
        k[0] += 1
        with torch.cuda.stream(streams[lane]), torch.no_grad():
            b = rj.to(dev, non_blocking=True)
            J.jpeg_eval_forward(model, b, lane=lane) if views is None else J.jpeg_views_forward(model, b, views, lane=lane)
    for views in (None, "flip", "ten", None):
        for _ in range(4):
            step(views)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            step(views)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / 20
        print(f"(c) packed host batch -> H2D -> decode -> views {views} -> forward_u8 (2 in flight): {dt * 1e3:.3f} ms per batch of "
              f"{B}, {B / dt:,.0f} images/s", flush=True)
    one_pass(None)                                   # starts the workers: not counted
    rates = {None: [], "flip": [], "ten": []}
    for _ in range(2):                               # alternated
        for views in rates:
            rates[views].append(one_pass(views))
    for views, v in rates.items():
        print(f"(c) end to end, DataLoader({a.workers} spawned workers, pin_memory) -> collate_jpeg -> decode -> views {views} -> "
              f"forward_u8 (2 in flight): {statistics.mean(v):,.0f} images/s (passes {', '.join(f'{x:,.0f}' for x in v)}) over "
              f"{a.loader_batches} batches of {B}", flush=True)
    del loader
    J.check_jpeg(dev)
    preprocess.check_ragged(dev)


def leg_d(a):
    def headline(tree):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "20"], cwd=tree,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"bench.py failed in {tree}:\n{r.stdout[-1000:]}\n{r.stderr[-2000:]}")
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        return out
    res = {"tree": [], "parent": []}
    for _ in range(2):                               # alternated
        res["parent"].append(headline(a.parent_tree))
        res["tree"].append(headline(ROOT))
    key = "value"                                    # images/s, the headline
    for name, runs in res.items():
        print(f"(d) bench.py --gpus 1 --steps {a.bench_steps} --warmup 20, {name}: {key} {', '.join(f'{r[key]:,.0f}' for r in runs)}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libttnet.so built from the parent commit")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit, for leg (d)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loader-batches", type=int, default=24)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--legs", default="abcd")
    a = ap.parse_args()
    if "d" in a.legs and a.parent_tree:              # first: fresh processes, before this one holds the device
        leg_d(a)
    rng = np.random.default_rng(0)
    uni = preprocess.pack_u8(list(rng.integers(0, 256, size=(B, 375, 500, 3), dtype=np.uint8))).to(dev)
    sizes = synth.imagenet_like_sizes(B, seed=0)
    mixed = preprocess.pack_u8([rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]).to(dev)
    workloads = [(f"{B} x 375x500", uni), (f"mixed {B} images ({len(set(sizes))} sizes)", mixed)]
    if "a" in a.legs:
        leg_a(a, workloads)
    if "b" in a.legs:
        leg_b(a, workloads)
    del uni, mixed, workloads
    if "c" in a.legs:
        leg_c(a)


if __name__ == "__main__":
    main()
