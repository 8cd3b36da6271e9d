"""Ragged Resize(256) + CenterCrop(224) (ttnet_resize_center_crop_u8_ragged, csrc/preproc.hip) on the device:
  1. device time on 256 images of 375 x 500, beside the single-size kernel (ttnet_resize_center_crop_u8) in the same
     process, the two alternated;
  2. device time on a seeded ImageNet-like mix of 256 sizes (synth.imagenet_like_sizes: mostly 500 x 375 / 375 x 500 /
     500 x 333, a few up to 3000 x 4000);
  3. images/s of pack -> H2D -> resize -> forward_u8 (TT-small) with two batches in flight, for both batches; the
     host packing (pack_u8, one thread) is timed on its own and the pipeline is also run from pre-packed pinned batches.
usage: python tools/ragged_bench.py [reps]"""
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np
import torch

from _util import args_for, spec_and_state
from scale_imagenet_amd import preprocess, synth, ttnet

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
B = 256
dev = torch.device("cuda:0")


def ev_time(fn, reps=REPS):
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


rng = np.random.default_rng(0)
uni = [rng.integers(0, 256, size=(B, 375, 500, 3), dtype=np.uint8) for _ in range(2)]
uni_dev = [torch.from_numpy(u).to(dev) for u in uni]
uni_r = [preprocess.pack_u8(list(u)).to(dev) for u in uni]
assert torch.equal(preprocess.resize_center_crop_u8(uni_dev[0]), preprocess.resize_center_crop_u8_ragged(uni_r[0]))
single, ragged = [], []
for _ in range(3):                       # alternated
    single.append(ev_time(lambda i: preprocess.resize_center_crop_u8(uni_dev[i % 2])))
    ragged.append(ev_time(lambda i: preprocess.resize_center_crop_u8_ragged(uni_r[i % 2])))
print(f"uniform {B} x 375x500: single-size kernel {min(single):.1f} us (runs {', '.join(f'{t:.1f}' for t in single)}); "
      f"ragged kernel {min(ragged):.1f} us (runs {', '.join(f'{t:.1f}' for t in ragged)}); ratio {min(ragged) / min(single):.2f}")

sizes = synth.imagenet_like_sizes(B, seed=0)
mixed_ims = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]
t0 = time.perf_counter()
mixed_host = preprocess.pack_u8(mixed_ims)
t_pack = time.perf_counter() - t0
mixed_r = mixed_host.to(dev)
t_mixed = ev_time(lambda i: preprocess.resize_center_crop_u8_ragged(mixed_r))
mb = mixed_host.data.numel() / 2 ** 20
print(f"mixed {B} images ({len(set(sizes))} distinct sizes, {mb:.0f} MiB, largest {max(sizes, key=lambda s: s[0] * s[1])}): "
      f"ragged kernel {t_mixed:.1f} us; pack_u8 on the host {t_pack * 1e3:.1f} ms")

spec, st = spec_and_state("small")
m = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()})
m = m.to(dev).eval().reserve(B)
m.set_lanes(2)
streams = [torch.cuda.Stream(dev) for _ in range(2)]


def pipeline(batches, pack_images=None, k=40):
    """two batches in flight: on stream i % 2, [pack ->] H2D (pinned, non-blocking) -> ragged resize -> forward_u8"""
    def step(i):
        with torch.cuda.stream(streams[i % 2]):
            r = preprocess.pack_u8(pack_images).pin_memory() if pack_images is not None else batches[i % len(batches)]
            preprocess.imgnet_eval_forward(m, r.to(dev, non_blocking=True), lane=i % 2)
    with torch.no_grad():
        for i in range(4):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            step(i)
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return k * B / el, el / k * 1e6


uni_pinned = [preprocess.pack_u8(list(u)).pin_memory() for u in uni]
mixed_pinned = [mixed_host.pin_memory()]
for name, batches, ims in [("uniform 375x500", uni_pinned, list(uni[0])), ("mixed", mixed_pinned, mixed_ims)]:
    ips, us = pipeline(batches)
    ips_p, us_p = pipeline(batches, pack_images=ims, k=10)
    print(f"pipeline {name}, two batches in flight: H2D -> resize -> forward_u8 {ips:,.0f} images/s ({us:.0f} us per batch); "
          f"with pack_u8 + pin on the host thread {ips_p:,.0f} images/s ({us_p:.0f} us per batch)")
preprocess.check_ragged(dev)
