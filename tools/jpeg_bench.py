"""Device JPEG decoding (ttnet_jpeg_decode_ragged) against host decoding with Pillow, every leg timed the same way.
Batches of 256 are built from the committed fixtures (tests/golden/jpeg: the 500 x 375 / 375 x 500 and 600 x 560
quality-90 files and the other device-decoded ones, repeated).

    python tools/jpeg_bench.py [--batch 256] [--windows 5] [--iters 20] [--workers 16] [--loader-batches 64]
    python tools/jpeg_bench.py --progressive     (the progressive legs only; needs Pillow to re-encode the batch)

Legs (medians over timed windows after warm-up):
  1. host cost per image on one thread: pack_jpeg (header walk + packing) against Pillow decode + pack_u8;
  2. decode only, from a packed batch already on the device (images/s, compressed MB/s, sequential-fallback share);
  3. device pipeline from a packed, pinned host batch, two batches in flight on two lanes / streams:
     H2D -> decode -> ragged resize -> forward_u8, against the same for Pillow-decoded pixels:
     H2D -> ragged resize -> forward_u8 (host packing excluded from both);
  4. end to end: the same DataLoader (spawned workers, pin_memory, two batches in flight) over the files' bytes, whose
     collate_fn is either collate_jpeg or Pillow decode + collate_u8 (host packing included in both).
--progressive: the same batch composition re-encoded progressively by Pillow (same tables and sampling, libjpeg's
default scan script), timed the same way: decode only next to the sequential batch of the same run, and the loader end
to end with collate_jpeg_progressive (device decode) against collate_jpeg (which decodes every such file with Pillow
in the worker).
Legs 1 and 4 need Pillow; without it they are skipped and say so.  Per-kernel device times: run under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scale_imagenet_amd import jpeg as J, preprocess, ttnet  # noqa: E402


def fixture_files():
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "ref_jpeg.json")) as f:
        ents = [e for e in json.load(f)["images"] if e["device"]]
    big = [e for e in ents if e["h"] * e["w"] >= 375 * 500]
    pick = big * 3 + [e for e in ents if e not in big]
    out = []
    for e in pick:
        with open(os.path.join(gold, "jpeg", e["name"] + ".jpg"), "rb") as f:
            out.append(f.read())
    return out


def batch_of(files, n, start=0):
    return [files[(start + i) % len(files)] for i in range(n)]


def pil_decode(b):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


class Files(torch.utils.data.Dataset):
    def __init__(self, files, n):
        self.files, self.n = files, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.files[i % len(self.files)], 0


def collate_pillow(batch):
    """The host-decode loader: Pillow decodes in the worker, then collate_u8 packs."""
    return preprocess.collate_u8([(pil_decode(b), t) for b, t in batch])


def median_windows(fn, iters, windows, dev, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    res = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(dev)
        res.append((time.perf_counter() - t0) / iters)
    return statistics.median(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--loader-batches", type=int, default=64)
    ap.add_argument("--progressive", action="store_true", help="the progressive legs only")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    files = fixture_files()
    if a.progressive:
        return progressive_legs(a, dev, files)
    data = batch_of(files, a.batch)
    nbytes = sum(len(b) for b in data)
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False

    # 1. host cost per image, one thread
    t_pack = statistics.median(_t(lambda: J.pack_jpeg(data)) for _ in range(5))
    rj_host = J.pack_jpeg(data).pin_memory()
    print(f"batch {a.batch}: {nbytes / 2**20:.2f} MiB of files, {rj_host.data.numel() / 2**20:.2f} MiB packed, "
          f"{rj_host.out_bytes / 2**20:.1f} MiB decoded")
    print(f"host, one thread: pack_jpeg {t_pack / a.batch * 1e6:.0f} us per image ({t_pack * 1e3:.1f} ms per batch)")
    if have_pil:
        t_pil = statistics.median(_t(lambda: [pil_decode(b) for b in data]) for _ in range(3))
        ims = [pil_decode(b) for b in data]
        t_pu8 = statistics.median(_t(lambda: preprocess.pack_u8(ims)) for _ in range(3))
        print(f"host, one thread: Pillow decode {t_pil / a.batch * 1e6:.0f} us + pack_u8 {t_pu8 / a.batch * 1e6:.0f} us "
              f"per image ({(t_pil + t_pu8) * 1e3:.1f} ms per batch)")
    else:
        print("host, one thread: Pillow is not importable here; Pillow legs skipped")

    # 2. decode only
    rj = rj_host.to(dev)
    J.decode_ragged(rj)
    J.jpeg_counters(dev)
    dt = median_windows(lambda: J.decode_ragged(rj), a.iters, a.windows, dev)
    _, nseq = J.jpeg_counters(dev)
    runs = 3 + a.windows * a.iters
    nseg = sum(J.parse_header(b).segments() for b in data)
    print(f"decode only: {dt * 1e3:.3f} ms per batch, {a.batch / dt:,.0f} images/s, {nbytes / dt / 1e6:,.0f} MB/s "
          f"compressed; sequential fallback: {nseq / runs:.2f} of {nseg} segments per batch")

    # 3. device pipelines from packed, pinned host batches, two in flight
    from _util import args_for, spec_and_state
    _, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    model.set_lanes(2)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    k = [0]

    def step(fwd, host_batch):
        lane = k[0] & 1
        k[0] += 1
        with torch.cuda.stream(streams[lane]), torch.no_grad():
            fwd(model, host_batch.to(dev, non_blocking=True), lane=lane)
    dt_j = median_windows(lambda: step(J.jpeg_eval_forward, rj_host), a.iters, a.windows, dev)
    print(f"device pipeline, packed host batch -> H2D -> decode -> resize -> forward_u8 (2 in flight): "
          f"{dt_j * 1e3:.3f} ms per batch, {a.batch / dt_j:,.0f} images/s")
    if have_pil:
        r_host = preprocess.pack_u8(ims).pin_memory()
        dt_u = median_windows(lambda: step(preprocess.imgnet_eval_forward, r_host), a.iters, a.windows, dev)
        print(f"device pipeline, packed Pillow-decoded host batch -> H2D -> resize -> forward_u8 (2 in flight): "
              f"{dt_u * 1e3:.3f} ms per batch, {a.batch / dt_u:,.0f} images/s")

    # 4. end to end through the same DataLoader
    if not have_pil:
        print("end to end: Pillow is not importable here; the host-decode loader leg is skipped")
    legs = [("collate_jpeg (device decode)", J.collate_jpeg, J.jpeg_eval_forward)]
    if have_pil:
        legs.append(("Pillow decode + collate_u8", collate_pillow, preprocess.imgnet_eval_forward))
    for name, collate, fwd in legs:
        loader = torch.utils.data.DataLoader(
            Files(files, a.batch * a.loader_batches), batch_size=a.batch, num_workers=a.workers, collate_fn=collate,
            pin_memory=True, multiprocessing_context="spawn", persistent_workers=True, prefetch_factor=2)
        times = []
        for rep in range(3):                          # the first pass starts the workers: not counted
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i, (b, _) in enumerate(loader):
                with torch.cuda.stream(streams[i & 1]), torch.no_grad():
                    fwd(model, b.to(dev, non_blocking=True), lane=i & 1)
            torch.cuda.synchronize(dev)
            if rep:
                times.append(time.perf_counter() - t0)
        t = statistics.median(times)
        n = a.batch * a.loader_batches
        print(f"end to end, DataLoader({a.workers} spawned workers, pin_memory) -> {name} -> ... -> forward_u8 "
              f"(2 in flight): {n / t:,.0f} images/s over {a.loader_batches} batches")
        del loader
    J.check_jpeg(dev)


def to_progressive(b):
    from PIL import Image
    out = io.BytesIO()
    Image.open(io.BytesIO(b)).save(out, "JPEG", quality="keep", subsampling="keep", progressive=True, optimize=True)
    return out.getvalue()


def loader_rate(a, dev, model, streams, files, collate, fwd):
    loader = torch.utils.data.DataLoader(
        Files(files, a.batch * a.loader_batches), batch_size=a.batch, num_workers=a.workers, collate_fn=collate,
        pin_memory=True, multiprocessing_context="spawn", persistent_workers=True, prefetch_factor=2)
    times = []
    for rep in range(3):                          # the first pass starts the workers: not counted
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i, (b, _) in enumerate(loader):
            with torch.cuda.stream(streams[i & 1]), torch.no_grad():
                fwd(model, b.to(dev, non_blocking=True), lane=i & 1)
        torch.cuda.synchronize(dev)
        if rep:
            times.append(time.perf_counter() - t0)
    del loader
    return a.batch * a.loader_batches / statistics.median(times), a.batch * a.loader_batches / max(times)


def progressive_legs(a, dev, files):
    prog = [to_progressive(b) for b in files]
    seq_b, prog_b = batch_of(files, a.batch), batch_of(prog, a.batch)
    t_pack = statistics.median(_t(lambda: J.pack_jpeg(prog_b, progressive=True)) for _ in range(5))
    t_fall = statistics.median(_t(lambda: J.pack_jpeg(prog_b)) for _ in range(3))
    rs, rp = J.pack_jpeg(seq_b).to(dev), J.pack_jpeg(prog_b, progressive=True).to(dev)
    assert set(rp.descriptors()["kind"].tolist()) == {J.KIND_PROGRESSIVE}
    chk = J.pack_jpeg(prog_b[:16])                # Pillow's pixels, copied through (the buffer's 16-byte padding aside)
    ref = J.decode_ragged(chk.to(dev)).data[:chk.out_bytes].cpu()
    got = J.decode_ragged(J.pack_jpeg(prog_b[:16], progressive=True).to(dev)).data[:chk.out_bytes].cpu()
    assert torch.equal(got, ref), "the device's progressive decode differs from Pillow's"
    print(f"progressive batch {a.batch}: {sum(len(b) for b in prog_b) / 2**20:.2f} MiB of files "
          f"({sum(len(b) for b in seq_b) / 2**20:.2f} MiB sequential), {rp.data.numel() / 2**20:.2f} MiB packed")
    print(f"host, one thread: pack_jpeg(progressive=True) {t_pack / a.batch * 1e6:.0f} us per image; "
          f"pack_jpeg (Pillow fallback) {t_fall / a.batch * 1e6:.0f} us per image")
    for _ in range(20):                           # clocks up before the first timed window
        J.decode_ragged(rs)
    res = {}
    for name, rj in (("sequential", rs), ("progressive", rp), ("sequential", rs), ("progressive", rp)):
        res.setdefault(name, []).append(median_windows(lambda: J.decode_ragged(rj), a.iters, a.windows, dev))
    for name, v in res.items():
        print(f"decode only, {name}: {min(v) * 1e3:.3f} / {max(v) * 1e3:.3f} ms per batch (two alternating runs of "
              f"{a.windows} windows x {a.iters} decodes, medians), {a.batch / statistics.mean(v):,.0f} images/s")
    if a.loader_batches < 1:                      # (--loader-batches 0: the decode legs alone, e.g. under rocprofv3)
        return J.check_jpeg(dev)
    from _util import args_for, spec_and_state
    _, st = spec_and_state("small")
    model = ttnet.TT_vf_19lv3_imgnet_small(args_for("small"))
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    model = model.to(dev).eval().reserve(a.batch)
    model.set_lanes(2)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for name, collate in (("collate_jpeg_progressive (device decode)", J.collate_jpeg_progressive),
                          ("collate_jpeg (Pillow fallback in the worker)", J.collate_jpeg)):
        med, low = loader_rate(a, dev, model, streams, prog, collate, J.jpeg_eval_forward)
        print(f"end to end, progressive files, DataLoader({a.workers} spawned workers, pin_memory) -> {name} -> ... -> "
              f"forward_u8 (2 in flight): {med:,.0f} images/s over {a.loader_batches} batches (slower of two passes "
              f"{low:,.0f})")
    J.check_jpeg(dev)


def _t(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
