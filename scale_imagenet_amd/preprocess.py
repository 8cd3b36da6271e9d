"""GPU side of the reference's eval input transform (utils/preprocess.py:104-108, main.py:208):

    transforms.Resize(256) -> transforms.CenterCrop(224) -> transforms.ToTensor() -> transforms.Normalize(mean, std)

``resize_center_crop_u8`` does the first two on decoded uint8 HWC images already on the device
(libttnet: ttnet_resize_center_crop_u8, csrc/preproc.hip); the last two are fused into the stem by
``model.forward_u8``.  JPEG decoding from file bytes runs on the device too (``jpeg.py``: ``decode_ragged``,
``jpeg_eval_forward``).

A decoder batch of ImageNet images has many sizes.  ``pack_u8`` / ``collate_u8`` put such a batch into one flat
buffer plus descriptors (``RaggedU8``), and ``resize_center_crop_u8_ragged`` resizes and crops all of it in one
launch (ttnet_resize_center_crop_u8_ragged), in input order.

Views (``Views``, ``eval_views``, ``make_views``, ``resize_views_u8_ragged``) are crops other than that one centre crop:
the corner and mirrored crops of ``FiveCrop`` / ``TenCrop``, or boxes the caller chose, several per image, resized by the
same kernel in one launch; ``imgnet_views_forward`` forwards all of them and returns the mean of their logits
(``mean_views``), torchvision's ``outputs.view(n, V, -1).mean(1)``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib

# the largest image side pack_u8 accepts (ttnet_resize_center_crop_u8_ragged serves it at resize 256 / crop 224)
MAX_SIDE = 8192
# ttnet_image_desc (include/ttnet.h): int64 offset, int32 h, int32 w -- 16 bytes, viewed as int64 [n, 2] in torch
DESC_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])
assert DESC_DTYPE.itemsize == C.sizeof(_lib.ImageDesc) == 16


class RaggedU8:
    """A batch of decoded uint8 HWC images of mixed sizes: ``data`` (uint8 [bytes], image i at byte offset
    ``desc[i]``), ``desc`` (int64 [n, 2]: the 16-byte ttnet_image_desc records), and the largest height and
    width in the batch.  Move it with ``.to(device, non_blocking=True)``; ``DataLoader(pin_memory=True)`` calls
    ``.pin_memory()``."""

    def __init__(self, data: torch.Tensor, desc: torch.Tensor, max_h: int, max_w: int):
        if data.dtype != torch.uint8 or data.dim() != 1 or desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 2:
            raise RuntimeError(f"RaggedU8: expected uint8 [bytes] and int64 [n,2], got {data.dtype} {tuple(data.shape)}, "
                               f"{desc.dtype} {tuple(desc.shape)}")
        if data.device != desc.device:
            raise RuntimeError(f"RaggedU8: data on {data.device}, descriptors on {desc.device}")
        self.data, self.desc, self.max_h, self.max_w = data, desc, int(max_h), int(max_w)

    def __len__(self) -> int:
        return self.desc.shape[0]

    @property
    def device(self) -> torch.device:
        return self.data.device

    def to(self, device, non_blocking: bool = False) -> "RaggedU8":
        return RaggedU8(self.data.to(device, non_blocking=non_blocking), self.desc.to(device, non_blocking=non_blocking),
                        self.max_h, self.max_w)

    def pin_memory(self) -> "RaggedU8":
        return RaggedU8(self.data.pin_memory(), self.desc.pin_memory(), self.max_h, self.max_w)

    def descriptors(self) -> np.ndarray:
        """The descriptors as a numpy record array (offset, h, w)."""
        return self.desc.cpu().numpy().view(DESC_DTYPE).reshape(-1)


def pack_u8(images: Sequence) -> RaggedU8:
    """HWC uint8 images (numpy arrays or CPU tensors) of any sizes -> one host ``RaggedU8``, images back to back
    in order.  Raises RuntimeError naming the first image that is not uint8 [h, w, 3] with 1 <= h, w <= MAX_SIDE."""
    n = len(images)
    if n < 1 or n > 65535:
        raise RuntimeError(f"pack_u8: expected 1 to 65535 images, got {n}")
    arrays = []
    for i, im in enumerate(images):
        if isinstance(im, torch.Tensor):
            if im.is_cuda:
                raise RuntimeError(f"pack_u8: image {i} is on {im.device}; pack decoded host images")
            im = im.numpy()
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            desc = f"{im.dtype} {tuple(im.shape)}" if isinstance(im, np.ndarray) else type(im).__name__
            raise RuntimeError(f"pack_u8: image {i} must be uint8 HWC [h, w, 3], got {desc}")
        if not (1 <= im.shape[0] <= MAX_SIDE and 1 <= im.shape[1] <= MAX_SIDE):
            raise RuntimeError(f"pack_u8: image {i} is {im.shape[1]}x{im.shape[0]}; sides must lie in [1, {MAX_SIDE}]")
        arrays.append(im)
    desc = np.zeros(n, dtype=DESC_DTYPE)
    sizes = np.array([a.size for a in arrays], dtype=np.int64)
    desc["offset"][1:] = np.cumsum(sizes)[:-1]
    desc["h"] = [a.shape[0] for a in arrays]
    desc["w"] = [a.shape[1] for a in arrays]
    data = torch.empty(int(sizes.sum()), dtype=torch.uint8)
    flat = data.numpy()
    for a, off, sz in zip(arrays, desc["offset"], sizes):
        flat[off:off + sz] = a.reshape(-1)           # (copies a non-contiguous view too)
    return RaggedU8(data, torch.from_numpy(desc.view(np.int64).reshape(n, 2)), int(desc["h"].max()), int(desc["w"].max()))


def collate_u8(batch):
    """``DataLoader`` ``collate_fn`` for ``(image, target)`` pairs of decoded uint8 HWC images of any sizes:
    returns ``(RaggedU8, targets)`` with the targets collated as the default collate does."""
    images, targets = zip(*batch)
    return pack_u8(images), torch.utils.data.default_collate(list(targets))


class _StickyCount:
    """A count the device adds to and the host learns of late: ``dev`` (int32 [n] on the device, handed to the
    kernels) and ``host``, its pinned mirror.  The call that may add to it frames itself with ``raise_pending`` and
    ``mirror``, neither of which synchronises: a count that an earlier call left shows in the mirror and is raised
    then.  ``read`` synchronises and is exact.  Nothing is raised or copied while a graph is being captured."""

    def __init__(self, device: torch.device, n: int, raiser):
        self.dev = torch.zeros(n, dtype=torch.int32, device=device)
        self.host = torch.zeros(n, dtype=torch.int32).pin_memory()
        self.raiser = raiser                       # raiser(count) raises the error that names element 0

    def raise_pending(self, capturing: bool):
        if not capturing and int(self.host[0]):
            count = int(self.host[0])
            self.dev[0].zero_()
            self.host[0] = 0
            self.raiser(count)

    def mirror(self, capturing: bool):
        if not capturing:
            self.host.copy_(self.dev, non_blocking=True)

    def read(self, clear: bool = True) -> List[int]:
        torch.cuda.synchronize(self.dev.device)
        counts = self.dev.cpu().tolist()
        if clear and any(counts):
            self.dev.zero_()
            self.host.zero_()
        return counts


def _raise_bad(count: int):
    raise RuntimeError(f"resize_center_crop_u8_ragged / resize_views_u8_ragged: {count} image or view descriptor(s) of an "
                       "earlier batch were out of bounds (h, w beyond max_h / max_w, bytes past the buffer, or a view that "
                       "include/ttnet.h calls invalid): their crops are zero")


# per device: the running count of bad descriptors
_bad: Dict[torch.device, _StickyCount] = {}


def check_ragged(device=None):
    """Synchronise ``device`` and raise if any ragged call on it met a bad descriptor (then clear the count).
    ``resize_center_crop_u8_ragged`` reports one on a later call without synchronising; call this after the
    last batch of a loop."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device in _bad:
        count = _bad[device].read()[0]
        if count:
            _raise_bad(count)


def resize_center_crop_u8_ragged(r: RaggedU8, resize: int = 256, crop: int = 224) -> torch.Tensor:
    """A ragged batch on a HIP device -> uint8 [n, crop, crop, 3] in input order, one asynchronous kernel launch
    (capturable in a graph).  A bad descriptor gives a zero crop and makes a later call raise (the device count is
    copied to the host after each call, without a synchronisation); ``check_ragged`` checks at once."""
    if not isinstance(r, RaggedU8):
        raise RuntimeError(f"expected a RaggedU8 (pack_u8 / collate_u8), got {type(r).__name__}")
    if not r.data.is_cuda:
        raise RuntimeError(f"the ragged batch is on {r.device}: move it with .to(device, non_blocking=True)")
    dev = r.data.device
    if dev not in _bad:
        _bad[dev] = _StickyCount(dev, 1, _raise_bad)
    bad = _bad[dev]
    capturing = torch.cuda.is_current_stream_capturing()
    bad.raise_pending(capturing)
    data = r.data if r.data.data_ptr() % 16 == 0 else r.data.clone()
    desc = r.desc.contiguous()
    n = len(r)
    out = torch.empty((n, crop, crop, 3), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().ttnet_resize_center_crop_u8_ragged(
            C.c_void_p(data.data_ptr()), data.numel(), C.c_void_p(desc.data_ptr()), n, r.max_h, r.max_w, int(resize),
            int(crop), C.c_void_p(out.data_ptr()), C.c_void_p(bad.dev.data_ptr()), C.c_void_p(stream)))
        bad.mirror(capturing)
    return out


# ttnet_view_desc (include/ttnet.h): int32[12], 48 bytes
VIEW_FIELDS = ("image", "flags", "bx", "by", "bw", "bh", "nw", "nh", "x0", "y0")
VIEW_FAMILIES = _lib.VIEW_FAMILIES                         # name -> (TTNET_VIEWS_* code, views per image)


class Views:
    """View descriptors: ``desc`` (int32 [nv, 12], the 48-byte ttnet_view_desc records: image, flags, bx, by, bw, bh,
    nw, nh, x0, y0, 0, 0) and ``max_scale``, the bound on ``bw / nw`` and ``bh / nh`` that sizes the resize.  ``per_image``
    is V for the image-major families of ``eval_views`` (view ``i * V + v``), None for a free list."""

    def __init__(self, desc: torch.Tensor, max_scale: float, per_image: "int | None" = None):
        if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 12:
            raise RuntimeError(f"Views: expected int32 [nv, 12], got {desc.dtype} {tuple(desc.shape)}")
        if not max_scale >= 1.0:
            raise RuntimeError(f"Views: max_scale must be at least 1, got {max_scale}")
        self.desc, self.max_scale, self.per_image = desc, float(max_scale), per_image

    def __len__(self) -> int:
        return self.desc.shape[0]

    @property
    def device(self) -> torch.device:
        return self.desc.device

    def to(self, device, non_blocking: bool = False) -> "Views":
        return Views(self.desc.to(device, non_blocking=non_blocking), self.max_scale, self.per_image)

    def pin_memory(self) -> "Views":
        return Views(self.desc.pin_memory(), self.max_scale, self.per_image)

    def records(self) -> np.ndarray:
        """The descriptors on the host, int32 [nv, 12]."""
        return self.desc.cpu().numpy()


def _family(family: str) -> Tuple[int, int]:
    if family not in VIEW_FAMILIES:
        raise ValueError(f"views must be one of {', '.join(sorted(VIEW_FAMILIES))}, got {family!r}")
    return VIEW_FAMILIES[family]


def _check_resize_crop(resize: int, crop: int):
    if crop < 1 or resize < crop:
        raise ValueError(f"resize {resize} must be at least crop {crop} >= 1 (torchvision would pad)")


def make_views(records: Sequence, sizes: Sequence[Tuple[int, int]], crop: int = 224) -> Views:
    """Views from explicit boxes, on the host: what a caller with regions of interest or augmentation boxes (a
    RandomResizedCrop sampler of its own, say) passes to ``resize_views_u8_ragged``.  A record is a mapping with the keys
    ``image, bx, by, bw, bh`` and optionally ``nw, nh`` (default ``crop``), ``x0, y0`` (default 0), ``flip`` (default
    False), or the ten numbers ``(image, flags, bx, by, bw, bh, nw, nh, x0, y0)``; ``sizes[i]`` is ``(h, w)`` of image
    i.  Raises ValueError naming the first record and field that is not valid (include/ttnet.h: when a view is valid);
    ``max_scale`` is the largest ``bw / nw``, ``bh / nh`` among them, at least 1."""
    n = len(records)
    if n < 1 or n > 65535:
        raise ValueError(f"make_views: expected 1 to 65535 records, got {n}")
    if crop < 1:
        raise ValueError(f"make_views: crop must be positive, got {crop}")
    desc = np.zeros((n, 12), dtype=np.int32)
    max_scale = 1.0
    for k, rec in enumerate(records):
        if isinstance(rec, dict):
            unknown = set(rec) - set(VIEW_FIELDS) - {"flip"}
            if unknown or "flags" in rec:
                raise ValueError(f"make_views: record {k} has unknown keys {sorted(unknown | ({'flags'} & set(rec)))}")
            missing = [f for f in ("image", "bx", "by", "bw", "bh") if f not in rec]
            if missing:
                raise ValueError(f"make_views: record {k} lacks {missing}")
            v = [rec["image"], 1 if rec.get("flip", False) else 0, rec["bx"], rec["by"], rec["bw"], rec["bh"],
                 rec.get("nw", crop), rec.get("nh", crop), rec.get("x0", 0), rec.get("y0", 0)]
        else:
            v = list(rec)
            if len(v) != 10:
                raise ValueError(f"make_views: record {k} must be a mapping or the ten numbers {VIEW_FIELDS}, got {len(v)} values")
        for name, x in zip(VIEW_FIELDS, v):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not -2 ** 31 <= int(x) < 2 ** 31:
                raise ValueError(f"make_views: record {k}: {name} must be an int32, got {x!r}")
        image, flags, bx, by, bw, bh, nw, nh, x0, y0 = (int(x) for x in v)
        if not 0 <= image < len(sizes):
            raise ValueError(f"make_views: record {k}: image {image} outside [0, {len(sizes)})")
        h, w = (int(s) for s in sizes[image])
        if flags & ~1:
            raise ValueError(f"make_views: record {k}: flags {flags} has bits other than bit 0 (flip)")
        if bw < 1 or bx < 0 or bx + bw > w:
            raise ValueError(f"make_views: record {k}: box columns [{bx}, {bx} + {bw}) outside the image's {w}")
        if bh < 1 or by < 0 or by + bh > h:
            raise ValueError(f"make_views: record {k}: box rows [{by}, {by} + {bh}) outside the image's {h}")
        if not (1 <= nw <= 65536 and 1 <= nh <= 65536):
            raise ValueError(f"make_views: record {k}: resized size {nw}x{nh} outside [1, 65536]")
        if x0 < 0 or x0 + crop > nw:
            raise ValueError(f"make_views: record {k}: window columns [{x0}, {x0} + {crop}) outside the resized {nw}")
        if y0 < 0 or y0 + crop > nh:
            raise ValueError(f"make_views: record {k}: window rows [{y0}, {y0} + {crop}) outside the resized {nh}")
        desc[k, :10] = (image, flags, bx, by, bw, bh, nw, nh, x0, y0)
        max_scale = max(max_scale, bw / nw, bh / nh)
    return Views(torch.from_numpy(desc), max_scale)


def eval_views_host(sizes: Sequence[Tuple[int, int]], family: str, resize: int = 256, crop: int = 224) -> Views:
    """The numpy twin of ``eval_views`` for ``sizes`` = ``[(h, w), ..]``: the same descriptors, computed on the host.
    For comparison (tests, tools) only -- the product's views come from the device generator."""
    code, V = _family(family)
    _check_resize_crop(resize, crop)
    desc = np.zeros((len(sizes) * V, 12), dtype=np.int32)
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            desc[i * V:(i + 1) * V, 0] = i                 # (not decoded: invalid views)
            continue
        nh, nw = h, w
        if not ((w <= h and w == resize) or (h <= w and h == resize)):
            nh, nw = (int(resize * h / w), resize) if w <= h else (resize, int(resize * w / h))
        mx, my = nw - crop, nh - crop
        cx, cy = int(round(mx / 2.0)), int(round(my / 2.0))
        five = [(0, 0, 0), (mx, 0, 0), (0, my, 0), (mx, my, 0), (cx, cy, 0)]
        windows = {"center": [(cx, cy, 0)], "flip": [(cx, cy, 0), (mx - cx, cy, 1)], "five": five,
                   "ten": five + [(mx, 0, 1), (0, 0, 1), (mx, my, 1), (0, my, 1), (mx - cx, cy, 1)]}[family]
        for v, (x0, y0, flip) in enumerate(windows):
            desc[i * V + v, :10] = (i, flip, 0, 0, w, h, nw, nh, x0, y0)
    max_h, max_w = max(int(s[0]) for s in sizes), max(int(s[1]) for s in sizes)
    return Views(torch.from_numpy(desc), _lib.load().ttnet_eval_views_max_scale(max(max_h, 1), max(max_w, 1), int(resize)), V)


def eval_views(r: RaggedU8, family: str, resize: int = 256, crop: int = 224) -> Views:
    """The ``family`` ("center": 1 view per image, "flip": 2, "five": 5, "ten": 10; include/ttnet.h) of every image of a
    ragged batch on the device, image-major, written by one small kernel from the image descriptors where they are
    (ttnet_make_eval_views: nothing is read back, so it follows ``decode_ragged`` without the host knowing any size).
    Asynchronous on the current stream, capturable."""
    code, V = _family(family)
    _check_resize_crop(resize, crop)
    if not isinstance(r, RaggedU8) or not r.data.is_cuda:
        raise RuntimeError("eval_views: expected a RaggedU8 on a HIP device (the generator has no CPU path; eval_views_host "
                           "restates it for comparison)")
    n = len(r)
    if n * V > 65535:
        raise RuntimeError(f"eval_views: {n} images x {V} views exceed 65535 views per call")
    dev = r.data.device
    idesc = r.desc.contiguous()
    desc = torch.empty((n * V, 12), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        lib = _lib.load()
        _lib.check(lib.ttnet_make_eval_views(C.c_void_p(idesc.data_ptr()), n, int(resize), int(crop), code,
                                             C.c_void_p(desc.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return Views(desc, lib.ttnet_eval_views_max_scale(r.max_h, r.max_w, int(resize)), V)


def resize_views_u8_ragged(r: RaggedU8, views: Views, crop: int = 224) -> torch.Tensor:
    """The views of a ragged batch, both on a HIP device -> uint8 [nv, crop, crop, 3] in view order: one asynchronous
    kernel launch (ttnet_resize_views_u8_ragged), capturable.  An invalid view gives a zero crop and is added to the
    count ``resize_center_crop_u8_ragged`` keeps: a later call of either raises, ``check_ragged`` checks at once."""
    if not isinstance(r, RaggedU8) or not isinstance(views, Views):
        raise RuntimeError(f"expected a RaggedU8 and Views, got {type(r).__name__} and {type(views).__name__}")
    if not r.data.is_cuda or views.device != r.data.device:
        raise RuntimeError(f"the ragged batch is on {r.device}, the views on {views.device}: move both to one HIP device")
    dev = r.data.device
    if dev not in _bad:
        _bad[dev] = _StickyCount(dev, 1, _raise_bad)
    bad = _bad[dev]
    capturing = torch.cuda.is_current_stream_capturing()
    bad.raise_pending(capturing)
    data = r.data if r.data.data_ptr() % 16 == 0 else r.data.clone()
    idesc = r.desc.contiguous()
    vdesc = views.desc.contiguous()
    if vdesc.data_ptr() % 16:
        vdesc = vdesc.clone()
    nv = len(views)
    out = torch.empty((nv, crop, crop, 3), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().ttnet_resize_views_u8_ragged(
            C.c_void_p(data.data_ptr()), data.numel(), C.c_void_p(idesc.data_ptr()), len(r), C.c_void_p(vdesc.data_ptr()), nv,
            views.max_scale, int(crop), C.c_void_p(out.data_ptr()), C.c_void_p(bad.dev.data_ptr()), C.c_void_p(stream)))
        bad.mirror(capturing)
    return out


def _check_mean_args(shape, V: int):
    if not 1 <= V <= _lib.VIEWS_MAX:
        raise ValueError(f"mean_views: V must be in [1, {_lib.VIEWS_MAX}], got {V}")
    if len(shape) != 2 or shape[0] < V or shape[0] % V:
        raise ValueError(f"mean_views: expected logits [n * {V}, n_classes], got {tuple(shape)}")


def mean_views(logits: torch.Tensor, V: int) -> torch.Tensor:
    """float32 HIP logits ``[n * V, C]`` (image-major) -> ``[n, C]``: the mean over each image's V rows, summed in
    ascending view order in float64 (ttnet_mean_views) -- torchvision's ``outputs.view(n, V, -1).mean(1)`` with a stated
    order.  One asynchronous launch, capturable."""
    if (not logits.is_cuda) or logits.dtype != torch.float32:
        raise RuntimeError(f"expected float32 HIP logits, got {logits.dtype} on {logits.device}: ttnet_mean_views has no CPU "
                           "path (mean_views_host restates it for comparison)")
    _check_mean_args(logits.shape, V)
    logits = logits.contiguous()
    n, c = logits.shape[0] // V, logits.shape[1]
    out = torch.empty((n, c), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        stream = torch.cuda.current_stream(logits.device).cuda_stream
        _lib.check(_lib.load().ttnet_mean_views(C.c_void_p(logits.data_ptr()), n, int(V), c, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(stream)))
    return out


def mean_views_host(logits, V: int) -> np.ndarray:
    """The same arithmetic in numpy (float64 sum in ascending view order, one division, rounded to float32): for
    comparison only."""
    x = np.asarray(logits.cpu() if isinstance(logits, torch.Tensor) else logits, dtype=np.float32)
    _check_mean_args(x.shape, V)
    x = x.reshape(x.shape[0] // V, V, x.shape[1])
    acc = np.zeros((x.shape[0], x.shape[2]), dtype=np.float64)
    for v in range(V):
        acc += x[:, v].astype(np.float64)
    return (acc / np.float64(V)).astype(np.float32)


def resize_center_crop_u8(x_u8: torch.Tensor, resize: int = 256, crop: int = 224) -> torch.Tensor:
    """uint8 HIP tensor [N,H,W,3] (one image size per call, as a decoder batch delivers) ->
    uint8 [N,crop,crop,3]."""
    if (not x_u8.is_cuda) or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3:
        raise RuntimeError(f"expected a uint8 HIP tensor [N,H,W,3], got {x_u8.dtype} {tuple(x_u8.shape)} on {x_u8.device}")
    x_u8 = x_u8.contiguous()
    n, h, w, _ = x_u8.shape
    out = torch.empty((n, crop, crop, 3), device=x_u8.device, dtype=torch.uint8)
    with torch.cuda.device(x_u8.device):
        stream = torch.cuda.current_stream(x_u8.device).cuda_stream
        _lib.check(_lib.load().ttnet_resize_center_crop_u8(C.c_void_p(x_u8.data_ptr()), n, h, w, int(resize), int(crop),
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out


def imgnet_eval_forward(model, x_u8, lane: int = 0) -> torch.Tensor:
    """``model(imgnet_transform(False)(image))`` for a batch of decoded images: of one size (uint8 [N,H,W,3]), or
    of mixed sizes (``RaggedU8`` on the device, from ``collate_u8``)."""
    if isinstance(x_u8, RaggedU8):
        return model.forward_u8(resize_center_crop_u8_ragged(x_u8), lane=lane)
    return model.forward_u8(resize_center_crop_u8(x_u8), lane=lane)


def imgnet_views_forward(model, r: RaggedU8, family: str, lane: int = 0) -> torch.Tensor:
    """Multi-crop evaluation of a ragged batch on the device: ``Resize(256)`` -> the ``family`` of 224 crops ("flip",
    "five", "ten"; "center" is ``imgnet_eval_forward``) -> ``forward_u8`` on all ``n * V`` crops -> the mean of each
    image's V rows of logits, ``[n, n_classes]``.  Size the plan for ``n * V`` (``model.reserve``)."""
    views = eval_views(r, family)
    return mean_views(model.forward_u8(resize_views_u8_ragged(r, views), lane=lane), views.per_image)
