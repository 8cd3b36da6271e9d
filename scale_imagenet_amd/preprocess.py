"""GPU side of the reference's eval input transform (utils/preprocess.py:104-108, main.py:208):

    transforms.Resize(256) -> transforms.CenterCrop(224) -> transforms.ToTensor() -> transforms.Normalize(mean, std)

``resize_center_crop_u8`` does the first two on decoded uint8 HWC images already on the device
(libttnet: ttnet_resize_center_crop_u8, csrc/preproc.hip); the last two are fused into the stem by
``model.forward_u8``.  JPEG decoding from file bytes runs on the device too (``jpeg.py``: ``decode_ragged``,
``jpeg_eval_forward``).

A decoder batch of ImageNet images has many sizes.  ``pack_u8`` / ``collate_u8`` put such a batch into one flat
buffer plus descriptors (``RaggedU8``), and ``resize_center_crop_u8_ragged`` resizes and crops all of it in one
launch (ttnet_resize_center_crop_u8_ragged), in input order.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence

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
    raise RuntimeError(f"resize_center_crop_u8_ragged: {count} image descriptor(s) of an earlier batch were out of "
                       "bounds (h, w beyond max_h / max_w or bytes past the buffer): their crops are zero")


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
