"""ctypes binding of libttnet.so (include/ttnet.h).

There is no fallback: if the library is missing or a call fails, this raises.  The only
torch objects that reach the C ABI are raw ``data_ptr()`` addresses and the current HIP
stream handle.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libttnet.so")

TTNET_F32, TTNET_I64, TTNET_U8, TTNET_U16, TTNET_U64 = 0, 1, 2, 3, 4
TOPK_MAX = 32                                              # TTNET_TOPK_MAX
VIEWS_MAX = 32                                             # TTNET_VIEWS_MAX
VIEW_FAMILIES = {"center": (0, 1), "flip": (1, 2), "five": (2, 5), "ten": (3, 10)}     # TTNET_VIEWS_*: (code, views per image)
VARIANTS = {"small": 0, "xsmall": 1, "full": 2, "valexnet": 3}


class NetDesc(C.Structure):
    _fields_ = [("variant", C.c_int32), ("nfilter", C.c_int32), ("tfilter", C.c_int32),
                ("layers", C.c_int32), ("image_h", C.c_int32), ("image_w", C.c_int32),
                ("max_batch", C.c_int32), ("reserved", C.c_int32)]


class ImageDesc(C.Structure):
    """ttnet_image_desc: image i of a ragged batch is uint8 HWC [h][w][3] at byte ``offset`` of the source buffer."""
    _fields_ = [("offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32)]


class JpegDesc(C.Structure):
    """ttnet_jpeg_desc: one image of a JPEG batch (include/ttnet.h), 80 bytes."""
    _fields_ = [("data_offset", C.c_int64), ("data_bytes", C.c_int64), ("table_offset", C.c_int64),
                ("out_offset", C.c_int64), ("block_offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32),
                ("kind", C.c_int32), ("ncomp", C.c_int32), ("restart_interval", C.c_int32),
                ("comp", (C.c_uint8 * 4) * 3), ("reserved", C.c_int32 * 2)]


class JpegScan(C.Structure):
    """ttnet_jpeg_scan: one scan of a progressive image (include/ttnet.h), 32 bytes."""
    _fields_ = [("data_offset", C.c_uint32), ("data_bytes", C.c_uint32), ("restart_interval", C.c_uint16),
                ("ncomp", C.c_uint8), ("slot", C.c_uint8), ("comp", C.c_uint8 * 4), ("ss", C.c_uint8), ("se", C.c_uint8),
                ("ah", C.c_uint8), ("al", C.c_uint8), ("table", C.c_uint8 * 4), ("reserved", C.c_int32 * 2)]


class EvalAcc(C.Structure):
    """ttnet_eval_acc: the device-resident accumulator of ttnet_eval_metrics (include/ttnet.h), 64 bytes."""
    _fields_ = [("loss_sum", C.c_double), ("images", C.c_int64), ("hits1", C.c_int64), ("hits5", C.c_int64),
                ("bad_targets", C.c_int64), ("reserved", C.c_int64 * 3)]


class TTNetError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libttnet status {status}: {message}")
        self.status = status


# every symbol include/ttnet.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS: List[Tuple[str, object, list]] = [
    ("ttnet_plan_create", C.c_int, [C.POINTER(NetDesc), C.c_int, C.POINTER(_P)]),
    ("ttnet_plan_set_tensor", C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int]),
    ("ttnet_plan_finalize", C.c_int, [_P, _P]),
    ("ttnet_forward", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("ttnet_plan_set_lanes", C.c_int, [_P, C.c_int]),
    ("ttnet_forward_lane", C.c_int, [_P, C.c_int, _P, C.c_int64, _P, _P]),
    ("ttnet_plan_set_input_norm", C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("ttnet_forward_u8", C.c_int, [_P, C.c_int, _P, C.c_int64, _P, _P]),
    ("ttnet_resize_center_crop_u8", C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("ttnet_resize_center_crop_u8_ragged", C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                                     _P, _P, _P]),
    ("ttnet_resize_views_u8_ragged", C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_double, C.c_int, _P, _P, _P]),
    ("ttnet_make_eval_views", C.c_int, [_P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("ttnet_eval_views_max_scale", C.c_double, [C.c_int, C.c_int, C.c_int]),
    ("ttnet_mean_views", C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P]),
    ("ttnet_jpeg_ctx_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("ttnet_jpeg_ctx_reserve", C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64]),
    ("ttnet_jpeg_decode_ragged", C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    ("ttnet_jpeg_ctx_destroy", None, [_P]),
    ("ttnet_eval_metrics", C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P, _P]),
    ("ttnet_topk_rows", C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _P, _P]),
    ("ttnet_class_counts", C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P]),
    ("ttnet_forward_from_stem_bits", C.c_int, [_P, _P, C.c_int64, _P, _P]),
    ("ttnet_read_stage", C.c_int, [_P, C.c_char_p, C.c_int64, _P, C.c_size_t, C.c_int, _P]),
    ("ttnet_plan_get_table", C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    ("ttnet_plan_set_table", C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    ("ttnet_plan_table_usage_enable", C.c_int, [_P, C.c_int]),
    ("ttnet_plan_table_usage_reset", C.c_int, [_P, _P]),
    ("ttnet_table_usage_add", C.c_int, [_P, C.c_int, _P]),
    ("ttnet_plan_get_table_usage", C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    ("ttnet_plan_set_care", C.c_int, [_P, C.c_char_p, _P, C.c_size_t]),
    ("ttnet_plan_clear_care", C.c_int, [_P]),
    ("ttnet_care_misses", C.c_int, [_P, C.c_int, _P, _P]),
    ("ttnet_minimise_workspace", C.c_int64, [C.c_int, C.c_int64]),
    ("ttnet_minimise_covers", C.c_int, [_P, _P, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    ("ttnet_minimise_rounds_workspace", C.c_int64, [C.c_int, C.c_int64]),
    ("ttnet_minimise_covers_rounds", C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    ("ttnet_cover_support_workspace", C.c_int64, [C.c_int, C.c_int64]),
    ("ttnet_cover_support", C.c_int, [_P, _P, C.c_int64, _P, _P, _P, C.c_int64, C.c_int, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int64, _P]),
    ("ttnet_certify_u8", C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_double, C.c_int, C.c_double, _P, _P, _P]),
    ("ttnet_certify_box_u8", C.c_int, [_P, C.c_int, _P, _P, C.c_int64, _P, C.c_int, C.c_double, _P, _P, _P]),
    ("ttnet_certify_patch_u8", C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P]),
    ("ttnet_attack_patch_u8", C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _P, _P, _P]),
    ("ttnet_patch_paste_u8", C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int64, _P, _P]),
    ("ttnet_attack_propose_u8", C.c_int, [_P, C.c_int, _P, _P, C.c_int64, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    ("ttnet_attack_select_u8", C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, C.c_double, _P, _P, _P, _P, _P, C.c_int, _P]),
    ("ttnet_plan_query", C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    ("ttnet_launch_partition", C.c_int, [C.c_char_p, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.c_int]),
    ("ttnet_plan_set_profiling", C.c_int, [_P, C.c_int]),
    ("ttnet_plan_last_timings", C.c_int, [_P, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]),
    ("ttnet_plan_destroy", None, [_P]),
    ("ttnet_comm_unique_id", C.c_int, [_P]),
    ("ttnet_comm_create", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("ttnet_allgather_logits", C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, _P]),
    ("ttnet_comm_destroy", None, [_P]),
    ("ttnet_last_error", C.c_char_p, []),
    ("ttnet_version", C.c_char_p, []),
]

_lib = None


def load() -> C.CDLL:
    """Load libttnet.so (once).  Raises if it has not been built: there is no other path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m scale_imagenet_amd.build` "
            "(hipcc, gfx950).  scale_imagenet_amd has no CPU or eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int) -> int:
    if status < 0:
        raise TTNetError(status, load().ttnet_last_error().decode("utf-8", "replace"))
    return status


def launch_partition(what: str, *args: int) -> Tuple[int, ...]:
    """ttnet_launch_partition: the launch arithmetic of csrc/partition.h by name (no plan, no device)."""
    a = (C.c_int64 * max(1, len(args)))(*args)
    out = (C.c_int64 * 8)()
    return tuple(out[:check(load().ttnet_launch_partition(what.encode(), a, len(args), out, len(out)))])
