"""Shared by tests/test_attack_patch_cpu.py and tests/test_gpu_attack_patch.py: cached runs of the patch twin through the
float64 oracle forward, the oracle's margin of a batch of images, and the random-corner baseline (test infrastructure)."""
from functools import lru_cache

import numpy as np

from _attack_util import NORMS, images_np, nominal, oracle_forward, setup
from scale_imagenet_amd import attack as AT
from scale_imagenet_amd import certify as CF

IMAGES = (0, 1, 7)                  # mostly falsifiable, mixed and robust positions on the synthetic checkpoint
LOGIT_TOL = 1e-5


def images3():
    return np.ascontiguousarray(images_np()[list(IMAGES)])


def classes3(norm: str) -> np.ndarray:
    return np.asarray(nominal(norm)[3])[list(IMAGES)]


@lru_cache(maxsize=None)
def twin(norm: str, patch, stride: int, amp: int, rounds: int = 2, min_margin: float = 0.0, confirm: str = "all"):
    """``attack_patch_cpu`` on images 0, 1, 7 with the oracle's own classes, judged by the oracle forward."""
    _, st, luts = setup()
    mean, std = NORMS[norm]
    return AT.attack_patch_cpu(st, luts, images3(), classes3(norm), patch, stride, amp, rounds, min_margin,
                               forward=oracle_forward(norm), mean=mean, std=std, confirm=confirm)


def tolerance() -> float:
    """``1e-9 * sum|A|``: the sweep twin's tolerance for two float64 summation orders of the same real number."""
    return 1e-9 * float(np.abs(AT.head_cpu(setup()[1])).sum())


def oracle_margins(norm: str, x_u8: np.ndarray, classes: np.ndarray, chunk: int = 512) -> np.ndarray:
    """float64 ``logit_c - max_{j != c} logit_j`` of the oracle forward (its logits are float32 values)."""
    fwd = oracle_forward(norm)
    out = np.empty(len(x_u8))
    for a in range(0, len(x_u8), chunk):
        l = fwd(x_u8[a:a + chunk])[2].astype(np.float64)
        c = np.asarray(classes[a:a + chunk])
        own = l[np.arange(len(c)), c]
        l[np.arange(len(c)), c] = -np.inf
        out[a:a + chunk] = own - l.max(axis=1)
    return out


def witnesses(res) -> np.ndarray:
    """Every (image, position) of a result pasted: uint8 ``[n * P, 32, 32, 3]``."""
    n, py, px = res.map.shape
    return AT.paste_cpu(res.x0, res.patch, res.stride, res.fills_numpy(), np.arange(n * py * px))


def random_corner_falsified(norm: str, patch, stride: int, amp: int, budget: int, min_margin: float = 0.0, seed: int = 20251021) -> np.ndarray:
    """bool ``[3, P]``: positions at which one of ``budget`` random per-byte corners of the patch's box loses the class by
    the oracle forward.  Fixed seed."""
    h, w = patch
    x, cls = images3(), classes3(norm)
    org = CF.patch_origins(patch, stride)
    rng = np.random.default_rng(seed)
    out = np.zeros((len(x), len(org)), dtype=bool)
    for i in range(len(x)):
        b = x[i].astype(np.int64)
        imgs = np.broadcast_to(x[i], (len(org), budget, 32, 32, 3)).copy()
        for p, (y0, x0) in enumerate(org):
            hi = rng.integers(0, 2, size=(budget, h, w, 3)).astype(bool)
            box = b[y0:y0 + h, x0:x0 + w]
            imgs[p, :, y0:y0 + h, x0:x0 + w] = np.where(hi, np.minimum(255, box + amp), np.maximum(0, box - amp))
        m = oracle_margins(norm, imgs.reshape(-1, 32, 32, 3), np.full(len(org) * budget, cls[i]))
        out[i] = (m.reshape(len(org), budget) < -min_margin).any(axis=1)
    return out
