"""Shared by tests/test_attack_cpu.py and tests/test_gpu_attack.py: the synthetic checkpoint, the 64 synthetic images, the
float64 oracle forward in the shape ``attack_cpu`` wants, and cached runs of the twin (test infrastructure; imports oracle/)."""
from functools import lru_cache

import numpy as np

from _certify_util import normalise, oracle_pre
from _util import spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import attack as AT
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import cifar, synth

N = 64
STD16 = (16.0, 16.0, 16.0)          # one byte level is small in normalised space: certified, falsified and open images at once
NORMS = {"cifar": (cifar.CIFAR_MEAN, cifar.CIFAR_STD), "std16": (cifar.CIFAR_MEAN, STD16)}


@lru_cache(maxsize=None)
def setup():
    spec, st = spec_and_state("valexnet")
    luts, near = OB.build_all_luts(st, spec)
    assert not any(v.any() for v in near.values())
    return spec, st, luts


@lru_cache(maxsize=None)
def images_np(n=N):
    a = np.ascontiguousarray(synth.synth_images_u8(n, hw=(32, 32)).transpose(0, 2, 3, 1))
    a.setflags(write=False)
    return a


def oracle_forward(norm: str):
    """``forward`` for ``attack_cpu``: uint8 images -> (stem bits, feature bits, float32 logits) of the float64 oracle."""
    spec, st, luts = setup()
    mean, std = NORMS[norm]

    def forward(x_u8):
        bits = (oracle_pre(st, normalise(np.asarray(x_u8).astype(np.float64), mean, std)) >= 0).astype(np.uint8)
        y, logits = OB.valexnet_from_stem_bits(bits, st, spec, luts)
        return bits, y, logits.astype(np.float32)
    return forward


@lru_cache(maxsize=None)
def nominal(norm: str, n=N):
    """(stem bits, feature bits, logits, classes) of the oracle on the images themselves."""
    bits, y, logits = oracle_forward(norm)(images_np(n))
    return bits, y, logits, logits.argmax(axis=1)


@lru_cache(maxsize=None)
def twin_attack(norm: str, eps: int, rounds: int = 3, min_margin: float = 0.0):
    """(records, witnesses) of ``attack_cpu`` through the oracle forward, on the oracle's own classes."""
    _, st, luts = setup()
    mean, std = NORMS[norm]
    return AT.attack_cpu(st, luts, images_np(), nominal(norm)[3], eps, rounds, min_margin, forward=oracle_forward(norm), mean=mean, std=std)


@lru_cache(maxsize=None)
def twin_certify(norm: str, eps: float):
    _, st, luts = setup()
    mean, std = NORMS[norm]
    return CF.certify_cpu(st, luts, images_np(), nominal(norm)[3], eps, mean=mean, std=std)


def box(x0: np.ndarray, levels: int):
    x = x0.astype(np.int64)
    return np.maximum(0, x - levels).astype(np.uint8), np.minimum(255, x + levels).astype(np.uint8)


def runner_up(logits: np.ndarray, classes: np.ndarray) -> np.ndarray:
    other = np.array(logits, dtype=np.float64)
    other[np.arange(len(classes)), classes] = -np.inf
    return other.argmax(axis=1)


def threshold_band(scores: np.ndarray, rel: float = 2.0 ** -40) -> np.ndarray:
    """bool like ``scores`` ([n, 2, 32, 32, 3]): bytes whose score lies within ``rel * M`` of a decision threshold of the
    candidates (zero, or ``tau * M``).  A score that is exactly zero is a byte that no pushed stem bit reaches (row and column
    31, fields without an unknown bit): an empty sum on either side, not a near tie."""
    M = np.abs(scores).reshape(scores.shape[0], 2, -1).max(axis=2)[:, :, None, None, None]
    band = np.zeros(scores.shape, dtype=bool)
    for tau in AT.TAUS:
        band |= np.abs(np.abs(scores) - tau * M) <= rel * M
    return band & (scores != 0)
