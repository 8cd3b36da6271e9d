"""Inputs and BatchNorm parameters beyond the synthetic ones for the stem, and the near-tie band that scales with them
(test infrastructure; shared by tests/test_stem_split_bound_cpu.py and tests/test_gpu_stem_values.py).

The band.  The stem carries every float32 operand as two fp16 terms and keeps three of the four products
(scale_imagenet_amd/csrc/stem.hip), so its pre-activation is off by a small multiple of 2^-22 of the sum of the
MAGNITUDES of its terms,  E = sum_taps |w * scale| * |pooled x| + |shift|  (oracle/ttnet_bits.py: stem_pre64_cond), whatever
cancels inside the sum.  OB.NEAR_TIE = 1e-5 was stated for the synthetic model on the synthetic images, where E is at
most E0 (about 49: computed here from the oracle on the 8 golden images, not a constant).  For other operands the band is

    tau(o) = NEAR_TIE * max(1, E(o) / E0)

which is never narrower than the flat band and grows only where an output's operands are larger than the synthetic ones.
"""
from functools import lru_cache

import numpy as np

from _util import spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import synth

BN = "features.2"
CASES = ["synthetic", "gaussian", "synthetic x 100", "synthetic x 1500", "synthetic x 1e-4", "gaussian + 300",
         "gamma x 2^(ch % 13 - 6), one negative, one zero", "running_var x 4^(ch % 13 - 6), running_mean x 20"]
BN_CASES = CASES[6:]
NEGATED_CHANNEL, ZERO_CHANNEL = 5, 9


@lru_cache(maxsize=None)
def e0() -> float:
    """The largest E of the synthetic configuration on its 8 golden images."""
    _, st = spec_and_state("small")
    return float(OB.stem_pre64_cond(synth.synth_images(8), st)[1].max())


def tau(E: np.ndarray) -> np.ndarray:
    return OB.NEAR_TIE * np.maximum(1.0, E / e0())


def oracle_rows(x: np.ndarray, st, scaled: bool = False, chunk: int = 16):
    """The float64 oracle over images x in the form the GPU tests compare: (want, band) as row-packed uint64 [N,p,56]
    -- bit x of want is (pre >= 0), bit x of band is |pre| < tau (``scaled``) or |pre| < NEAR_TIE.  Both read-only."""
    want, band = [], []
    for i0 in range(0, x.shape[0], chunk):
        pre, E = OB.stem_pre64_cond(x[i0:i0 + chunk], st, chunk=chunk, cond=scaled)
        want.append(OB.pack_rows((pre >= 0).astype(np.uint8)))
        band.append(OB.pack_rows((np.abs(pre) < (tau(E) if scaled else OB.NEAR_TIE)).astype(np.uint8)))
    want, band = np.concatenate(want), np.concatenate(band)
    want.setflags(write=False)
    band.setflags(write=False)
    return want, band


def count_bits(words: np.ndarray) -> int:
    nz = words[words != 0]
    return int(OB.unpack_rows(nz, 64).sum()) if nz.size else 0


def check_rows(rows: np.ndarray, want: np.ndarray, band: np.ndarray, what: str) -> int:
    """Every bit of the GPU's rows equals the oracle's outside the band.  Returns the number of differing bits inside."""
    assert rows.shape == want.shape == band.shape, (what, rows.shape, want.shape)
    diff = rows ^ want
    outside = diff & ~band
    if outside.any():
        n, ch, y = (int(v) for v in np.argwhere(outside)[0])
        xs = np.flatnonzero(OB.unpack_rows(outside[n, ch, y], 56)).tolist()
        images = np.flatnonzero(outside.reshape(len(outside), -1).any(axis=1))
        raise AssertionError(f"{what}: {count_bits(outside)} bits differ from the float64 oracle outside the near-tie band, in "
                             f"{len(images)} of {len(rows)} images (first {images[:8].tolist()}); first at image {n} (items "
                             f"{7 * n} .. {7 * n + 6}), channel {ch}, row {y} (row block {y // 8}), columns {xs[:8]}")
    return count_bits(diff)


def case_state(name: str):
    """The state dict of a case: the synthetic one, or a copy with the stem's BatchNorm changed."""
    _, st = spec_and_state("small")
    if name not in BN_CASES:
        return st
    st = {k: v.copy() for k, v in st.items()}
    p = st[f"{BN}.weight"].shape[0]
    e = (np.arange(p) % 13 - 6).astype(np.float64)
    if name == BN_CASES[0]:
        g = st[f"{BN}.weight"].astype(np.float64) * 2.0 ** e
        g[NEGATED_CHANNEL] = -g[NEGATED_CHANNEL]
        g[ZERO_CHANNEL] = 0.0
        st[f"{BN}.weight"] = g.astype(np.float32)
    else:
        st[f"{BN}.running_var"] = (st[f"{BN}.running_var"].astype(np.float64) * 4.0 ** e).astype(np.float32)
        st[f"{BN}.running_mean"] = (st[f"{BN}.running_mean"] * np.float32(20.0)).astype(np.float32)
    return st


def case_images(name: str, n: int) -> np.ndarray:
    """float32 [n,3,224,224]; the first images of a larger n are the images of a smaller one."""
    if name.startswith("gaussian"):
        x = np.empty((n, 3, 224, 224), dtype=np.float32)
        for i in range(n):                                    # (one stream per image: a prefix stays a prefix)
            x[i] = np.random.default_rng(4000 + i).standard_normal((3, 224, 224), dtype=np.float32)
        return x + np.float32(300.0) if name.endswith("300") else x
    x = synth.synth_images(n)
    factor = {"synthetic x 100": 100.0, "synthetic x 1500": 1500.0, "synthetic x 1e-4": 1e-4}.get(name, 1.0)
    return (x * np.float32(factor)).astype(np.float32)
