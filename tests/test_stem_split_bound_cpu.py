"""The near-tie band that scales with the operands, pinned on the CPU (no GPU needed).

tests/_stem_cases.py states the band  tau(o) = NEAR_TIE * max(1, E(o) / E0).  Here the split arithmetic of
scale_imagenet_amd/csrc/stem.hip is emulated in numpy -- the float32 pooled value x 16 as two fp16 terms, float32(w * scale)
x the tensor's power-of-two prescale as two fp16 terms, the BatchNorm shift as the 22nd k-row, the three kept products --
and summed in float64.  For every case of tests/_stem_cases.py (full mantissas, large offsets, tiny magnitudes, BatchNorm
scales 2^12 apart, a negative and a zero gamma) the emulated pre-activation stays within half the band of the float64
oracle, the band holds at most 1e-4 of the outputs, and the bits are not nearly constant.  Measured, 4 images:

    case                                              err / tau    share in band
    synthetic                                           0.10          7e-6
    gaussian (full mantissas)                           0.06          1e-5
    synthetic x 100                                     0.33          1e-6
    synthetic x 1500 (pooled x 16 up to 55,000)         0.29          0
    synthetic x 1e-4                                    0.002         0
    gaussian + 300                                      0.24          0
    gamma x 2^(ch % 13 - 6), one negative, one zero     0.28          2e-5
    running_var x 4^(ch % 13 - 6), running_mean x 20    0.25          7e-6

What the emulation leaves out is the float32 accumulation inside the MFMAs (33 instructions on one accumulator): that
part is measured on the GPU alone, by tests/test_gpu_stem_values.py against the same band.
"""
import numpy as np
import pytest

import _stem_cases as SC
from _util import spec_and_state
from oracle import ttnet_bits as OB
from scale_imagenet_amd import synth

N = 4
X_PRESCALE = 16.0


def test_cond_oracle_equals_stem_pre64():
    _, st = spec_and_state("small")
    x = synth.synth_images(N)
    ref = OB.stem_pre64(x, st)
    pre, E = OB.stem_pre64_cond(x, st, chunk=3)           # (a last chunk of one image)
    assert pre.shape == E.shape == ref.shape
    assert np.abs(pre - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (E >= np.abs(pre) * (1 - 1e-12)).all()
    # E from its definition, on one image
    x64 = x[:1].astype(np.float64)
    pooled = 0.25 * (x64[:, :, 0::2, 0::2] + x64[:, :, 0::2, 1::2] + x64[:, :, 1::2, 0::2] + x64[:, :, 1::2, 1::2])
    s, t = OB.fold_bn(st, "features.2")
    mag = {"features.1.weight": np.abs(st["features.1.weight"].astype(np.float64) * s[:, None, None, None]).astype(np.float64),
           "features.2.weight": np.ones_like(s, dtype=np.float64), "features.2.bias": np.abs(t),
           "features.2.running_mean": np.zeros_like(s), "features.2.running_var": np.full_like(s, 1.0 - OB.BN_EPS)}
    want = OB.stem_pre64(np.abs(pooled).repeat(2, axis=2).repeat(2, axis=3), mag)
    assert np.abs(E[:1] - want).max() <= 1e-12 * want.max()


def test_e0_is_the_synthetic_scale():
    assert 30.0 < SC.e0() < 80.0
    assert (SC.tau(np.array([0.0, SC.e0(), 3 * SC.e0()])) == OB.NEAR_TIE * np.array([1.0, 1.0, 3.0])).all()


def _split(v):
    """float64 -> the two fp16 terms (as float64) of float32(v): h1 = fp16(v), h2 = fp16(v - h1)."""
    v32 = v.astype(np.float32)
    h1 = v32.astype(np.float16).astype(np.float64)
    h2 = (v32.astype(np.float64) - h1).astype(np.float32).astype(np.float16).astype(np.float64)
    return h1, h2


def _weight_prescale(wf):
    amax = float(np.abs(wf).max())
    if not (amax > 0.0) or not np.isfinite(amax):
        return 1.0
    _, e = np.frexp(np.float32(amax))
    return float(2.0 ** int(np.clip(14 - int(e), -60, 60)))


def emulate(x, st):
    """The stem's pre-activation as the kernel forms it, but for a float64 sum of its exact fp16 x fp16 products."""
    w = st["features.1.weight"]
    p = w.shape[0]
    s, t = OB.fold_bn(st, "features.2")
    wf = (w.astype(np.float64).reshape(p, -1) * s[:, None]).astype(np.float32)           # BatchNorm scale folded in float32
    ws = _weight_prescale(wf)
    w1, w2 = _split(wf.astype(np.float64) * ws)
    # the shift row: constant c in two slots, shift / c in the first (two terms), what is left of it in the second
    sh = t * ws * X_PRESCALE
    amax, c = float(np.abs(sh).max()), 1.0
    while amax / c > 16384.0 and c < 32768.0:
        c *= 2.0
    assert amax / c <= 32768.0, "the folded shift does not fit the shift row"
    a1, a2 = _split(sh / c)
    b1, b2 = _split(sh / c - a1 - a2)
    shift_term = (a1 + a2 + b1 + b2) * c
    # pooled exactly as the kernel forms it: float32, left to right, x 0.25 x 16
    v = (((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + x[:, :, 1::2, 0::2]) + x[:, :, 1::2, 1::2]) * np.float32(0.25 * X_PRESCALE)
    assert v.dtype == np.float32 and np.abs(v).max() < 65504.0
    x1, x2 = _split(v.astype(np.float64))
    c1, c2 = OB.stem_im2col(x1), OB.stem_im2col(x2)
    acc = c1 @ (w1 + w2).T + c2 @ w1.T + shift_term[None, :]                            # w2 x1 + w1 x1 + w1 x2
    n = x.shape[0]
    return (acc / (ws * X_PRESCALE)).reshape(n, 56, 56, p).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("case", SC.CASES)
def test_emulated_split_stays_inside_half_the_band(case):
    st, x = SC.case_state(case), SC.case_images(case, N)
    pre, E = OB.stem_pre64_cond(x, st)
    tau = SC.tau(E)
    err = float((np.abs(emulate(x, st) - pre) / tau).max())
    share = float((np.abs(pre) < tau).mean())
    ones = float((pre >= 0).mean())
    print(f"{case}: err / tau {err:.3f}, share in band {share:.1e}, one-bits {ones:.3f}, max E / E0 {E.max() / SC.e0():.3g}")
    assert err <= 0.5
    assert share <= 1e-4
    assert 0.2 <= ones <= 0.8
