"""The definition of the care-set misses on the bit oracle (test infrastructure; imports oracle/), shared by the care
tests: the canonical index of every lookup of every ``Block_TT``, from the device's own ``features.3`` stage on the
device's own tables, as ``expected_usage`` of tests/test_gpu_table_usage.py forms them."""
import numpy as np

from oracle import ttnet_bits as OB
from scale_imagenet_amd import minimise


def lookup_indices(stem_rows, spec, luts):
    """``{Block_TT name: uint32 [N, G, Ho, Wo]}`` canonical indices, from row-packed stem bits [N, p, 56]."""
    x = OB.unpack_rows(stem_rows, 56)
    out = {}
    for blk in spec.blocks:
        taps = {}
        y = OB.multihead_block_bits(x, luts, blk, spec.variant, taps)
        for b in (blk.conv1, blk.conv2, blk.conv3):
            out[b.name] = OB.window_index(x, b)
        outs = [taps[f"{blk.name}.out{k}"] for k in (1, 2, 3, 4)]
        n_, c, hh, ww = outs[0].shape
        outf = np.stack(outs, axis=2).reshape(n_, 4 * c, hh, ww)     # channel 4c + branch, after the branch padding
        out[blk.convf.name] = OB.window_index(outf, blk.convf)
        x = y
    return out


def expected_rows(indices, spec, masks):
    """int32 [N, B]: per image and ``Block_TT`` (the order of ``spec.block_tts()``), the lookups whose care bit is 0; a
    block without a bitmap in ``masks`` gives 0."""
    blocks = spec.block_tts()
    n = next(iter(indices.values())).shape[0]
    rows = np.zeros((n, len(blocks)), dtype=np.int32)
    for col, b in enumerate(blocks):
        if b.name not in masks:
            continue
        keep = minimise.unpack_bits(masks[b.name], b.fan_in_bits)    # bool [G, 2^n]
        idx = indices[b.name]
        g = np.arange(b.groups).reshape(1, -1, 1, 1)
        rows[:, col] = (~keep[g, idx]).reshape(n, -1).sum(axis=1)
    return rows


def usage_of(indices, spec):
    """int64 usage counts ``{name: [G, 2^n]}`` of the same lookups."""
    out = {}
    for b in spec.block_tts():
        idx = indices[b.name]
        out[b.name] = np.stack([np.bincount(idx[:, g].ravel(), minlength=1 << b.fan_in_bits)
                                for g in range(b.groups)]).astype(np.int64)
    return out
