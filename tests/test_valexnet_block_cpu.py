"""CPU: the block geometry shared by the twins of the certificate and of the witness search
(scale_imagenet_amd/valexnet_block.py) against the bit oracle ``OB.valexnet_from_stem_bits``: which features a stem bit
reaches, the window inputs as the inverse of that, and the block on fully known planes."""
import numpy as np

import _attack_util as U
from oracle import ttnet_bits as OB
from scale_imagenet_amd import certify as CF
from scale_imagenet_amd import valexnet_block as VB

# the four corners, one bit on each edge, one interior bit; the ends of the first conv3 group, the start of the second, the last
POSITIONS = [(0, 0), (0, 9), (9, 0), (9, 9), (0, 5), (9, 5), (5, 0), (5, 9), (5, 5)]
CHANNELS = (0, 7, 8, 63)


def test_reached_equals_the_features_a_flip_changes_under_parity_tables():
    """With tables that are the parity of their inputs a feature changes exactly when the flipped bit is in its window."""
    spec, st, luts = U.setup()
    parity = {}
    for name, t in luts.items():
        par = np.array([bin(i).count("1") & 1 for i in range(t.shape[1])], dtype=t.dtype)
        parity[name] = np.ascontiguousarray(np.broadcast_to(par[None, :, None], t.shape))
    bits = np.random.default_rng(11).integers(0, 2, size=(1, 64, 10, 10)).astype(np.uint8)
    flips = [(ch, y, x) for ch in CHANNELS for y, x in POSITIONS]
    flipped = np.repeat(bits, len(flips), axis=0)
    for q, (ch, y, x) in enumerate(flips):
        flipped[q, ch, y, x] ^= 1
    y0, _ = OB.valexnet_from_stem_bits(bits, st, spec, parity)
    y1, _ = OB.valexnet_from_stem_bits(flipped, st, spec, parity)
    valid, fc, oy, ox, _ = VB.reached()
    counts = {}
    for q, (ch, y, x) in enumerate(flips):
        want = set(np.flatnonzero(y1[q].reshape(-1) != y0[0].reshape(-1)).tolist())
        v = valid[:, ch, y, x] != 0
        mine = ((fc[:, ch, y, x] * 11 + oy[:, ch, y, x]) * 11 + ox[:, ch, y, x])[v].tolist()
        assert len(set(mine)) == len(mine) and set(mine) == want, (ch, y, x, sorted(set(mine) ^ want))
        counts[(ch, y, x)] = len(want)
    print("features reached per position:", {p: counts[(0,) + p] for p in POSITIONS})
    for (ch, y, x), k in counts.items():
        assert k == counts[(0, y, x)]                                    # the channel changes which features, not how many
        assert (k == VB.N_REACH) == (y not in (0, 9) and x not in (0, 9)) and k <= VB.N_REACH


def test_window_inputs_are_the_inverse_of_reach():
    valid, fc, oy, ox, p = VB.reached()
    seen = 0
    for t, ch, y, x in np.argwhere(valid != 0):
        f = int(fc[t, ch, y, x])
        kind = f // 64
        assert kind == (0 if t < 6 else 1 if t < 12 else 2 if t < 20 else 3) and 0 <= p[t, ch, y, x] < VB.WINDOW_SIZE[kind]
        assert 0 <= oy[t, ch, y, x] < 11 and 0 <= ox[t, ch, y, x] < 11
        got = VB.window_input(kind, f % 64, int(oy[t, ch, y, x]), int(ox[t, ch, y, x]), int(p[t, ch, y, x]))
        want_ch = 8 * (ch // 8) + int(p[t, ch, y, x]) if kind == 2 else ch
        assert got == (want_ch, y, x) and want_ch == ch, (t, ch, y, x, got)
        seen += 1
    assert seen == int((valid != 0).sum()) and seen > 20 * 64 * 64
    assert VB.window_input(0, 3, 0, 0, 0) is None and VB.window_input(1, 3, 10, 9, 5) is None      # paddings
    assert VB.window_input(0, 3, 9, 10, 3) is None and VB.window_input(0, 3, 9, 10, 2) == (3, 9, 9)


def test_block_planes_with_known_bits_equal_the_oracle():
    spec, st, luts = U.setup()
    rng = np.random.default_rng(12)
    tables = {name: rng.integers(0, 2, size=t.shape).astype(t.dtype) for name, t in luts.items()}
    bits = rng.integers(0, 2, size=(2, 64, 10, 10)).astype(np.uint8)
    want, _ = OB.valexnet_from_stem_bits(bits, st, spec, tables)
    ylo, yhi = CF.block_planes_cpu(tables, bits, bits)
    assert ylo.shape == (2, 256, 11, 11) and np.array_equal(ylo, want) and np.array_equal(yhi, want)
