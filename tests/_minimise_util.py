"""Helpers shared by the minimiser's rounds tests (copies of the small ones in test_gpu_minimise.py / test_minimise_cpu.py)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from scale_imagenet_amd import minimise as M

SENTINEL = 0x5EA7BEEF
DENSITIES = ((0.5, 0.0), (0.3, 0.4), (0.05, 0.9), (0.9, 0.05), (0.02, 0.0))      # test_gpu_minimise.random_functions

# (n, don't-care share, rng seed) of the four literal-count sets, 30 functions each
SETS = ((6, 0.0, 60), (6, 0.4, 64), (8, 0.0, 80), (8, 0.4, 84))


def random_functions(seed, n, count, densities=DENSITIES):
    rng = np.random.default_rng(seed)
    on, dc = [], []
    for i in range(count):
        p_on, p_dc = densities[i % len(densities)]
        r = rng.random(1 << n)
        on.append(M.pack_bits(r < p_on))
        dc.append(M.pack_bits((r >= p_on) & (r < p_on + p_dc)))
    return np.stack(on), np.stack(dc)


def literal_set(n, dcf, seed, count=30):
    """``(on, dc)`` bitmaps ``[count, words]``: f = half the patterns, d = a share ``dcf`` of them, ON = f & ~d, DC = d."""
    rng = np.random.default_rng(seed)
    on, dc = [], []
    for _ in range(count):
        f = rng.random(2 ** n) < 0.5
        d = rng.random(2 ** n) < dcf
        on.append(M.pack_bits(f & ~d))
        dc.append(M.pack_bits(d))
    return np.stack(on), np.stack(dc)


def twin(on, dc, n, rounds=0, workers=8):
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda i: M.minimise_cpu(on[i], None if dc is None else dc[i], n, rounds), range(len(on))))


def assert_same(got, want, tag):
    assert len(got) == len(want), tag
    for f, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), f"{tag} function {f}: {len(a)} cubes on the device, {len(b)} from the twin"
        if not np.array_equal(a, b):
            d = np.flatnonzero(a != b)
            raise AssertionError(f"{tag} function {f}: {len(d)} of {len(a)} keys differ, first at {d[0]}: device {int(a[d[0]]):#x}, "
                                 f"twin {int(b[d[0]]):#x}")


def size(cubes):
    """(literals, cubes): what step 9 compares."""
    return M.literal_total(cubes), len(cubes)


def evaluate_text(text, n):
    """An expression in the printed style on all 2^n patterns (x_j = index bit n-1-j)."""
    idx = np.arange(1 << n)
    env = {f"x_{j}": ((idx >> (n - 1 - j)) & 1).astype(bool) for j in range(n)}
    return np.broadcast_to(eval(text, {"__builtins__": {}}, {**env, "True": True, "False": False}), idx.shape)
