"""gate_block_kernel at the smallest shapes that reach every code path, against the CPU bit oracle.

tests/test_gpu_gate_batches.py walks the batch partition at real batch sizes; this file is the quick companion for
changes INSIDE the phases of the kernel (index forming, table layout, transposes, border handling): the block outputs
read back through ttnet_read_stage are compared bit for bit with oracle/ttnet_bits.py on the GPU's own tables, at

  batches  1, and R - 1, R, R + 1 for the round sizes R = 8 / 16 / 32 of the three geometries (a full round, a round one
           image short, one image over: rounds with idle task slots, slices with and without images);
  widths   p = 16 (one strand pair, plain placement) and p = 64 (the 4-pair placement);
  depths   --layers 0 and --layers 2, which together run 56 -> 29, 29 -> 15, 15 -> 8 and 8 -> 5, each last-block
           variant included;
  taps     one case also reads out1 .. out4 of every block, which reruns the non-last blocks with the tap buffer
           attached (the last block's branch dwords are its output anyway);
  inputs   seeded random bits of three densities, with an all-zero, an all-one and two checkerboard images among
           them, so that the zero border and both majorities see both constants.

No tolerance: every compared stage is equal or the test fails.  ("flatten" is float: the bound is that of
test_gpu_parity.py::test_random_bits_against_bit_oracle.)
"""
import numpy as np
import pytest
import torch

import _gate_partition as GP
import test_gpu_gate_batches as GB
from oracle import ttnet_bits as OB
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

ROUNDS = (8, 16, 32)                                                       # fused_round<HO>() for HO = 29, 15, 8 (and 5)
SIZES = sorted({1} | {r + d for r in ROUNDS for d in (-1, 0, 1)})
N_MAX = max(SIZES)
CONSTANT_IMAGES = (1, 2, 3, 4)                                              # all zero, all one, checkerboard, inverse (image 0 stays random)

# (nfilter, tfilter, --layers, read the branch taps)
CASES = [(2, 8, 0, False), (2, 8, 2, False), (8, 8, 0, False), (8, 8, 2, False), (8, 8, 2, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def test_round_sizes_are_the_kernels():
    assert [GP.fused_round(ho) for ho in (29, 15, 8)] == list(ROUNDS)
    geoms = set()
    for layers in (0, 2):
        blocks = GP.blocks_of(make_spec("small", 8, 8, layers))
        assert GP.fusable(blocks)
        geoms |= {(b.H, b.HO) for b in blocks}
    assert geoms == {(56, 29), (29, 15), (15, 8), (8, 5)}


@pytest.mark.parametrize("nfilter,tfilter,layers,taps", CASES)
def test_block_outputs_against_bit_oracle(dev, nfilter, tfilter, layers, taps):
    tag = f"small p={nfilter * tfilter} --layers {layers}{' +taps' if taps else ''}"
    m, spec, st = GB.build_model("small", nfilter, tfilter, layers, dev, N_MAX)
    assert m._any_plan().query("gate_path") == GB.PATH_FUSED, tag
    luts = {b.name: m.get_table(b.name) for b in spec.block_tts()}
    bits = GB.sweep_bits(N_MAX, spec.p, 56, seed=77 + 1000 * spec.p + layers, edges=CONSTANT_IMAGES)
    stages, feat, _ = GB.oracle_pass(bits, st, spec, luts)
    if not taps:
        stages = {k: v for k, v in stages.items() if ".out" not in k}
    else:
        assert sum(".out" in k for k in stages) >= 4 * (len(spec.blocks) - 1), sorted(stages)
    rows_dev = torch.from_numpy(OB.pack_rows(bits).view(np.int64)).to(dev)
    # before each size the workspace is overwritten with other images' results (see run_and_check of the batch sweep)
    scrub_dev = torch.from_numpy(OB.pack_rows(np.roll(1 - bits, 1, axis=0)).view(np.int64)).to(dev)
    for n in SIZES:
        with torch.no_grad():
            m.forward_from_stem_bits(scrub_dev)
            m.forward_from_stem_bits(rows_dev[:n])
        for stage, want in stages.items():
            got = m.read_stage(stage, n)
            wrong = (got != want[:n]).reshape(n, -1).any(axis=1)
            assert not wrong.any(), f"{tag} n={n}: stage {stage} differs from the bit oracle in {int(wrong.sum())} of {n} images, first image {int(np.flatnonzero(wrong)[0])}"
        flat = m.read_stage("flatten", n)
        bound = 5e-7 * max(1.0, np.abs(feat[:n]).max()) + 1e-6
        assert np.abs(flat - feat[:n]).max() <= bound, f"{tag} n={n}: flatten off by {np.abs(flat - feat[:n]).max():.3e} (bound {bound:.1e})"
    print(f"{tag}: sizes {SIZES}, {len(stages)} stages + flatten equal to the oracle")
