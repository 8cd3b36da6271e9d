"""The gate paths at real batch sizes: every image of every batch against the CPU bit oracle.

The code that decides which image a workgroup handles, in how many rounds and with which LDS table buffer only does
anything at batch sizes far above the 2, 3 or 8 images of the other oracle comparisons.  Here every geometry runs a
list of batch sizes derived from the launch arithmetic (tests/_gate_partition.py; tests/test_gate_batch_sizes_cpu.py
asserts on the CPU that the lists reach one, two and three rounds, a last round of one image, unequal slices, the
even-forcing rule and all three placement branches), on ONE plan reserved for the largest size, in an order that goes
up, down and up again; before each size the whole workspace is overwritten by a forward of N_max other images, so an
image that a kernel fails to write cannot read back the right answer of an earlier run.  The oracle (oracle/ttnet_bits.py on the GPU's own tables, which other tests pin to float64)
evaluates all N_max images once; a batch of n is the prefix bits[:n].  Nothing is sampled: every stage of every image
of every batch is compared.

The full variant (fan-in 30, gate_full.hip) has no tables: the oracle evaluates every block directly in float64
(OB.apply_direct), and the sweep runs twice, on the default path (split-fp16 / float32 with a float64 pass over the
listed outputs) and with TTNET_FULL_EXACT=1, at sizes that put every grid-stride loop of its kernels into a second sweep.
"""
import hashlib
import os
import time
from contextlib import contextmanager
from argparse import Namespace
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import _gate_partition as GP
from _util import scaled_tol
from oracle import ttnet_bits as OB
from scale_imagenet_amd import synth, ttnet
from scale_imagenet_amd.spec import VAlexSpec, make_spec

pytestmark = pytest.mark.gpu

CLASSES = {"small": ttnet.TT_vf_19lv3_imgnet_small, "xsmall": ttnet.TT_vf_19lv3_imgnet_xsmall,
           "valexnet": ttnet.TT_FHE_XSMALL_vAlexnet, "full": ttnet.TT_vf_19lv3_imgnet}
PATH_TWO_LAUNCH, PATH_FUSED, PATH_XSMALL, PATH_FULL, PATH_VALEXNET = range(5)      # "gate_path" of ttnet_plan_query
WORKERS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def sweep_bits(n, c, hw, seed, edges=()):
    """uint8 [n, c, hw, hw]: seeded, per-image density drawn from {0.5, 0.1, 0.9}.  The images at ``edges`` are
    constant ones: the first four are all zero, all one, checkerboard and inverse checkerboard; every further one
    holds one of those four patterns per channel, drawn per image, so that no two of them are alike.  All n images
    are distinct (asserted): an image written to another image's slot is seen."""
    rng = np.random.default_rng(seed)
    dens = rng.choice(np.array([0.5, 0.1, 0.9], dtype=np.float32), size=n)
    bits = np.empty((n, c, hw, hw), dtype=np.uint8)
    for i0 in range(0, n, 64):
        i1 = min(n, i0 + 64)
        bits[i0:i1] = rng.random((i1 - i0, c, hw, hw), dtype=np.float32) < dens[i0:i1, None, None, None]
    yy, xx = np.mgrid[0:hw, 0:hw]
    checker = ((yy + xx) & 1).astype(np.uint8)
    patterns = np.stack([np.zeros_like(checker), np.ones_like(checker), checker, 1 - checker])
    for k, i in enumerate(edges):
        bits[i] = patterns[k] if k < 4 else patterns[rng.integers(0, 4, size=c)]
    keys = {hashlib.blake2b(img.tobytes(), digest_size=16).digest() for img in bits}
    assert len(keys) == n, f"{n - len(keys)} of the {n} input images repeat another one"
    return bits


def build_model(variant, nfilter, tfilter, layers, dev, n_max):
    """A model with synthetic uncalibrated state (as the geometry tests of test_gpu_parity.py), its plan created."""
    if variant == "valexnet":
        spec = VAlexSpec()
        args = Namespace(nfilter=8, tfilter=8, layers=1, groups=[1, None, 4, None])
        st = synth.synth_state_dict(spec)
    else:
        spec = make_spec(variant, nfilter, tfilter, layers)
        args = Namespace(nfilter=nfilter, tfilter=tfilter, layers=layers, groups=[1, None, 4, None])
        st = synth.synth_state_dict(spec, calibrated=False)
    m = CLASSES[variant](args)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(n_max)
    hw = 10 if variant == "valexnet" else 56
    # (a random image of its own seed: no image of the sweep, so the warm-up leaves no right answer behind)
    rows = OB.pack_rows((np.random.default_rng(7).random((1, spec.p, hw, hw)) < 0.5).astype(np.uint8))
    with torch.no_grad():
        m.forward_from_stem_bits(torch.from_numpy(rows.view(np.int64)).to(dev))      # creates the plan, builds the tables
    torch.cuda.synchronize()
    assert m._any_plan().query("max_batch") == n_max
    return m, spec, st


def oracle_pass(bits, st, spec, luts):
    """The bit oracle over all images, in chunks of at most 64 on a thread pool (numpy releases the GIL in the
    gathers).  Returns ({stage: packed rows [N, C, H]}, float64 features [N, fcsize], float64 logits [N, classes])."""
    n = bits.shape[0]
    chunk = max(16, min(64, -(-n // WORKERS)))          # (chunks below ~16 images spend their time in Python, holding the GIL)
    spans = [(i0, min(n, i0 + chunk)) for i0 in range(0, n, chunk)]

    def run(span):
        b = bits[span[0]:span[1]]
        if spec.variant == "valexnet":
            y, logits = OB.valexnet_from_stem_bits(b, st, spec, luts)
            return {"features.5": OB.pack_rows(y)}, y.reshape(len(b), -1).astype(np.float64), logits
        taps = {}
        feat = OB.features_from_stem_bits(b, st, spec, luts, taps)       # forward_from_stem_bits without its head
        del taps["flatten"], taps[spec.blocks[-1].name]   # (the float output of the last block is compared as "flatten")
        return {k: OB.pack_rows(v) for k, v in taps.items()}, feat, None

    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        parts = list(ex.map(run, spans))
    stages = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    feat = np.concatenate([p[1] for p in parts])
    if spec.variant == "valexnet":
        return stages, feat, np.concatenate([p[2] for p in parts])
    # the float64 head once over all features: forward_from_stem_bits(bits) = head64(features_from_stem_bits(bits))
    return stages, feat, OB.head64(feat, st, f"features.{4 + len(spec.blocks) + 2}")


def first_bad(mask):
    bad = np.flatnonzero(mask)
    return int(bad[0]), len(bad)


@contextmanager
def env_set(monkeypatch, env):
    """Environment variables that gate_full.hip reads at every launch, set around one model's forwards."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def tie_report(image_bits, st, spec, stage):
    """For the failure text of a full-variant mismatch: how many outputs of the float64 oracle sit at |pre| < 1e-12 and
    below OB.NEAR_TIE in the Block_TTs of the stage's block, for that one image.  The GPU sums in another order than the
    oracle (a 1e-16 relative effect), so a differing bit at |pre| < 1e-12 is an exact tie turned by summation order; the
    assertion is not loosened for it, the text only says so."""
    blk = [b for b in spec.blocks if stage.startswith(b.name)][0]
    out, keep = [], OB.NEAR_TIE
    try:
        for bound in (1e-12, keep):
            OB.NEAR_TIE = bound                           # (apply_direct reads it when it fills ``near``)
            near = {}
            OB.features_from_stem_bits(image_bits[None], st, spec, None, None, near)
            out.append(", ".join(f"{k.rsplit('_', 1)[1]} {int(v.sum())}" for k, v in near.items() if k.startswith(blk.name)))
    finally:
        OB.NEAR_TIE = keep
    return (f" [float64 oracle, this image, outputs with |pre| < 1e-12: {out[0]}; with |pre| < {keep:g}: {out[1]}.  A bit that differs "
            f"only at |pre| < 1e-12 is an exact tie turned by summation order, not a kernel fault]")


def run_and_check(tag, m, spec, rows_dev, scrub_dev, n, stages, feat, exact, blocks, path, listed=None, ties=None):
    """One batch of n images on model m against the oracle.  Returns (stage rows, flatten, logits) of the GPU.

    The buffers of a plan are image-major from a fixed base and nothing clears them between forwards, so after a run
    of the same images every slot would already hold its right answer, and an image that a kernel fails to write would
    read back correct.  Before each size the whole workspace is therefore overwritten by a forward of N_max OTHER
    images (``scrub_dev``): what a kernel does not write at this n then holds another image's result.

    ``listed`` (full variant): receives the growth of the plan's running totals "full_listed_pw" / "full_listed_dw" across
    the forward of the n images alone (the scrub forward excluded), and the seconds that forward took.  ``ties``: called
    with (first differing image, stage) for a note in the failure text."""
    plan = m._any_plan()
    with torch.no_grad():
        m.forward_from_stem_bits(scrub_dev)
        if listed is not None:
            before = plan.query("full_listed_pw"), plan.query("full_listed_dw")       # (synchronises)
            t0 = time.time()
        y_dev = m.forward_from_stem_bits(rows_dev[:n])
    if listed is not None:
        listed["pw"], listed["dw"] = plan.query("full_listed_pw") - before[0], plan.query("full_listed_dw") - before[1]
        listed["seconds"] = time.time() - t0
    y = y_dev.cpu().numpy()
    if path in (PATH_FUSED, PATH_TWO_LAUNCH):             # the restated partition against the launchers' own arithmetic
        for i, b in enumerate(blocks):
            want = GP.fused_grid(n, b.C) if path == PATH_FUSED else GP.stage1_grid(n, b.C)
            assert plan.query(f"gate_grid:{i}") == want, f"{tag} n={n}: tests/_gate_partition.py drifted from the launcher of block {i}"
    got = {}
    for stage, want in stages.items():
        got[stage] = m.read_stage(stage, n)
        wrong = (got[stage] != want[:n]).reshape(n, -1).any(axis=1)
        if wrong.any():
            i, cnt = first_bad(wrong)
            where = ""
            if path == PATH_FUSED:
                bi = [k for k, b in enumerate(spec.blocks) if stage.startswith(b.name)][0]
                where = f" [fused block {bi}: {GP.fused_locate(i, n, blocks[bi].C, blocks[bi].HO)}]"
            if ties is not None:
                where = ties(i, stage)
            pytest.fail(f"{tag} n={n}: stage {stage} differs from the bit oracle in {cnt} of {n} images, first image {i}{where}")
    flat = m.read_stage("flatten", n)
    if spec.variant == "valexnet":
        wrong = (flat != feat[:n]).any(axis=1)
    else:
        # float32 table entries averaged in float32, read back from lin1's fp16 x 2 operand format (the bound of
        # test_random_bits_against_bit_oracle)
        wrong = (np.abs(flat - feat[:n]) > 5e-7 * max(1.0, np.abs(feat[:n]).max()) + 1e-6).any(axis=1)
    if wrong.any():
        i, cnt = first_bad(wrong)
        pytest.fail(f"{tag} n={n}: flatten outside its bound in {cnt} of {n} images, first image {i}, "
                    f"max |diff| {np.abs(flat - feat[:n]).max():.3e}")
    ref = exact[:n]
    tol = scaled_tol(ref)
    err = np.abs(y - ref).max(axis=1)
    print(f"{tag} n={n}: |logit| max {np.abs(ref).max():.2f}, |gpu - exact| max {err.max():.2e} (tolerance {tol:.2e})")
    if (err > tol).any():
        i, cnt = first_bad(err > tol)
        pytest.fail(f"{tag} n={n} (lin1 at M={n}): logits beyond {tol:.2e} in {cnt} images, first image {i}: {err[i]:.3e}; max {err.max():.3e}")
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > tol
    flipped = clear & (y.argmax(1) != ref.argmax(1))
    if flipped.any():
        i, cnt = first_bad(flipped)
        pytest.fail(f"{tag} n={n}: argmax differs from the exact head in {cnt} images with a clear top-2 gap, first image {i}")
    assert plan.query("range_overflow") == 0, f"{tag} n={n}: range flag raised"
    return got, flat, y_dev


def sweep(tag, dev, variant, nfilter, tfilter, layers, sizes, monkeypatch=None, both_paths=False, expect_path=None,
          full_modes=False):
    """Build the model(s) of a geometry on plans reserved for max(sizes), run the oracle once over all images, then
    every size in GP.run_order.  ``both_paths``: a two-launch plan (TTNET_GATE_UNFUSED=1, read at plan creation) and a
    fused plan of the same geometry; each is checked against the oracle and they are compared with each other.
    ``full_modes`` (full variant): a plan on the default path and one that runs under TTNET_FULL_EXACT=1, both created
    under TTNET_NO_GRAPH=1 (read once, at plan creation) so that no captured graph freezes what gate_full.hip reads from
    the environment at every launch; the stages of the two must be the same bytes, and the float64 list counters are
    bounded (default) or still (exact)."""
    t0 = time.time()
    n_max = max(sizes)
    models, envs = [], [{}, {}]
    if both_paths:
        monkeypatch.setenv("TTNET_GATE_UNFUSED", "1")
        models.append(("two-launch by switch", PATH_TWO_LAUNCH) + build_model(variant, nfilter, tfilter, layers, dev, n_max))
        monkeypatch.delenv("TTNET_GATE_UNFUSED")
        models.append(("fused", PATH_FUSED) + build_model(variant, nfilter, tfilter, layers, dev, n_max))
    elif full_modes:
        monkeypatch.setenv("TTNET_NO_GRAPH", "1")
        for name in ("TTNET_FULL_EXACT", "TTNET_FULL_TAU_SCALE"):
            monkeypatch.delenv(name, raising=False)
        envs = [{}, {"TTNET_FULL_EXACT": "1"}]
        for label, env in zip(("default", "TTNET_FULL_EXACT=1"), envs):
            with env_set(monkeypatch, env):
                models.append((label, PATH_FULL) + build_model(variant, nfilter, tfilter, layers, dev, n_max))
            assert models[-1][2]._any_plan().query("graphs_enabled") == 0, f"{tag}: {label}: the plan would capture graphs"
    else:
        assert os.environ.get("TTNET_GATE_UNFUSED") is None
        models.append((tag, expect_path) + build_model(variant, nfilter, tfilter, layers, dev, n_max))
    for label, path, m, _, _ in models:
        got_path = m._any_plan().query("gate_path")
        print(f"{tag}: {label}: gate_path {got_path}")
        assert got_path == path, f"{tag}: {label} runs on gate path {got_path}, expected {path}"
    _, _, m0, spec, st = models[0]
    blocks = [] if variant == "valexnet" else GP.blocks_of(spec)
    # (the full variant has no tables, get_table refuses: the oracle evaluates every block directly in float64)
    luts = None if variant == "full" else {b.name: m0.get_table(b.name) for b in spec.block_tts()}
    for _, _, m, _, _ in models[1:] if luts is not None else ():
        for b in spec.block_tts():
            assert np.array_equal(m.get_table(b.name), luts[b.name]), f"{tag}: the two plans built different tables for {b.name}"
    hw = 10 if variant == "valexnet" else 56
    if variant == "valexnet":
        edges = GP.flat_edge_images(GP.VA_KERNELS, sizes)
    elif variant == "full":
        edges = GP.full_edge_images(spec, sizes)
    elif variant == "xsmall":
        edges = GP.flat_edge_images(GP.xs_kernels(blocks), sizes)
    else:
        edges = set(GP.slice_edge_images(blocks, sizes)) if both_paths or not GP.fusable(blocks) else set()
        edges = sorted(edges | set(GP.edge_images(blocks, sizes) if GP.fusable(blocks) else ()))
    bits = sweep_bits(n_max, spec.p, hw, seed=1000 * spec.p + 10 * layers + len(variant), edges=edges)
    t1 = time.time()
    stages, feat, exact = oracle_pass(bits, st, spec, luts)
    t2 = time.time()
    rows_dev = torch.from_numpy(OB.pack_rows(bits).view(np.int64)).to(dev)
    # slot i of the scrub batch: the inverse of image i - 1, so no slot holds its own image or a constant one's twin
    scrub_dev = torch.from_numpy(OB.pack_rows(np.roll(1 - bits, 1, axis=0)).view(np.int64)).to(dev)
    order = GP.run_order(sizes)
    seen, gpu_s = {}, 0.0                                  # full_modes: (mode, n) -> (list growth, logits) of the first run of n
    for n in order:
        res = []
        for k, (label, path, m, _, _) in enumerate(models):
            if not full_modes:
                res.append(run_and_check(f"{tag} [{label}]", m, spec, rows_dev, scrub_dev, n, stages, feat, exact, blocks, path))
                continue
            listed = {}
            with env_set(monkeypatch, envs[k]):
                res.append(run_and_check(f"{tag} [{label}]", m, spec, rows_dev, scrub_dev, n, stages, feat, exact, blocks, path,
                                         listed=listed, ties=lambda i, stage: tie_report(bits[i], st, spec, stage)))
            gpu_s += listed.pop("seconds")
            pairs, outputs = n * GP.full_pw_pairs(spec), n * GP.full_dw_outputs(spec)
            print(f"{tag} [{label}] n={n}: {listed['pw']} of {pairs} (pixel, group) pairs and {listed['dw']} of {outputs} depthwise outputs listed")
            if envs[k]:
                assert listed == {"pw": 0, "dw": 0}, f"{tag} [{label}] n={n}: the float64 path listed {listed}"
            else:
                assert 0 < listed["pw"] < pairs / 8 and 0 <= listed["dw"] < outputs / 100, (tag, n, listed, pairs, outputs)
            first = seen.setdefault((k, n), (listed, res[-1][2]))
            assert first[0] == listed, f"{tag} [{label}] n={n}: listed {listed} now, {first[0]} the first time"
            assert torch.equal(first[1], res[-1][2]), f"{tag} [{label}] n={n}: logits differ between two runs of the same batch"
        if full_modes:
            for stage in res[0][0]:
                assert np.array_equal(res[0][0][stage], res[1][0][stage]), f"{tag} n={n}: {stage} differs between the default and the float64 path"
        if both_paths:
            (s_u, f_u, y_u), (s_f, f_f, y_f) = res
            for stage in s_u:
                assert np.array_equal(s_u[stage], s_f[stage]), f"{tag} n={n}: {stage} differs between the two-launch and the fused plan"
            assert np.array_equal(f_u, f_f), f"{tag} n={n}: flatten differs between the two-launch and the fused plan"
            assert torch.equal(y_u, y_f), f"{tag} n={n}: logits differ between the two-launch and the fused plan"
    print(f"{tag}: sizes {order}: {sum(order) * len(models)} images compared with the oracle over {len(stages)} stages, flatten and "
          f"logits; oracle pass over {n_max} images {t2 - t1:.1f} s on {WORKERS} threads, whole sweep {time.time() - t0:.1f} s"
          + (f", of which {gpu_s:.1f} s in the forwards of the compared batches" if full_modes else ""))
    if full_modes:
        assert order.count(n_max) == 2 and all((k, n_max) in seen for k in range(2))


def small_sizes(nfilter, tfilter, layers, both=False):
    blocks = GP.blocks_of(make_spec("small", nfilter, tfilter, layers))
    if GP.fusable(blocks) and not both:
        return GP.fused_sizes(blocks)
    return GP.two_launch_sizes(blocks, fused_too=both)


FUSED_ONLY, BOTH_PATHS, TWO_LAUNCH_BY_GEOMETRY, XSMALL = GP.FUSED_ONLY, GP.BOTH_PATHS, GP.TWO_LAUNCH_BY_GEOMETRY, GP.XSMALL


@pytest.mark.parametrize("nfilter,tfilter,layers", FUSED_ONLY)
def test_small_fused_batches(dev, nfilter, tfilter, layers):
    """TT-small on the fused path at p = 16, 48, 96, 128: plain placement with even and odd strand counts, the
    8-pair placement (p = 128) and, in the later blocks of p = 16, the 4-pair one; p = 16 needs 2049 images to put
    three rounds into a workgroup of its first block."""
    sweep(f"small p={nfilter * tfilter} --layers {layers}", dev, "small", nfilter, tfilter, layers,
          small_sizes(nfilter, tfilter, layers), expect_path=PATH_FUSED)


@pytest.mark.parametrize("nfilter,tfilter,layers", BOTH_PATHS)
def test_small_fused_and_two_launch_by_switch(dev, monkeypatch, nfilter, tfilter, layers):
    """p = 64 at --layers 0, 1, 2 and p = 32: the fused plan and the plan that TTNET_GATE_UNFUSED=1 keeps on the two
    launches of gate.hip (gate_path 1 and 0), each against the oracle and against each other, bit for bit."""
    sweep(f"small p={nfilter * tfilter} --layers {layers}", dev, "small", nfilter, tfilter, layers,
          small_sizes(nfilter, tfilter, layers, both=True), monkeypatch=monkeypatch, both_paths=True)


@pytest.mark.parametrize("nfilter,tfilter,layers", TWO_LAUNCH_BY_GEOMETRY)
def test_small_two_launch_by_geometry(dev, nfilter, tfilter, layers):
    """--layers 3 / 4: a stride-1 block keeps the whole net on the two-launch kernels."""
    sweep(f"small p={nfilter * tfilter} --layers {layers}", dev, "small", nfilter, tfilter, layers,
          small_sizes(nfilter, tfilter, layers), expect_path=PATH_TWO_LAUNCH)


@pytest.mark.parametrize("nfilter,tfilter,layers", XSMALL)
def test_xsmall_batches(dev, nfilter, tfilter, layers):
    """The flat-grid kernels of gate_xs.hip."""
    sizes = GP.flat_sizes(GP.xs_kernels(GP.blocks_of(make_spec("xsmall", nfilter, tfilter, layers))))
    sweep(f"xsmall p={nfilter * tfilter} --layers {layers}", dev, "xsmall", nfilter, tfilter, layers, sizes, expect_path=PATH_XSMALL)


def test_valexnet_batches(dev):
    """gate_va.hip through forward_from_stem_bits with rows [n][64][10], against OB.valexnet_from_stem_bits."""
    sweep("valexnet", dev, "valexnet", 8, 8, 1, GP.flat_sizes(GP.VA_KERNELS), expect_path=PATH_VALEXNET)


def test_full_batches(dev, monkeypatch):
    """gate_full.hip (fan-in 30, p = 60 --layers 1): the sizes of GP.full_sizes put every grid-stride loop of full_dw_* and
    full_pw_* on both sides of its second sweep.  Default path and TTNET_FULL_EXACT=1, each against the float64 oracle
    (OB.apply_direct, no tables) and against each other; the list counters of the default path stay a small share."""
    nfilter, tfilter, layers = GP.FULL[0]
    sweep(f"full p={nfilter * tfilter} --layers {layers}", dev, "full", nfilter, tfilter, layers,
          GP.full_sizes(make_spec("full", nfilter, tfilter, layers)), monkeypatch=monkeypatch, expect_path=PATH_FULL, full_modes=True)
