"""The float64 fall-back of the full variant (gate_full.hip), forced: every stage against the CPU bit oracle.

By default the split-fp16 / float32 pass of the full variant lists about 1 in 1000 (pixel, group) pairs and 1 in 10^5
depthwise outputs for the float64 pass, so the float64 pass over the list is almost idle in every other test, and the
branch of full_dw_fix_kernel that recomputes everything after an overflow of the list never runs.  TTNET_FULL_TAU_SCALE
(read at every launch) multiplies the error bound that decides what is listed: 1e30 lists every output.  On one plan
reserved for 40 images (tests/_gate_partition.py FULL_FALLBACK; tests/test_gate_batch_sizes_cpu.py asserts on the CPU
which branch each n takes) this file runs

  * n = 5, everything listed: the depthwise lists hold every output (``all == false`` with a full list), the float64 pass
    of every 1x1 block walks its list in several sweeps, every bit of every row word is patched with atomics;
  * n = 6: the depthwise list of features.4 overflows (recompute all), those of features.5 and .6 do not;
  * n = 40: every depthwise block overflows; the 1x1 main kernels of features.4 take two sweeps;
  * n = 40 with an intermediate scale: fast bits and patched bits share row words;
  * n = 6 and n = 5 in flight on two lanes, each with its own list area;
  * and afterwards the default path again, which must not see anything left in the list area.

Each forward follows a scrub forward of the 40 inverted images, and is compared bit for bit with the float64 oracle
(oracle/ttnet_bits.py, apply_direct; one pass over the 40 images, shared) and with the TTNET_FULL_EXACT=1 run of the same n;
flatten and the logits are held to the bounds of tests/test_gpu_gate_batches.py.  With everything listed the growth of the
plan's counters is exact: n * full_pw_pairs and n * full_dw_outputs (the depthwise counter counts past the cap), which
pins the masking of the idle lanes of a row bundle in the list code.

The intermediate scales, measured on an MI355X on these 40 images (TTNET_FULL_TAU_SCALE: listed share of the 900,320
(pixel, group) pairs, of the 7,896,000 depthwise outputs):
    1 (default)  0.0118   0.0001
    1e1          0.1304   0.0009
    1e2          0.6845   0.0141
    3e2          0.9556   0.0448
    1e3          0.9999   0.1488
    3e3          1.0000   0.3712
    1e4          1.0000   0.7289
    1e5, 1e30    1.0000   1.0000
The bound of the depthwise blocks is some 300 times tighter against their pre-activations than that of the 1x1 blocks, so no
single scale lists a middling share of both, and of 1e2, 1e3 and 1e4 none puts the share of pairs into [0.05, 0.6] (1e2 is
just above it).  The test therefore takes one scale per kind, in two forwards: 1e1 for the 1x1 blocks (0.1304 of the pairs)
and 1e3, the first of the three that serves, for the depthwise blocks (0.1488 of the outputs; nearly every pair is listed
beside them).
"""
import numpy as np
import pytest
import torch

import _gate_partition as GP
import test_gpu_gate_batches as GB
from oracle import ttnet_bits as OB
from scale_imagenet_amd import synth

pytestmark = pytest.mark.gpu

MAX_BATCH, N_LISTS_ALL, N_MIXED, N_OVERFLOW = GP.FULL_FALLBACK
EVERYTHING = "1e30"
PARTLY_SCALE = {"pw": "1e1", "dw": "1e3"}            # one scale per counter: see the table above
ENV = ("TTNET_FULL_EXACT", "TTNET_FULL_TAU_SCALE")


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    c = Ctx()
    c.dev = torch.device("cuda", 0)
    nfilter, tfilter, layers = GP.FULL[0]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("TTNET_NO_GRAPH", "1")             # read once, at plan creation: no graph may freeze a value of ENV
        for name in ENV:
            mp.delenv(name, raising=False)
        c.m, c.spec, c.st = GB.build_model("full", nfilter, tfilter, layers, c.dev, MAX_BATCH)
    assert c.m._any_plan().query("graphs_enabled") == 0 and c.m._any_plan().query("gate_path") == GB.PATH_FULL
    c.bits = GB.sweep_bits(MAX_BATCH, c.spec.p, 56, seed=6040, edges=(0, N_LISTS_ALL - 1, N_MIXED - 1, MAX_BATCH - 1))
    c.stages, c.feat, c.exact = GB.oracle_pass(c.bits, c.st, c.spec, None)
    c.rows_dev = torch.from_numpy(OB.pack_rows(c.bits).view(np.int64)).to(c.dev)
    c.scrub_dev = torch.from_numpy(OB.pack_rows(np.roll(1 - c.bits, 1, axis=0)).view(np.int64)).to(c.dev)
    c.pairs, c.outputs = GP.full_pw_pairs(c.spec), GP.full_dw_outputs(c.spec)
    c.runs = {}
    return c


def run(c, monkeypatch, n, scale=None, exact=False, fresh=False):
    """A scrub forward, then the forward of images [:n] under the given switches, checked against the oracle (every stage
    bit for bit, flatten, logits, argmax, range flag: GB.run_and_check).  Returns (list growth, stages, flatten, logits);
    the first result of each (n, scale, exact) is kept for the comparisons between runs and returned again unless ``fresh``."""
    key = (n, scale, exact)
    if fresh or key not in c.runs:
        for name in ENV:
            monkeypatch.delenv(name, raising=False)
        if exact:
            monkeypatch.setenv("TTNET_FULL_EXACT", "1")
        if scale is not None:
            monkeypatch.setenv("TTNET_FULL_TAU_SCALE", scale)
        listed = {}
        tag = f"full n={n} " + ("TTNET_FULL_EXACT=1" if exact else f"TTNET_FULL_TAU_SCALE={scale}")
        got, flat, y = GB.run_and_check(tag, c.m, c.spec, c.rows_dev, c.scrub_dev, n, c.stages, c.feat, c.exact, GP.blocks_of(c.spec),
                                        GB.PATH_FULL, listed=listed, ties=lambda i, stage: GB.tie_report(c.bits[i], c.st, c.spec, stage))
        print(f"{tag}: {listed['pw']} of {n * c.pairs} (pixel, group) pairs, {listed['dw']} of {n * c.outputs} depthwise outputs listed; "
              f"forward {listed.pop('seconds') * 1e3:.1f} ms")
        for name in ENV:
            monkeypatch.delenv(name, raising=False)
        if fresh:
            return listed, got, flat, y
        c.runs[key] = (listed, got, flat, y)
    return c.runs[key]


def same_bits_as_exact(c, monkeypatch, n, got):
    listed, want, _, _ = run(c, monkeypatch, n, exact=True)
    assert listed == {"pw": 0, "dw": 0}, f"TTNET_FULL_EXACT=1 listed {listed}"
    for stage in want:
        assert np.array_equal(got[stage], want[stage]), f"n={n}: {stage} differs from the TTNET_FULL_EXACT=1 run"


@pytest.mark.parametrize("n", [N_LISTS_ALL, N_MIXED, N_OVERFLOW], ids=["list_holds_everything", "features4_overflows", "every_block_overflows"])
def test_everything_listed(ctx, monkeypatch, n):
    """TTNET_FULL_TAU_SCALE=1e30: every emitted bit comes from the float64 pass, through the list (n = 5), through the
    recompute-all branch in features.4 only (n = 6) or in every block (n = 40)."""
    listed, got, _, _ = run(ctx, monkeypatch, n, scale=EVERYTHING)
    same_bits_as_exact(ctx, monkeypatch, n, got)
    # every (pixel, group) pair and every depthwise output exactly once: no idle lane of a row bundle, nothing twice
    assert listed == {"pw": n * ctx.pairs, "dw": n * ctx.outputs}, (n, listed, n * ctx.pairs, n * ctx.outputs)


def test_partly_listed(ctx, monkeypatch):
    """Intermediate scales at n = 40, one per kind of block: the float64 pass patches some bits of a row word whose other
    bits the fast pass wrote.  The share of the kind a scale is chosen for must stay strictly inside (0.02, 0.9), so that
    this cannot turn into nothing or everything listed."""
    n = N_OVERFLOW
    for kind, total in (("pw", n * ctx.pairs), ("dw", n * ctx.outputs)):
        listed, got, _, _ = run(ctx, monkeypatch, n, scale=PARTLY_SCALE[kind])
        same_bits_as_exact(ctx, monkeypatch, n, got)
        share = listed[kind] / total
        print(f"TTNET_FULL_TAU_SCALE={PARTLY_SCALE[kind]}: share of {kind} listed {share:.4f}")
        assert 0.02 < share < 0.9, (kind, PARTLY_SCALE[kind], listed, total)


def test_two_lanes_in_flight(ctx, monkeypatch):
    """Everything listed, n = 6 on lane 0 and n = 5 on lane 1, issued on two streams before any synchronisation: each lane
    has its own list area, and both must give the bytes of their single-lane runs."""
    c = ctx
    _, want6, flat6, y6 = run(c, monkeypatch, N_MIXED, scale=EVERYTHING)
    _, want5, flat5, y5 = run(c, monkeypatch, N_LISTS_ALL, scale=EVERYTHING)
    monkeypatch.setenv("TTNET_FULL_TAU_SCALE", EVERYTHING)
    c.m.set_lanes(2)
    assert c.m._any_plan().query("lanes") == 2
    x1 = torch.from_numpy(synth.synth_images(1)).to(c.dev)
    streams = [torch.cuda.Stream(c.dev), torch.cuda.Stream(c.dev)]
    jobs = {0: (N_MIXED, want6, flat6, y6), 1: (N_LISTS_ALL, want5, flat5, y5)}
    torch.cuda.synchronize()
    # forward_from_stem_bits runs on the lane of the latest forward, so a one-image forward picks the lane; read_stage
    # reads the lane used last: two rounds, each lane last once
    for lanes in ((0, 1), (1, 0)):
        y = {}
        with torch.no_grad():
            for lane in lanes:
                with torch.cuda.stream(streams[lane]):
                    c.m(x1, lane=lane)
                    c.m.forward_from_stem_bits(c.scrub_dev)
                    y[lane] = c.m.forward_from_stem_bits(c.rows_dev[:jobs[lane][0]])
        torch.cuda.synchronize()
        last = lanes[-1]
        n, want, flat, _ = jobs[last]
        for stage in want:
            assert np.array_equal(c.m.read_stage(stage, n), want[stage]), f"lane {last} (n={n}) with lane {lanes[0]} in flight: {stage}"
        assert np.array_equal(c.m.read_stage("flatten", n), flat), f"lane {last}: flatten"
        for lane in lanes:
            assert torch.equal(y[lane], jobs[lane][3]), f"lane {lane} (n={jobs[lane][0]}): logits differ from the single-lane run"
    assert c.m._any_plan().query("range_overflow") == 0


def test_default_path_afterwards(ctx, monkeypatch):
    """After forwards that filled the list area to the brim: the default path on the 40 images still equals the oracle and
    lists a small share again (nothing sticky is left behind)."""
    n = N_OVERFLOW
    full, _, _, _ = run(ctx, monkeypatch, n, scale=EVERYTHING, fresh=True)
    assert full == {"pw": n * ctx.pairs, "dw": n * ctx.outputs}
    listed, got, _, _ = run(ctx, monkeypatch, n, fresh=True)
    same_bits_as_exact(ctx, monkeypatch, n, got)
    assert 0 < listed["pw"] < n * ctx.pairs / 8 and 0 <= listed["dw"] < n * ctx.outputs / 100, listed
