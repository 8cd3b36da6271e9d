"""GPU: ttnet_cover_support (csrc/rules.hip) against its numpy twin, ``rules.cover_support_cpu``: every comparison is
``np.array_equal`` on integers.  The raw calls go through ctypes with a cube cap larger than every count, 0xFFFFFFFF keys
past ``counts[f]``, output buffers pre-filled with a sentinel and slack behind them that must come back untouched.

The covers come from the minimiser's CPU twin (small n), from constructions (parity: all minterms; constants) and, at
n = 16, from ``minimise_device``, which tests of its own compare with its twin.  The sizes are the smallest that reach every
path: one-word bitmaps (n < 5), the word edge (n = 5), more patterns than a pass of the workgroup (n >= 11), covers of
more cubes than a staged chunk (1,024), more functions than workgroups (1,024)."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from _minimise_util import random_functions
from scale_imagenet_amd import _lib, minimise as M, rules as R, synth, ttnet
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEEF5EA7BEEF
POISON = 0xFFFFFFFF
SLACK = 64
CHUNK = 1024                                         # kSupChunk of csrc/rules.hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Buffers:
    """Device buffers of one raw call: cubes ``[F, cap]`` poisoned past the counts, outputs filled with a sentinel, each
    with ``SLACK`` elements behind it."""

    def __init__(self, dev, covers, usage, rows, n, keep=None, cap=None, lost=True):
        self.n, self.total = n, len(covers)
        self.counts = np.array([len(c) for c in covers], dtype=np.int32)
        self.cap = cap = int(cap if cap is not None else max(int(self.counts.max()), 1) + 5)
        packed = np.full((self.total, cap), POISON, dtype=np.uint32)
        flags = np.ones((self.total, cap), dtype=np.uint8)               # (a set flag on a poisoned key must not matter)
        for f, keys in enumerate(covers):
            packed[f, : len(keys)] = keys
            if keep is not None:
                flags[f, : len(keys)] = np.asarray(keep[f]) != 0
        self.cubes = to_dev(packed.view(np.int32), dev)
        self.counts_t = to_dev(self.counts, dev)
        self.keep = to_dev(flags, dev) if keep is not None else None
        self.usage = to_dev(np.asarray(usage, dtype=np.int64), dev)
        self.rows = to_dev(np.asarray(rows, dtype=np.int32), dev)
        self.words = M.n_words(n)
        fill = lambda count, dtype: torch.full((count + SLACK,), SENTINEL if dtype == torch.int64 else 0x5EA7BEEF,
                                               dtype=dtype, device=dev)
        self.out = [fill(self.total * cap, torch.int64) for _ in range(3)]
        self.totals = fill(self.total * 4, torch.int64)
        self.lost = fill(self.total * self.words, torch.int32) if lost else None
        self.work = torch.empty(_lib.check(_lib.load().ttnet_cover_support_workspace(n, self.total)), dtype=torch.uint8, device=dev)

    def call(self, dev, **over):
        a = dict(cubes=ptr(self.cubes), counts=ptr(self.counts_t), cap=self.cap, keep=ptr(self.keep), usage=ptr(self.usage),
                 rows=ptr(self.rows), n_rows=self.usage.shape[0], n=self.n, total=self.total, hits=ptr(self.out[0]),
                 first=ptr(self.out[1]), sole=ptr(self.out[2]), totals=ptr(self.totals), lost=ptr(self.lost), work=ptr(self.work),
                 work_bytes=self.work.numel())
        a.update(over)
        return _lib.load().ttnet_cover_support(a["cubes"], a["counts"], a["cap"], a["keep"], a["usage"], a["rows"], a["n_rows"], a["n"],
                                               a["total"], a["hits"], a["first"], a["sole"], a["totals"], a["lost"], a["work"],
                                               a["work_bytes"], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def untouched(self):
        """No output element holds anything but the sentinel (after a refused call)."""
        torch.cuda.synchronize()
        bufs = self.out + [self.totals] + ([self.lost] if self.lost is not None else [])
        return all(bool((b == b[-1]).all()) for b in bufs)

    def result(self):
        """The outputs in the twin's form, after checking the slack and the zeros past every count."""
        torch.cuda.synchronize()
        per = []
        for k, b in enumerate(self.out):
            a = b.cpu().numpy()
            assert (a[self.total * self.cap:] == np.int64(SENTINEL)).all(), f"output {k}: written past [n_funcs][cube_cap]"
            a = a[: self.total * self.cap].reshape(self.total, self.cap)
            for f in range(self.total):
                assert not a[f, self.counts[f]:].any(), f"output {k}, function {f}: not zero past its count"
            per.append([a[f, : self.counts[f]].copy() for f in range(self.total)])
        t = self.totals.cpu().numpy()
        assert (t[self.total * 4:] == np.int64(SENTINEL)).all(), "totals: written past [n_funcs][4]"
        lost = None
        if self.lost is not None:
            w = self.lost.cpu().numpy().view(np.uint32)
            assert (w[self.total * self.words:] == 0x5EA7BEEF).all(), "lost_bits: written past [n_funcs][words]"
            lost = w[: self.total * self.words].reshape(self.total, self.words)
        bad = int(self.work[:8].cpu().numpy().view(np.int64)[0])
        return dict(hits=per[0], first=per[1], sole=per[2], totals=t[: self.total * 4].reshape(self.total, 4), lost_bits=lost, bad_rows=bad)


def assert_same(got, want, tag):
    for key in ("hits", "first", "sole"):
        for f, (a, b) in enumerate(zip(got[key], want[key])):
            if not np.array_equal(a, b):
                d = np.flatnonzero(a != b)
                raise AssertionError(f"{tag}: {key} of function {f}: {len(d)} of {len(a)} cubes differ, first at {d[0]}: device "
                                     f"{int(a[d[0]])}, twin {int(b[d[0]])}")
    assert np.array_equal(got["totals"], want["totals"]), f"{tag}: totals\n{got['totals']}\n{want['totals']}"
    assert got["bad_rows"] == want["bad_rows"], tag
    if want["lost_bits"] is not None and got["lost_bits"] is not None:
        assert np.array_equal(got["lost_bits"], want["lost_bits"]), f"{tag}: lost_bits"


def device_vs_twin(dev, covers, usage, rows, n, keep=None, tag="", **kw):
    b = Buffers(dev, covers, usage, rows, n, keep, **kw)
    assert b.call(dev) == 0, _lib.load().ttnet_last_error()
    got = b.result()
    want = R.cover_support_cpu(covers, usage, rows, n, keep, lost_bits=True)
    assert_same(got, want, tag)
    return got, want


def random_usage(seed, rows, n, zero_share=0.5, high=1000):
    """int64 ``[rows, 2^n]``: a share of the patterns never looked up, the others up to ``high`` times."""
    rng = np.random.default_rng(seed)
    u = rng.integers(1, high, size=(rows, 1 << n), dtype=np.int64)
    u[rng.random(u.shape) < zero_share] = 0
    return u


def random_keep(seed, covers, share=0.6):
    rng = np.random.default_rng(seed)
    return [rng.random(len(c)) < share for c in covers]


def cpu_covers(on, dc, n, rounds=0):
    return [M.minimise_cpu(on[i], dc[i], n, rounds) for i in range(len(on))]


def check_identities(res, covers, usage, rows, n):
    """What holds for every result, kept or pruned."""
    for f, keys in enumerate(covers):
        covered, lost = int(res["totals"][f, 0]), int(res["totals"][f, 1])
        assert int(res["first"][f].sum()) == covered
        assert (res["sole"][f] <= res["first"][f]).all() and (res["first"][f] <= res["hits"][f]).all()
        if 0 <= rows[f] < len(usage):
            held = np.zeros(1 << n, dtype=bool)
            for pts in M.cube_patterns(keys, n):
                held[pts] = True
            assert covered + lost == int(usage[rows[f]][held].sum())


@pytest.mark.parametrize("n", [1, 4, 5, 8])
def test_small_functions_kept_and_pruned(dev, n):
    """Every function of n = 1; seeded random ones above, an empty cover and the constant-1 cover among them; two functions
    per usage row; without keep flags, with random ones, with all set and with none set."""
    if n == 1:
        flags = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=bool)
        on, dc = M.pack_bits(flags), np.zeros((4, 1), dtype=np.uint32)
    else:
        on, dc = random_functions(100 + n, n, 10)
        on[3], dc[3] = 0, 0                                              # constant 0: no cube
        on[4], dc[4] = M.pack_bits(np.ones(1 << n, dtype=bool)), 0       # constant 1: key 0
    covers = cpu_covers(on, dc, n)
    assert any(len(c) == 0 for c in covers) and any(len(c) == 1 and c[0] == 0 for c in covers)
    rows = np.arange(len(covers)) // 2
    usage = random_usage(n, int(rows.max()) + 1, n)
    got, _ = device_vs_twin(dev, covers, usage, rows, n, tag=f"n={n}")
    check_identities(got, covers, usage, rows, n)
    assert not got["totals"][:, [1, 3]].any() and not got["lost_bits"].any()       # nothing is lost without keep flags
    for name, keep in (("random", random_keep(n, covers)), ("all", [np.ones(len(c), bool) for c in covers]),
                       ("none", [np.zeros(len(c), bool) for c in covers])):
        pruned, _ = device_vs_twin(dev, covers, usage, rows, n, keep, tag=f"n={n} keep {name}")
        check_identities(pruned, covers, usage, rows, n)
        if name == "all":
            assert_same(pruned, got, f"n={n}: all flags set against no flags")
        if name == "none":
            for f, keys in enumerate(covers):                            # the whole cover is lost: mass and patterns
                held = np.zeros(1 << n, dtype=bool)
                for pts in M.cube_patterns(keys, n):
                    held[pts] = True
                assert pruned["totals"][f, 0] == 0 and pruned["totals"][f, 1] == got["totals"][f, 0]
                assert np.array_equal(pruned["lost_bits"][f], M.pack_bits(held))


def parity_cover(n):
    idx = np.arange(1 << n, dtype=np.uint32)
    odd = np.array([bin(i).count("1") & 1 for i in range(1 << n)], dtype=bool)
    return ((np.uint32((1 << n) - 1) << np.uint32(16)) | idx[odd]).astype(np.uint32)


def test_sixteen_input_parity_many_chunks_and_64_bit_carries(dev):
    """32,768 minterm cubes, 32 staged chunks, every pattern held exactly once; usage values above 2^33, so the sums need
    the carries of the 64-bit adds."""
    n = 16
    cover = parity_cover(n)
    assert len(cover) == 1 << 15
    rng = np.random.default_rng(16)
    usage = rng.integers(1 << 33, 1 << 35, size=(1, 1 << n), dtype=np.int64)
    usage[0, rng.random(1 << n) < 0.25] = 0
    got, _ = device_vs_twin(dev, [cover], usage, [0], n, tag="parity 16")
    assert np.array_equal(got["hits"][0], got["first"][0]) and np.array_equal(got["hits"][0], got["sole"][0])
    assert np.array_equal(got["hits"][0], usage[0][cover & 0xFFFF])
    assert int(got["totals"][0, 0]) == int(usage[0][cover & 0xFFFF].sum()) > 1 << 45


def test_keep_flags_whole_cover_nothing_and_a_chunk_straddling_range(dev):
    """The 12-input parity function (2,048 cubes, two chunks) three times in one batch: every cube dropped, none dropped,
    cubes 1,000 .. 1,099 dropped (the range straddles the chunk edge at 1,024)."""
    n = 12
    cover = parity_cover(n)
    assert len(cover) == 2 * CHUNK
    usage = random_usage(12, 1, n, zero_share=0.3)
    straddle = np.ones(len(cover), dtype=bool)
    straddle[1000:1100] = False
    keep = [np.zeros(len(cover), bool), np.ones(len(cover), bool), straddle]
    got, _ = device_vs_twin(dev, [cover] * 3, usage, [0, 0, 0], n, keep, tag="parity 12 keep")
    mass = int(usage[0][cover & 0xFFFF].sum())
    assert got["totals"][:, 0].tolist() == [0, mass, mass - int(usage[0][cover[1000:1100] & 0xFFFF].sum())]
    assert got["totals"][:, 3].tolist() == [len(cover), 0, 100]
    assert np.array_equal(M.unpack_bits(got["lost_bits"][2], n).nonzero()[0], np.sort(cover[1000:1100] & 0xFFFF))


@pytest.mark.parametrize("rounds", [0, 2])
def test_heavy_overlap_sixteen_inputs(dev, rounds):
    """A dense random function of 16 inputs: thousands of primes that overlap heavily, so first < hits and sole < first for
    most cubes, over several chunks; beside it a sparse one that shares its usage row."""
    n = 16
    rng = np.random.default_rng(160 + rounds)
    dense, sparse = rng.random(1 << n) < 0.85, rng.random(1 << n) < 0.02
    on = np.stack([M.pack_bits(dense), M.pack_bits(sparse)])
    covers = M.minimise_device(on, None, n, dev, rounds=rounds)
    assert len(covers[0]) > 2 * CHUNK
    usage = random_usage(161, 1, n, zero_share=0.6)
    got, _ = device_vs_twin(dev, covers, usage, [0, 0], n, tag=f"dense rounds={rounds}")
    assert (got["first"][0] < got["hits"][0]).any() and (got["sole"][0] < got["first"][0]).any()
    support = dict(hits=got["hits"], row_total=usage.sum(axis=1)[[0, 0]])
    keep = R.keep_by_support(support, min_hits=int(np.median(got["hits"][0])) + 1)      # under half of the dense cover stays
    assert 0 < keep[0].sum() < len(keep[0])
    pruned, _ = device_vs_twin(dev, covers, usage, [0, 0], n, keep, tag=f"dense rounds={rounds} pruned")
    check_identities(pruned, covers, usage, [0, 0], n)
    assert pruned["totals"][0, 3] > 0


def test_sixteen_functions_share_a_row_and_bad_rows_give_zeros(dev):
    n = 8
    on, dc = random_functions(88, n, 20)
    covers = cpu_covers(on, dc, n, rounds=1)
    usage = random_usage(8, 2, n)
    rows = np.array([1] * 16 + [0, -1, 2, 1], dtype=np.int32)            # rows 17 and 18 are out of range
    for keep in (None, random_keep(8, covers)):
        got, want = device_vs_twin(dev, covers, usage, rows, n, keep, tag="shared row")
        assert got["bad_rows"] == 2
        for f in (17, 18):
            assert not got["totals"][f].any() and not got["hits"][f].any() and not got["lost_bits"][f].any()
        assert got["totals"][16].any()


def test_more_functions_than_workgroups(dev):
    n = 4
    on, dc = random_functions(44, n, 1030)
    covers = cpu_covers(on, dc, n)
    usage = random_usage(4, 103, n, zero_share=0.2)
    device_vs_twin(dev, covers, usage, np.arange(1030) // 10, n, random_keep(4, covers), tag="1030 functions")


def test_lost_bits_null_gives_the_same_other_outputs(dev):
    n = 8
    on, dc = random_functions(81, n, 6)
    covers = cpu_covers(on, dc, n)
    usage, rows = random_usage(81, 3, n), [0, 0, 1, 1, 2, 2]
    for keep in (None, random_keep(81, covers)):
        with_bits, _ = device_vs_twin(dev, covers, usage, rows, n, keep, tag="with lost_bits")
        without, _ = device_vs_twin(dev, covers, usage, rows, n, keep, tag="without lost_bits", lost=False)
        assert without["lost_bits"] is None
        assert_same(without, with_bits, "lost_bits NULL against given")


def test_wrapper_matches_the_twin(dev):
    """``rules.cover_support``: lists in, lists out, numpy or device usage, the key names of the twin."""
    n = 6
    on, dc = random_functions(66, n, 7)
    covers = cpu_covers(on, dc, n)
    usage, rows = random_usage(66, 4, n), [0, 1, 2, 3, 3, 9, 0]
    keep = random_keep(66, covers)
    for kp in (None, keep):
        want = R.cover_support_cpu(covers, usage, rows, n, kp, lost_bits=True)
        for u in (usage, torch.from_numpy(usage).to(dev)):
            got = R.cover_support(covers, u, rows, n, kp, dev, lost_bits=True)
            assert sorted(got) == sorted(want)
            assert_same(got, want, "wrapper")
            assert np.array_equal(got["row_total"], want["row_total"]) and got["row_total"][5] == 0
    assert R.cover_support(covers, usage, rows, n, device=dev)["lost_bits"] is None
    with pytest.raises(ValueError):
        R.cover_support(covers, usage[:, :32], rows, n, device=dev)
    with pytest.raises(ValueError):
        R.cover_support(covers, usage, rows, n, keep[:-1], dev)


def test_error_contract_through_raw_ctypes_nothing_launched(dev):
    n = 6
    on, dc = random_functions(60, n, 3)
    covers = cpu_covers(on, dc, n)
    b = Buffers(dev, covers, random_usage(60, 1, n), [0, 0, 0], n)
    lib = _lib.load()
    INVALID = -1
    for name in ("cubes", "counts", "usage", "rows", "hits", "first", "sole", "totals", "work"):
        assert b.call(dev, **{name: C.c_void_p(None)}) == INVALID, name
        assert b"NULL" in lib.ttnet_last_error()
    for over in (dict(n=0), dict(n=17), dict(total=0), dict(cap=0), dict(cap=-3), dict(n_rows=-1), dict(work_bytes=b.work.numel() - 1),
                 dict(work_bytes=0)):
        assert b.call(dev, **over) == INVALID, over
    for name, t, off in (("cubes", b.cubes, 2), ("counts", b.counts_t, 1), ("rows", b.rows, 2), ("lost", b.lost, 2), ("usage", b.usage, 4),
                         ("hits", b.out[0], 4), ("first", b.out[1], 4), ("sole", b.out[2], 4), ("totals", b.totals, 4), ("work", b.work, 8)):
        assert b.call(dev, **{name: C.c_void_p(t.data_ptr() + off)}) == INVALID, f"misaligned {name}"
        assert b"aligned" in lib.ttnet_last_error()
    assert b.untouched(), "a refused call wrote to an output"
    assert lib.ttnet_cover_support_workspace(0, 1) == INVALID and lib.ttnet_cover_support_workspace(17, 1) == INVALID
    assert lib.ttnet_cover_support_workspace(4, 0) == INVALID
    assert lib.ttnet_cover_support_workspace(16, 5000) == 256 + 1024 * (10 << 16) and lib.ttnet_cover_support_workspace(1, 2) == 256 + 2 * 256
    assert b.call(dev) == 0                                              # the same buffers are served once the arguments are right
    assert_same(b.result(), R.cover_support_cpu(covers, b.usage.cpu().numpy(), [0, 0, 0], n, lost_bits=True), "after the refusals")


def test_graph_capture_replayed_twice_gives_the_same_bytes(dev):
    n = 12
    cover = parity_cover(n)
    on, dc = random_functions(120, n, 3, densities=((0.5, 0.0), (0.3, 0.4)))
    covers = [cover] + M.minimise_device(on, dc, n, dev)
    usage, rows = random_usage(120, 2, n), [0, 1, 1, 0]
    keep = random_keep(120, covers, share=0.8)
    b = Buffers(dev, covers, usage, rows, n, keep)
    want = R.cover_support_cpu(covers, usage, rows, n, keep, lost_bits=True)
    stream = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            assert b.call(dev) == 0
    snaps = []
    for _ in range(2):
        for t in b.out + [b.totals, b.lost]:
            t[: -SLACK].fill_(-1)                                        # a replay has to write everything again
        graph.replay()
        torch.cuda.synchronize()
        assert_same(b.result(), want, "graph replay")
        snaps.append([t.clone() for t in b.out + [b.totals, b.lost]])
    assert all(torch.equal(x, y) for x, y in zip(*snaps))


# ---- end to end: prune the covers of a model, and prove on the care sets what the pruned circuit still gets right ---------

MIN_SHARE = 1e-4          # of a group's lookups; see test_pruned_covers_end_to_end


def p16_model(dev):
    """TT-small p = 16 --layers 1 with synthetic weights, its plan built."""
    spec = make_spec("small", 2, 8, 1)
    st = synth.synth_state_dict(spec, calibrated=False)
    m = ttnet.TT_vf_19lv3_imgnet_small(Namespace(nfilter=2, tfilter=8, layers=1, groups=[1, None, 4, None]))
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    m = m.to(dev).eval().reserve(8)
    with torch.no_grad():
        m(torch.from_numpy(synth.synth_images(1)).to(dev))
    torch.cuda.synchronize()
    return m


_P16 = {}


def p16_support(dev):
    """``(model, batch, usage, rule_support(usage))``, made once: image 0 five times, images 1 .. 3 once."""
    if "m" not in _P16:
        m = p16_model(dev)
        x = torch.from_numpy(synth.synth_images(4)[[0, 0, 1, 0, 2, 0, 3, 0]]).to(dev)
        m.count_table_usage(True)
        with torch.no_grad():
            m(x)
        m.add_table_usage(0)
        torch.cuda.synchronize()
        usage = m.table_usage()
        m.count_table_usage(False)
        _P16.update(m=m, x=x, usage=usage, support=m.rule_support(usage))
    return _P16["m"], _P16["x"], _P16["usage"], _P16["support"]


def test_pruned_covers_end_to_end(dev):
    """Usage of a batch of 8 synthetic images -> ``rule_support`` -> prune by share -> ``care_after_prune`` -> ``set_care``; a
    second model gets the tables that the pruned DNF covers compute.  Every image without a care-set miss must get the same
    logits, bit for bit, from both.

    The batch is image 0 five times and images 1, 2, 3 once (covered images by duplication, as in test_gpu_table_care.py:
    distinct synthetic images each read entries that no other image reads).  The busiest group makes 8 x 56 x 56 = 25,088
    lookups, so MIN_SHARE = 1e-4 drops the cubes with at most 2 hits there and none in a group of fewer than 10,000 lookups.
    Every entry image 0 reads was read at least 5 times, so every cube that holds it stays: image 0 must be covered, while
    the cubes that only single lookups of images 1 .. 3 justify go.  Both are asserted, so the comparison cannot pass empty."""
    m, x, usage, support = p16_support(dev)
    base = M.care_masks(usage)
    blocks = {b.name: b for b in m.spec.block_tts()}
    assert list(support) == [b.name for b in m.spec.block_tts() if not b.last]
    care, tables, dropped = {}, {}, 0
    for name, s in support.items():
        b, n = blocks[name], s["n"]
        twin = R.cover_support_cpu(s["cubes"], usage[name], s["usage_row_of"], n)
        assert_same(s, twin, f"rule_support {name}")
        keep = R.keep_by_support(s, min_share=MIN_SHARE)
        dropped += sum(int((~k).sum()) for k in keep)
        pruned = R.cover_support(s["cubes"], usage[name], s["usage_row_of"], n, keep, dev, lost_bits=True)
        care[name] = R.care_after_prune(pruned["lost_bits"], b.groups, b.cout_g, base[name])
        t = np.zeros((b.groups, 1 << n, b.cout_g), dtype=np.uint8)
        for f, (keys, k) in enumerate(zip(s["cubes"], keep)):
            for pts in M.cube_patterns(keys[k], n):
                t[f // b.cout_g, pts, f % b.cout_g] = 1
        tables[name] = t
    assert dropped > 0, "MIN_SHARE drops no cube: the pruned model is the original"
    m.set_care(care)
    with torch.no_grad():
        y = m(x)
    misses = m.care_misses(0).cpu().numpy()
    covered = ~misses.any(axis=1)
    assert covered[[0, 1, 3, 5, 7]].all(), f"image 0 is not covered: misses per image {misses.sum(axis=1).tolist()}"
    m2 = p16_model(dev)
    changed = 0
    for name, t in tables.items():
        changed += int((t != m2.get_table(name)).sum())
        m2.set_table(name, t)
    assert changed > 0
    with torch.no_grad():
        y2 = m2(x)
    torch.cuda.synchronize()
    assert torch.equal(y[torch.from_numpy(covered).to(dev)], y2[torch.from_numpy(covered).to(dev)])


def test_command_line_report(dev, tmp_path):
    """What ``main --rule_support R.csv --rule_form cnf --rule_min_share S --table_gates_rounds 1`` writes after its evaluation."""
    import csv

    from scale_imagenet_amd import main as cli, report
    m, _, usage, support = p16_support(dev)
    path = str(tmp_path / "r.csv")
    cli.write_rule_support(Namespace(rule_support=path, rule_form="cnf", rule_min_share=MIN_SHARE, table_gates_rounds=1), m, usage)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == report.RULE_FIELDS + report.RULE_PRUNED_FIELDS
    assert [r[0] for r in rows[1:]] == list(support)
    col = {k: i for i, k in enumerate(rows[0])}
    for r in rows[1:]:
        b = next(b for b in m.spec.block_tts() if b.name == r[0])
        assert r[col["form"]] == "cnf" and int(r[col["inputs"]]) == b.fan_in_bits and int(r[col["functions"]]) == b.groups * b.cout_g
        assert 0 < int(r[col["kept_cubes"]]) <= int(r[col["cubes"]]) and int(r[col["kept_literals"]]) <= int(r[col["literals"]])
        assert 0.0 < float(r[col["top1pct_first_share"]]) <= float(r[col["top10pct_first_share"]]) <= 1.0
        assert int(r[col["unused_cubes"]]) == 0                          # every cube grew from an entry that was read
        # a dropped cube holds less than MIN_SHARE of its function's lookups, and no cover here has 1,000 cubes
        assert 0.0 <= float(r[col["lost_share"]]) < 1000 * MIN_SHARE
    assert any(int(r[col["kept_cubes"]]) < int(r[col["cubes"]]) for r in rows[1:])
    cli.write_rule_support(Namespace(rule_support=path, rule_form=None, rule_min_share=None, table_gates_rounds=0), m, usage)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == report.RULE_FIELDS
    assert [int(r[4]) for r in rows[1:]] == [sum(len(c) for c in s["cubes"]) for s in support.values()]
