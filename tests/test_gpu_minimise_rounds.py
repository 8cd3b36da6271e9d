"""GPU: ttnet_minimise_covers_rounds against its CPU twin (minimise_cpu(..., rounds)), key for key.

Every device cover must equal the twin's for the same ``rounds`` -- the same cubes in the same order -- so whatever the twin's
tests establish (never more literals, prime and irredundant, the pinned totals) holds for the device too.  Integer-exact: no
tolerances.  The shapes are the smallest at which the cube walk takes another path (test_gpu_minimise.py's docstring), the
batches those at which a workgroup meets its round state again."""
import ctypes as C
import glob
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from _minimise_util import SENTINEL, assert_same, evaluate_text, random_functions, size, twin
from scale_imagenet_amd import _lib, synth, ttnet
from scale_imagenet_amd import minimise as M
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

E_INVALID = -1                                                                  # TTNET_E_INVALID


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def as_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def raw_call(on_t, dc_t, n, rounds, cubes_t, cap, counts_t, work_t, work_bytes=None):
    """The C ABI itself on tensors the caller owns (asynchronous on the current stream); returns the status."""
    lib = _lib.load()
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    return lib.ttnet_minimise_covers_rounds(ptr(on_t), ptr(dc_t), n, on_t.shape[0], rounds, ptr(cubes_t), cap, ptr(counts_t), ptr(work_t),
                                            work_t.numel() if work_bytes is None else work_bytes,
                                            C.c_void_p(torch.cuda.current_stream(on_t.device).cuda_stream))


def buffers(dev, n, n_funcs, cap, tail=0):
    lib = _lib.load()
    work = torch.empty(_lib.check(lib.ttnet_minimise_rounds_workspace(n, n_funcs)), dtype=torch.uint8, device=dev)
    cubes = torch.full((n_funcs * cap + tail,), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((n_funcs,), SENTINEL, dtype=torch.int32, device=dev)
    return cubes, counts, work


def run_raw(dev, on, dc, n, rounds, cap):
    """One call with its own buffers -> (cubes [F * cap] int32, counts [F]) on the host."""
    cubes, counts, work = buffers(dev, n, len(on), cap)
    assert raw_call(as_dev(on, dev), None if dc is None else as_dev(dc, dev), n, rounds, cubes, cap, counts, work) == 0
    torch.cuda.synchronize()
    return cubes.cpu().numpy(), counts.cpu().numpy()


# index bits 3..6 (in-word and lane) and the stepped bits: the free-variable sets of test_free_variables_straddle_the_word_walk
STRADDLE = {9: [0b001111000, 0b111100000, 0b100010001], 11: [0b11111100000, 0b10000110000, 0b11111111110]}


def straddling_functions(n):
    """Functions whose primes are cubes with the free sets of STRADDLE: each cube alone, each with two more cubes of the same
    free set beside it, the union of those that leave two literals or more, and that union among scattered ON minterms and
    don't-cares, which the rounds then reduce and expand across the splits of the walk."""
    idx, full = np.arange(1 << n), (1 << n) - 1
    cube = lambda fr, base: (idx & ~fr & full) == (base & ~fr & full)
    alone = [cube(fr, 0x5555) for fr in STRADDLE[n]]
    trios = [cube(fr, 0x5555) | cube(fr, 0x2AAA) | cube(fr, 0x1234) for fr in STRADDLE[n]]
    union = np.logical_or.reduce([t for fr, t in zip(STRADDLE[n], trios) if bin(~fr & full).count("1") >= 2])
    r = np.random.default_rng(n).random(1 << n)
    on = alone + trios + [union, union | (r < 0.03), union | (r < 0.03)]
    dc = [np.zeros_like(union)] * (len(on) - 1) + [(r > 0.8) & ~union]
    return np.stack([M.pack_bits(a) for a in on]), np.stack([M.pack_bits(a) for a in dc])


@pytest.mark.parametrize("n,count", [(1, 10), (2, 10), (4, 20), (5, 20), (6, 20), (9, 15), (11, 10)])
def test_small_inputs_equal_the_twin(dev, n, count):
    on, dc = random_functions(3000 + n, n, count)
    if n in STRADDLE:
        s_on, s_dc = straddling_functions(n)
        on, dc = np.concatenate([on, s_on]), np.concatenate([dc, s_dc])
    plain = M.minimise_device(on, dc, n, dev)
    shrunk = 0
    for rounds in (1, 2, 4):
        got = M.minimise_device(on, dc, n, dev, rounds=rounds)
        assert_same(got, twin(on, dc, n, rounds), f"n={n} rounds={rounds}")
        for f in range(len(on)):
            M.check_cover(on[f], dc[f], n, got[f])
            assert size(got[f]) <= size(plain[f]), (n, rounds, f)
            shrunk += size(got[f]) < size(plain[f])
    assert shrunk > 0 or n < 4, "no cover of the batch got smaller: the rounds did nothing"


_SIXTEEN = {}


def small_p16(dev):
    """TT-small p = 16 --layers 0 with synthetic weights, four images forwarded with table usage on (built once)."""
    if "m" not in _SIXTEEN:
        spec = make_spec("small", 2, 8, 0)
        st = synth.synth_state_dict(spec, calibrated=False)
        m = ttnet.TT_vf_19lv3_imgnet_small(Namespace(nfilter=2, tfilter=8, layers=0, groups=[1, None, 4, None]))
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
        m = m.to(dev).eval().reserve(4)
        m.count_table_usage(True)
        with torch.no_grad():
            m(torch.from_numpy(synth.synth_images(4)).to(dev))
        m.add_table_usage(0)
        torch.cuda.synchronize()
        _SIXTEEN["m"], _SIXTEEN["usage"] = m, m.table_usage()
    return _SIXTEEN["m"], _SIXTEEN["usage"]


def test_sixteen_inputs(dev):
    n = 16
    m, _ = small_p16(dev)
    real = m.get_table("features.4.Block_conv1")[3, :, 0] == 1
    rng = np.random.default_rng(1616)
    f, d = rng.random(1 << n) < 0.5, rng.random(1 << n) < 0.4
    on = np.stack([M.pack_bits(real), M.pack_bits(f & ~d)])
    dc = np.stack([M.pack_bits(np.zeros(1 << n, dtype=bool)), M.pack_bits(d)])
    got = M.minimise_device(on, dc, n, dev, rounds=2)
    plain = M.minimise_device(on, dc, n, dev)
    assert_same(got, twin(on, dc, n, 2, workers=2), "n=16 rounds=2")
    for k in range(2):
        M.check_cover(on[k], dc[k], n, got[k])
        assert size(got[k]) < size(plain[k]), k


def test_no_rounds_through_the_new_entry_point_is_ttnet_minimise_covers(dev):
    n, count, cap = 8, 25, 256
    on, dc = random_functions(80, n, count)
    on_t, dc_t = as_dev(on, dev), as_dev(dc, dev)
    lib = _lib.load()
    old_work = torch.empty(_lib.check(lib.ttnet_minimise_workspace(n, count)), dtype=torch.uint8, device=dev)
    old_cubes, old_counts, _ = buffers(dev, n, count, cap)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.ttnet_minimise_covers(ptr(on_t), ptr(dc_t), n, count, ptr(old_cubes), cap, ptr(old_counts), ptr(old_work), old_work.numel(),
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    cubes, counts, work = buffers(dev, n, count, cap)
    assert raw_call(on_t, dc_t, n, 0, cubes, cap, counts, work) == 0
    torch.cuda.synchronize()
    assert torch.equal(cubes, old_cubes) and torch.equal(counts, old_counts)
    assert (counts.cpu().numpy() > 0).any() and (cubes.cpu().numpy() == SENTINEL).any()       # covers, and the rows' unused ends
    assert lib.ttnet_minimise_rounds_workspace(16, 5000) == 1024 * (16 << 16) and lib.ttnet_minimise_rounds_workspace(1, 2) == 2 * 256


def test_more_functions_than_workgroups(dev):
    """1,030 functions on 1,024 workgroups: six workgroups take a second function, after a first one that ran its rounds."""
    n, count = 4, 1030
    on, dc = random_functions(44, n, count)
    got = M.minimise_device(on, dc, n, dev, rounds=2)
    assert_same(got, twin(on, dc, n, 2), "1030 functions")


def test_constant_one_cube_and_dense_functions_in_one_batch(dev):
    n = 8
    idx = np.arange(1 << n)
    none, every = np.zeros(1 << n, dtype=bool), np.ones(1 << n, dtype=bool)
    one_cube = (idx & 0b10100000) == 0b10000000
    rnd_on, rnd_dc = random_functions(81, n, 6, densities=((0.5, 0.0), (0.4, 0.3)))
    flags = [(none, none), (every, none), (one_cube, none), (none, every), (one_cube, ~one_cube & (idx % 3 == 0))]
    on = np.concatenate([np.stack([M.pack_bits(a) for a, _ in flags]), rnd_on])
    dc = np.concatenate([np.stack([M.pack_bits(b) for _, b in flags]), rnd_dc])
    order = np.array([5, 0, 6, 1, 7, 2, 8, 3, 9, 4, 10])                        # dense and trivial functions interleaved
    on, dc = on[order], dc[order]
    for rounds in (1, 4):
        got = M.minimise_device(on, dc, n, dev, rounds=rounds)
        assert_same(got, twin(on, dc, n, rounds), f"mixed batch rounds={rounds}")
    assert [len(got[k]) for k in (1, 3, 5, 7)] == [0, 1, 1, 0]


def test_null_dc_is_an_all_zero_dc(dev):
    n = 8
    on, _ = random_functions(8, n, 12, densities=((0.5, 0.0), (0.1, 0.0), (0.9, 0.0)))
    a = M.minimise_device(on, None, n, dev, rounds=2)
    b = M.minimise_device(on, np.zeros_like(on), n, dev, rounds=2)
    assert_same(a, b, "dc NULL / zero")
    assert_same(a, twin(on, None, n, 2), "dc NULL")


def test_cap_overflow_reports_the_true_count_and_writes_nothing_past_the_cap(dev):
    n, rounds = 8, 2
    on, dc = random_functions(88, n, 5)
    want = twin(on, dc, n, rounds)
    sizes = [len(w) for w in want]
    cap = max(sizes) - 1
    assert cap >= 1
    cubes, counts, work = buffers(dev, n, 5, cap, tail=64)
    assert raw_call(as_dev(on, dev), as_dev(dc, dev), n, rounds, cubes, cap, counts, work) == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == sizes                                    # the TRUE sizes, also of the one that overflowed
    rows = cubes.cpu().numpy()
    assert (rows[5 * cap:] == SENTINEL).all()                                # nothing after the buffer
    for f in range(5):
        row = rows[f * cap:(f + 1) * cap]
        k = min(sizes[f], cap)
        assert np.array_equal(row[:k].view(np.uint32), want[f][:k]) and (row[k:] == SENTINEL).all(), f
    # a second call with the count as cap: the full covers
    full, full_counts = run_raw(dev, on, dc, n, rounds, max(sizes))
    assert full_counts.tolist() == sizes
    for f in range(5):
        assert np.array_equal(full.reshape(5, -1)[f, :sizes[f]].view(np.uint32), want[f]), f
    # cap 0: counts only
    cubes0, counts0, _ = buffers(dev, n, 5, 0, tail=8)
    assert raw_call(as_dev(on, dev), as_dev(dc, dev), n, rounds, cubes0, 0, counts0, work) == 0
    torch.cuda.synchronize()
    assert counts0.cpu().tolist() == sizes and (cubes0.cpu().numpy() == SENTINEL).all()
    # the retry of minimise_device
    assert_same(M.minimise_device(on, dc, n, dev, cube_cap=1, rounds=rounds), want, "retry from cap 1")


def test_determinism_and_graph_replay(dev):
    n, count, cap, rounds = 9, 40, 512, 2
    on_a, dc_a = random_functions(91, n, count)
    on_b, dc_b = random_functions(92, n, count)
    on_t, dc_t = as_dev(on_a, dev), as_dev(dc_a, dev)
    cubes, counts, work = buffers(dev, n, count, cap)

    def plain(on, dc):
        on_t.copy_(as_dev(on, dev))
        dc_t.copy_(as_dev(dc, dev))
        cubes.fill_(SENTINEL)
        assert raw_call(on_t, dc_t, n, rounds, cubes, cap, counts, work) == 0
        torch.cuda.synchronize()
        return cubes.cpu().numpy().copy(), counts.cpu().numpy().copy()

    first, again = plain(on_a, dc_a), plain(on_a, dc_a)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    want_b = plain(on_b, dc_b)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert raw_call(on_t, dc_t, n, rounds, cubes, cap, counts, work) == 0   # warm-up outside capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        status = raw_call(on_t, dc_t, n, rounds, cubes, cap, counts, work)
    assert status == 0
    for on, dc, want in ((on_a, dc_a, first), (on_b, dc_b, want_b)):            # replayed with new bitmap contents
        on_t.copy_(as_dev(on, dev))
        dc_t.copy_(as_dev(dc, dev))
        cubes.fill_(SENTINEL)
        counts.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(cubes.cpu().numpy(), want[0]) and np.array_equal(counts.cpu().numpy(), want[1])
    assert (want_b[1] <= cap).all()
    got = [want_b[0].reshape(count, cap)[f, :want_b[1][f]].view(np.uint32) for f in range(count)]
    assert_same(got, twin(on_b, dc_b, n, rounds), "graph inputs")


def test_invalid_arguments_launch_nothing(dev):
    n = 6
    on, dc = random_functions(6, n, 3)
    on_t, dc_t = as_dev(on, dev), as_dev(dc, dev)
    cubes, counts, work = buffers(dev, n, 3, 64)
    lib = _lib.load()
    assert raw_call(on_t, dc_t, n, 9, cubes, 64, counts, work) == E_INVALID
    assert b"rounds" in lib.ttnet_last_error()
    assert raw_call(on_t, dc_t, n, -1, cubes, 64, counts, work) == E_INVALID
    assert raw_call(on_t, dc_t, n, 2, cubes, 64, counts, work, work_bytes=work.numel() - 1) == E_INVALID
    assert b"ttnet_minimise_rounds_workspace" in lib.ttnet_last_error()
    small = _lib.check(lib.ttnet_minimise_workspace(n, 3))                   # enough for ttnet_minimise_covers, not for rounds
    assert small < work.numel() and raw_call(on_t, dc_t, n, 2, cubes, 64, counts, work, work_bytes=small) == E_INVALID
    assert raw_call(on_t, dc_t, n, 2, None, 64, counts, work) == E_INVALID
    assert raw_call(on_t, dc_t, n, 2, cubes, 64, None, work) == E_INVALID
    assert raw_call(on_t, dc_t, n, 2, cubes.view(torch.uint8)[1:], 32, counts, work) == E_INVALID      # misaligned cubes
    assert raw_call(on_t, dc_t, n, 2, cubes, 64, counts, work[4:], work_bytes=work.numel() - 4) == E_INVALID   # misaligned workspace
    assert raw_call(on_t, dc_t, 17, 2, cubes, 64, counts, work) == E_INVALID
    assert raw_call(on_t, dc_t, n, 2, cubes, -1, counts, work) == E_INVALID
    assert lib.ttnet_minimise_rounds_workspace(0, 3) == E_INVALID and lib.ttnet_minimise_rounds_workspace(17, 3) == E_INVALID
    torch.cuda.synchronize()
    assert (cubes.cpu().numpy() == SENTINEL).all() and (counts.cpu().numpy() == SENTINEL).all()       # nothing ran
    assert raw_call(on_t, dc_t, n, 2, cubes, 64, counts, work) == 0
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() >= 0).all()
    with pytest.raises(ValueError):
        M.minimise_device(on, dc, n, dev, rounds=9)


_COUNTS = {}


@pytest.mark.parametrize("name", ["features.4.Block_conv1", "features.4.Block_conv3"])      # a depthwise and a grouped 1x1 block
def test_end_to_end_gate_counts_and_export(dev, name, tmp_path):
    """``gate_counts(rounds=2)`` on the whole tables and with the don't-cares of the four images, as ``main --table_gates``
    asks for them, against the twin on every filter of the block.  The whole 16-input tables are the heavy case (covers of
    some thousand cubes): the twin takes most of this test's time there."""
    m, usage = small_p16(dev)
    if not _COUNTS:
        _COUNTS["full"] = m.gate_counts(), m.gate_counts(rounds=2)
        _COUNTS["seen"] = m.gate_counts(usage), m.gate_counts(usage, rounds=2)
    names = [b.name for b in m.spec.block_tts() if not b.last]
    table, u = m.get_table(name), usage[name]
    for use, key in ((None, "full"), (u, "seen")):
        plain, two = _COUNTS[key][0][name], _COUNTS[key][1][name]
        assert list(_COUNTS[key][1]) == names == list(_COUNTS[key][0])
        on, dc = M.pack_functions(table, use)
        assert two == M.gate_count_row(on, dc, 16, "cpu", rounds=2), key
        for block in names:                                                  # every block of the model, not only this one
            for lits in ("dnf_literals", "cnf_literals"):
                assert _COUNTS[key][1][block][lits] <= _COUNTS[key][0][block][lits], (key, block, lits)
        assert two["filters"] == plain["filters"] and two["constant"] == plain["constant"]
        assert two["dnf_literals"] + two["cnf_literals"] < plain["dnf_literals"] + plain["cnf_literals"], key
    # the files: the text reproduces the table column on every pattern seen
    cout_g = table.shape[2]
    out = m.export_truth_tables(name, str(tmp_path), block=4, sub_block=1, filters=[0, 5], usage=u, minimiser="device", rounds=2)
    covers = M.minimal_covers(on[[0, 5]], dc[[0, 5]], 16, "cpu", rounds=2)
    checked = 0
    for (f, rec), (dnf, cnf) in zip(out.items(), covers):
        col = table[f // cout_g, :, f % cout_g] == 1
        seen_f = u[f // cout_g] > 0
        if rec["dnf"] is None:
            assert len(np.unique(col[seen_f])) <= 1
            continue
        checked += 1
        assert rec["dnf"] == M.dnf_text(dnf, 16) and rec["cnf"] == M.cnf_text(cnf, 16)
        for key, stem in (("dnf", "DNF_expression"), ("cnf", "CNF_expression")):
            (path,) = glob.glob(os.path.join(str(tmp_path), f"{stem}_block4_filter_{f}_coefdefault_*_sousblock_1.txt"))
            text = open(path).read()
            assert text == rec[key]
            assert np.array_equal(evaluate_text(text, 16)[seen_f], col[seen_f]), (f, key)
    assert checked > 0
