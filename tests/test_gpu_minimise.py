"""GPU: ttnet_minimise_covers against its CPU twin (scale_imagenet_amd.minimise.minimise_cpu), key for key.

Every device cover must equal the twin's -- the same cubes in the same order, so the counts too -- and pass
``check_cover`` (exhaustive: equal to the function on the care set, every cube prime, no cube removable).  Integer-exact:
no tolerances.  Shapes are the smallest at which the kernel takes another path: bitmaps shorter than a word (n < 5), one
and two words (n = 5, 6), cubes whose free variables straddle the in-word / lane / loop split of the word walk
(n = 9, 11: word-index bits 4 and 6; n = 16: 11, five of them stepped by the loop), more workgroups than CUs."""
import ctypes as C
import glob
import os
from argparse import Namespace
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from scale_imagenet_amd import _lib, synth, ttnet
from scale_imagenet_amd import minimise as M
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEEF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def random_functions(seed, n, count, densities=((0.5, 0.0), (0.3, 0.4), (0.05, 0.9), (0.9, 0.05), (0.02, 0.0))):
    rng = np.random.default_rng(seed)
    on, dc = [], []
    for i in range(count):
        p_on, p_dc = densities[i % len(densities)]
        r = rng.random(1 << n)
        on.append(M.pack_bits(r < p_on))
        dc.append(M.pack_bits((r >= p_on) & (r < p_on + p_dc)))
    return np.stack(on), np.stack(dc)


def twin(on, dc, n, workers=8):
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda i: M.minimise_cpu(on[i], None if dc is None else dc[i], n), range(len(on))))


def assert_same(got, want, tag):
    assert len(got) == len(want), tag
    for f, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), f"{tag} function {f}: {len(a)} cubes on the device, {len(b)} from the twin"
        if not np.array_equal(a, b):
            d = np.flatnonzero(a != b)
            raise AssertionError(f"{tag} function {f}: {len(d)} of {len(a)} keys differ, first at {d[0]}: device {int(a[d[0]]):#x}, "
                                 f"twin {int(b[d[0]]):#x}")


def as_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def raw_call(on_t, dc_t, n, cubes_t, cap, counts_t, work_t, n_funcs=None, work_bytes=None):
    """The C ABI itself on tensors the caller owns (asynchronous on the current stream); returns the status."""
    lib = _lib.load()
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    return lib.ttnet_minimise_covers(ptr(on_t), ptr(dc_t), n, on_t.shape[0] if n_funcs is None else n_funcs, ptr(cubes_t), cap,
                                     ptr(counts_t), ptr(work_t), work_t.numel() if work_bytes is None else work_bytes,
                                     C.c_void_p(torch.cuda.current_stream(on_t.device).cuda_stream))


def buffers(dev, n, n_funcs, cap, tail=0):
    lib = _lib.load()
    work = torch.empty(_lib.check(lib.ttnet_minimise_workspace(n, n_funcs)), dtype=torch.uint8, device=dev)
    cubes = torch.full((n_funcs * cap + tail,), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.full((n_funcs,), SENTINEL, dtype=torch.int32, device=dev)
    return cubes, counts, work


@pytest.mark.parametrize("n,count", [(1, 10), (2, 10), (4, 20), (5, 20), (6, 20), (9, 15), (11, 10)])
def test_small_inputs_equal_the_twin(dev, n, count):
    on, dc = random_functions(1000 + n, n, count)
    got = M.minimise_device(on, dc, n, dev)
    assert_same(got, twin(on, dc, n), f"n={n}")
    for f in range(count):
        M.check_cover(on[f], dc[f], n, got[f])


def test_free_variables_straddle_the_word_walk(dev):
    """Hand-made cubes whose free variables sit on both sides of every split of the walk: index bits 3..6 (in-word and
    lane), 9..12 at n = 16 (lane bits end at word-index bit 6 = index bit 10 when bits 5..10 are free)."""
    for n, free_sets in ((9, [0b001111000, 0b111100000, 0b100010001]), (11, [0b11111100000, 0b10000110000, 0b11111111110]),
                         (16, [0xFFE0, 0xFFF0, 0x8421, 0x0FF0, 0xFFFE])):
        idx = np.arange(1 << n)
        on = np.stack([M.pack_bits((idx & ~fr & ((1 << n) - 1)) == (0x5555 & ~fr & ((1 << n) - 1))) for fr in free_sets])
        got = M.minimise_device(on, None, n, dev)
        for f, fr in enumerate(free_sets):
            mask = ~fr & ((1 << n) - 1)
            assert got[f].tolist() == [mask << 16 | (0x5555 & mask)], (n, hex(fr), [hex(int(k)) for k in got[f][:4]])


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
    rng = np.random.default_rng(16)
    r = rng.random(1 << n)
    one = np.zeros(1 << n, dtype=bool)
    one[40000] = True
    m, _ = small_p16(dev)
    real = m.get_table("features.4.Block_conv1")[3, :, 0] == 1
    none = np.zeros(1 << n, dtype=bool)
    cases = [("dense random", r < 0.5, none), ("sparse ON, 99 % don't-care", r < 0.005, (r >= 0.005) & (r < 0.995)),
             ("one ON pattern", one, ~one), ("ON empty", none, none), ("OFF empty", ~none, none),
             ("features.4.Block_conv1 group 3", real, none)]
    on = np.stack([M.pack_bits(c[1]) for c in cases])
    dc = np.stack([M.pack_bits(c[2]) for c in cases])
    got = M.minimise_device(on, dc, n, dev)
    assert_same(got, twin(on, dc, n, workers=6), "n=16")
    assert [len(g) for g in got][2:5] == [1, 0, 1] and got[2].tolist() == [0] and got[4].tolist() == [0]
    for f, c in enumerate(cases):
        M.check_cover(on[f], dc[f], n, got[f])


def test_one_function_and_more_workgroups_than_cus(dev):
    n = 6
    on, dc = random_functions(66, n, 300)
    want = twin(on, dc, n)
    assert_same(M.minimise_device(on, dc, n, dev), want, "300 functions")
    assert_same(M.minimise_device(on[17:18], dc[17:18], n, dev), want[17:18], "one function")


def test_null_dc_is_an_all_zero_dc(dev):
    n = 8
    on, _ = random_functions(8, n, 12, densities=((0.5, 0.0), (0.1, 0.0), (0.9, 0.0)))
    a = M.minimise_device(on, None, n, dev)
    b = M.minimise_device(on, np.zeros_like(on), n, dev)
    assert_same(a, b, "dc NULL / zero")
    assert_same(a, twin(on, None, n), "dc NULL")


def test_cap_overflow_reports_the_true_count_and_writes_nothing_past_the_cap(dev):
    n = 8
    on, dc = random_functions(88, n, 5)
    want = twin(on, dc, n)
    sizes = [len(w) for w in want]
    big = int(np.argmax(sizes))
    cap = sizes[big] - 1
    assert cap >= 1
    cubes, counts, work = buffers(dev, n, 5, cap, tail=64)
    assert raw_call(as_dev(on, dev), as_dev(dc, dev), n, cubes, cap, counts, work) == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == sizes                                    # the TRUE sizes, also of the one that overflowed
    rows = cubes.cpu().numpy()
    assert (rows[5 * cap:] == SENTINEL).all()                                # nothing after the buffer
    for f in range(5):
        row = rows[f * cap:(f + 1) * cap]
        k = min(sizes[f], cap)
        assert np.array_equal(row[:k].view(np.uint32), want[f][:k]) and (row[k:] == SENTINEL).all(), f
    # cap 0: counts only
    cubes0, counts0, _ = buffers(dev, n, 5, 0, tail=8)
    assert raw_call(as_dev(on, dev), as_dev(dc, dev), n, cubes0, 0, counts0, work) == 0
    torch.cuda.synchronize()
    assert counts0.cpu().tolist() == sizes and (cubes0.cpu().numpy() == SENTINEL).all()
    # the retry of minimise_device returns the full covers
    assert_same(M.minimise_device(on, dc, n, dev, cube_cap=cap), want, "retry")
    assert_same(M.minimise_device(on, dc, n, dev, cube_cap=1), want, "retry from cap 1")


def test_determinism_and_graph_replay(dev):
    n, count, cap = 9, 40, 512
    on_a, dc_a = random_functions(91, n, count)
    on_b, dc_b = random_functions(92, n, count)
    on_t, dc_t = as_dev(on_a, dev), as_dev(dc_a, dev)
    cubes, counts, work = buffers(dev, n, count, cap)

    def plain(on, dc):
        on_t.copy_(as_dev(on, dev))
        dc_t.copy_(as_dev(dc, dev))
        cubes.fill_(SENTINEL)
        assert raw_call(on_t, dc_t, n, cubes, cap, counts, work) == 0
        torch.cuda.synchronize()
        return cubes.cpu().numpy().copy(), counts.cpu().numpy().copy()

    first, again = plain(on_a, dc_a), plain(on_a, dc_a)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    want_b = plain(on_b, dc_b)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        assert raw_call(on_t, dc_t, n, cubes, cap, counts, work) == 0           # warm-up outside capture
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        status = raw_call(on_t, dc_t, n, cubes, cap, counts, work)
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
    assert_same(got, twin(on_b, dc_b, n), "graph inputs")


def test_invalid_arguments_launch_nothing(dev):
    n = 6
    on, dc = random_functions(6, n, 3)
    on_t, dc_t = as_dev(on, dev), as_dev(dc, dev)
    cubes, counts, work = buffers(dev, n, 3, 64)
    lib = _lib.load()
    E = -1                                                                   # TTNET_E_INVALID
    assert raw_call(on_t, dc_t, 0, cubes, 64, counts, work) == E
    assert raw_call(on_t, dc_t, 17, cubes, 64, counts, work) == E
    assert raw_call(on_t, dc_t, n, cubes, 64, counts, work, n_funcs=0) == E
    assert raw_call(on_t, dc_t, n, cubes, -1, counts, work) == E
    assert raw_call(on_t, dc_t, n, None, 64, counts, work) == E
    assert raw_call(on_t, dc_t, n, cubes, 64, None, work) == E
    assert raw_call(on_t, dc_t, n, cubes, 64, counts, work, work_bytes=work.numel() - 1) == E
    assert b"workspace" in lib.ttnet_last_error()
    assert raw_call(on_t, dc_t, n, cubes.view(torch.uint8)[1:], 32, counts, work) == E      # misaligned cubes
    assert lib.ttnet_minimise_covers(None, None, n, 3, C.c_void_p(cubes.data_ptr()), 64, C.c_void_p(counts.data_ptr()),
                                     C.c_void_p(work.data_ptr()), work.numel(), None) == E
    assert lib.ttnet_minimise_workspace(0, 3) == E and lib.ttnet_minimise_workspace(17, 3) == E and lib.ttnet_minimise_workspace(6, 0) == E
    assert lib.ttnet_minimise_workspace(16, 5000) == 1024 * (8 << 16) and lib.ttnet_minimise_workspace(1, 2) == 2 * 256
    torch.cuda.synchronize()
    assert (cubes.cpu().numpy() == SENTINEL).all() and (counts.cpu().numpy() == SENTINEL).all()       # nothing ran
    assert raw_call(on_t, dc_t, n, cubes, 64, counts, work) == 0
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() >= 0).all()


def evaluate_text(text, n):
    idx = np.arange(1 << n)
    env = {f"x_{j}": ((idx >> (n - 1 - j)) & 1).astype(bool) for j in range(n)}
    return np.broadcast_to(eval(text, {"__builtins__": {}}, {**env, "True": True, "False": False}), idx.shape)


_COUNTS = {}


@pytest.mark.parametrize("name", ["features.4.Block_conv1", "features.4.Block_conv3"])      # a depthwise and a grouped 1x1 block
def test_end_to_end_gate_counts_agree_with_the_twin(dev, name):
    m, usage = small_p16(dev)
    if not _COUNTS:
        _COUNTS["full"], _COUNTS["seen"] = m.gate_counts(), m.gate_counts(usage)
    full, seen = _COUNTS["full"], _COUNTS["seen"]
    names = [b.name for b in m.spec.block_tts() if not b.last]
    assert list(full) == names == list(seen) and "features.5.Block_convf" not in full
    table = m.get_table(name)
    for u, got in ((None, full[name]), (usage[name], seen[name])):
        on, dc = M.pack_functions(table, u)
        off = M.complement(on, dc, 16)
        covers = twin(np.concatenate([on, off]), np.concatenate([dc, dc]), 16, workers=16)
        want = dict(filters=len(on), constant=0, dnf_cubes=0, dnf_literals=0, cnf_cubes=0, cnf_literals=0)
        for d, c in zip(covers[:len(on)], covers[len(on):]):
            if M.literal_total(d) == 0 or M.literal_total(c) == 0:
                want["constant"] += 1
                continue
            want["dnf_cubes"] += len(d)
            want["dnf_literals"] += M.literal_total(d)
            want["cnf_cubes"] += len(c)
            want["cnf_literals"] += M.literal_total(c)
        assert got == want, (name, u is not None)


def test_end_to_end_dontcares_and_export(dev, tmp_path):
    m, usage = small_p16(dev)
    # don't-cares never cost: per filter, unless the filter is constant on the patterns seen
    name = "features.4.Block_conv2"
    table, u = m.get_table(name), usage[name]
    on0, dc0 = M.pack_functions(table)
    on1, dc1 = M.pack_functions(table, u)
    a = M.minimal_covers(on0, dc0, 16, "device", dev)
    b = M.minimal_covers(on1, dc1, 16, "device", dev)
    compared = 0
    for f in range(len(a)):
        if M.literal_total(b[f][0]) == 0 or M.literal_total(b[f][1]) == 0:
            continue
        compared += 1
        assert len(b[f][0]) <= len(a[f][0]) and len(b[f][1]) <= len(a[f][1]), f
        assert M.literal_total(b[f][0]) <= M.literal_total(a[f][0]) and M.literal_total(b[f][1]) <= M.literal_total(a[f][1]), f
    assert compared > 0
    # files for n = 16: the text reproduces the table column on every pattern seen
    out = m.export_truth_tables(name, str(tmp_path), block=4, sub_block=1, filters=[0, 5], usage=u, minimiser="device")
    checked = 0
    for f, rec in out.items():
        col = table[f, :, 0] == 1
        seen_f = u[f] > 0
        if rec["dnf"] is None:
            assert len(np.unique(col[seen_f])) <= 1
            continue
        checked += 1
        for key, stem in (("dnf", "DNF_expression"), ("cnf", "CNF_expression")):
            (path,) = glob.glob(os.path.join(str(tmp_path), f"{stem}_block4_filter_{f}_coefdefault_*_sousblock_1.txt"))
            text = open(path).read()
            assert text == rec[key]
            assert np.array_equal(evaluate_text(text, 16)[seen_f], col[seen_f]), (f, key)
        assert rec["dnf_literals"] > 0 and rec["cnf_literals"] > 0 and rec["csv"] and rec["cnf_with_y"]
    assert checked > 0
