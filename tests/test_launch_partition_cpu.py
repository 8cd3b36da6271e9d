"""ttnet_launch_partition on a machine without a GPU: its error contract, and the properties every partition it reports
must have (each (strand, slice) has one owner, the slices tile the batch, the stem's runs tile the items)."""
import ctypes as C

import pytest

from _gate_partition import part
from scale_imagenet_amd import _lib

SENTINEL = -12345


def _call(what, args, out_cap, n_args=None):
    """(status, out buffer of 8 values beyond which nothing may be written, message)"""
    part("fused.const")                                   # (builds the library if it is missing)
    lib = _lib.load()
    a = (C.c_int64 * max(1, len(args)))(*args)
    out = (C.c_int64 * 8)(*([SENTINEL] * 8))
    st = lib.ttnet_launch_partition(what.encode(), a, len(args) if n_args is None else n_args, out, out_cap)
    return st, list(out), lib.ttnet_last_error().decode()


def test_a_good_call_writes_its_values_and_nothing_more():
    st, out, _ = _call("fused.launch", [64, 29, 600], 8)
    assert st == 4 and out == [256, 32, 8, 1] + [SENTINEL] * 4
    st, out, _ = _call("fused.launch", [64, 29, 600], 4)                # out_cap exactly what the key writes
    assert st == 4 and out[4:] == [SENTINEL] * 4
    assert part("stem.run", 5, 150, 128) == (41, 8)


@pytest.mark.parametrize("what,args,out_cap,n_args,needle", [
    ("fused.lunch", [64, 29, 600], 8, None, "unknown key fused.lunch"),
    ("fused.launch", [64, 29], 8, None, "takes 3 arguments (C, HO, n), got 2"),
    ("fused.launch", [64, 29, 600, 1], 8, None, "takes 3 arguments"),
    ("stem.const", [], 8, 1, "takes 0 arguments"),
    ("fused.launch", [64, 29, 600], 3, None, "writes 4 values, out_cap is 3"),
    ("fused.launch", [64, 29, 600], 0, None, "out_cap is 0"),
    ("fused.launch", [64, 29, 0], 8, None, "n=0"),
    ("fused.launch", [64, 29, -3], 8, None, "n=-3"),
    ("stem.run", [0, 0, 128], 8, None, "n=0"),
    ("two_launch.stage1", [64, 0], 8, None, "n=0"),
    ("fused.launch", [60, 29, 600], 8, None, "C=60 must be a multiple of 8"),
    ("fused.owner", [0, 12, 600], 8, None, "C=12 must be a multiple of 8"),
    ("fused.launch", [0, 29, 600], 8, None, "C=0"),
    ("two_launch.stage1", [24, 600], 8, None, "C=24 must be a multiple of 16"),
    ("fused.owner", [256, 64, 600], 8, None, "b=256 but the grid is 256"),
    ("stem.run", [128, 150, 128], 8, None, "bid=128 but the grid is 128"),
    ("slice", [4, 10, 4], 8, None, "sl=4 but there are 4 slices"),
    ("full.row_bundle", [56, 65], 8, None, "W=65"),
])
def test_error_contract(what, args, out_cap, n_args, needle):
    st, out, msg = _call(what, args, out_cap, n_args)
    assert st < 0, (what, args)
    assert needle in msg, msg
    assert out == [SENTINEL] * 8                          # nothing written, in particular nothing past out_cap
    with pytest.raises(_lib.TTNetError):
        _lib.check(st)


def test_null_arguments_are_refused():
    lib = _lib.load()
    out = (C.c_int64 * 8)()
    assert lib.ttnet_launch_partition(None, None, 0, out, 8) < 0
    assert lib.ttnet_launch_partition(b"fused.round", None, 1, out, 8) < 0
    assert lib.ttnet_launch_partition(b"stem.const", None, 0, None, 8) < 0
    assert lib.ttnet_launch_partition(b"stem.const", None, 0, out, 8) == 4          # (no arguments: a null args is fine)


@pytest.mark.parametrize("strands", [2, 8, 16])
def test_every_strand_slice_has_one_owner_and_the_slices_tile_the_batch(strands):
    Cin = 8 * strands
    for n in range(1, 301):
        grid, slices, R, _ = part("fused.launch", Cin, 29, n)
        assert grid == strands * slices and 1 <= R <= 8
        owners = [part("fused.owner", b, Cin, n) for b in range(grid)]
        assert sorted(owners) == [(st, sl) for st in range(strands) for sl in range(slices)], (strands, n)
        bounds = [part("slice", sl, n, slices) for sl in range(slices)]
        assert bounds[0][0] == 0 and bounds[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:])) and all(n0 <= n1 for n0, n1 in bounds)
        assert max(n1 - n0 for n0, n1 in bounds) - min(n1 - n0 for n0, n1 in bounds) <= 1
        # the two-launch kernels cut the same way
        units, pf = part("two_launch.pf", Cin, n)
        assert units == strands and 1 <= pf <= n and units * pf <= max(256, units)
        if Cin % 16 == 0:
            g, n_dw, sl_dw, n_pw, sl_pw = part("two_launch.stage1", Cin, n)
            assert g == n_dw * sl_dw + n_pw * sl_pw and 1 <= sl_dw <= n and 1 <= sl_pw <= n


@pytest.mark.parametrize("G", [128, 256])
def test_stem_runs_tile_the_items(G):
    nblk = part("stem.const")[0]
    assert nblk == 7
    for n in range(1, 301):
        grid = part("stem.grid", n, G)[0]
        assert grid == min(nblk * n, G)
        runs = [part("stem.run", b, n, G) for b in range(grid)]
        assert runs[0][0] == 0 and sum(runs[-1]) == nblk * n
        assert all(a[0] + a[1] == b[0] for a, b in zip(runs, runs[1:])) and all(items >= 1 for _, items in runs)
        assert max(i for _, i in runs) - min(i for _, i in runs) <= 1
