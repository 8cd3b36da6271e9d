"""The batch sizes of tests/test_gpu_stem_batches.py reach what they are meant to reach (no GPU needed).

The GPU sweep compares bits; how long a workgroup's run of items is, whether it starts in the middle of an image and
whether an image boundary falls inside it follow from integer arithmetic alone (tests/_stem_partition.py, which reads
stem.hip's item partition, csrc/partition.h, from the library).  This file asserts that the size list reaches every case on both grids, so that the sweep
cannot quietly cover nothing.
"""
import pytest

import _stem_partition as SP


def test_restated_arithmetic():
    # the headline: 256 images on 128 workgroups, 14 items per run, every run on an image boundary
    rs = SP.runs(256, 128)
    assert len(rs) == 128 and {r.items for r in rs} == {14} and not any(r.starts_mid_image for r in rs)
    assert all(r.crosses_boundary and r.holds_whole_image for r in rs)
    # the largest sizes the float64 oracle saw before this sweep
    assert SP.run_lengths(37, 128) == [2, 3] and SP.run_lengths(64, 256) == [1, 2]
    assert SP.grid(1, 128) == SP.grid(1, 256) == 7 and SP.grid(19, 256) == 133 and SP.grid(19, 128) == 128
    assert SP.Run(5, 9).holds_whole_image and not SP.Run(5, 8).holds_whole_image and SP.Run(7, 7).holds_whole_image
    assert SP.Run(6, 2).crosses_boundary and not SP.Run(7, 7).crosses_boundary and not SP.Run(5, 2).crosses_boundary


@pytest.mark.parametrize("G", SP.GRIDS)
def test_every_item_belongs_to_exactly_one_run(G):
    for n in SP.SIZES:
        rs = SP.runs(n, G)
        assert rs[0].first == 0 and rs[-1].first + rs[-1].items == SP.NBLK * n
        assert all(a.first + a.items == b.first for a, b in zip(rs, rs[1:]))
        assert all(r.items >= 1 for r in rs)
        for b, r in enumerate(rs):
            whole = [j for j in range(r.items) if not SP.continues(b, j, n, G)]
            assert whole[0] == 0 and all((r.first + j) % SP.NBLK == 0 for j in whole[1:])


@pytest.mark.parametrize("G", SP.GRIDS)
def test_sizes_reach_every_case(G):
    sizes = SP.SIZES
    assert sizes == sorted(set(sizes)) and max(sizes) == SP.N_MAX <= 150
    all_runs = {n: SP.runs(n, G) for n in sizes}
    lengths = {n: {r.items for r in rs} for n, rs in all_runs.items()}
    seen = set().union(*lengths.values())
    # a grid smaller than G
    assert any(SP.grid(n, G) < G for n in sizes)
    # run lengths 1, 2, 3 (every stage buffer used once) and >= 4 (the stage ring wraps)
    assert {1, 2, 3} <= seen and max(seen) > SP.NSTAGE
    if G == 128:
        assert max(seen) >= 7
        assert any(r.holds_whole_image for rs in all_runs.values() for r in rs)
    # unequal run lengths within one launch
    assert any(len(l) > 1 for l in lengths.values())
    # runs that start mid-image (halo copy after a first whole tile that is not an image's first)
    assert any(r.starts_mid_image and r.items > 1 for rs in all_runs.values() for r in rs)
    # an image boundary inside a run, after at least one item and with items to follow (a whole-tile load mid-run)
    assert any(r.crosses_boundary for rs in all_runs.values() for r in rs)
    # a size with runs of several items none of which crosses a boundary
    assert any(max(lengths[n]) > 1 and not any(r.crosses_boundary for r in all_runs[n]) for n in sizes)
    # both parities of the run length at the wrap (the last item in either tile buffer)
    assert any(l % 2 for l in seen if l > SP.NSTAGE) and any(l % 2 == 0 for l in seen if l > SP.NSTAGE)


def test_the_sweep_goes_beyond_what_was_checked_before():
    assert max(SP.run_lengths(SP.N_MAX, 128)) >= 9 and max(SP.run_lengths(SP.N_MAX, 256)) >= 5
    assert sum(r.holds_whole_image for r in SP.runs(SP.N_MAX, 128)) == 42


def test_edge_images_of_the_uint8_sweep():
    for n in SP.SIZES:
        e = SP.edge_images(n, SP.GRID_U8)
        assert len(e) == min(4, n) == len(set(e)) and e[0] == 0 and all(0 <= i < n for i in e)
        if n > 1:
            assert e[1] == n - 1
    # at the largest size the third image has a run start inside it, the fourth begins in the middle of a run
    rs = SP.runs(SP.N_MAX, SP.GRID_U8)
    e = SP.edge_images(SP.N_MAX, SP.GRID_U8)
    assert any(r.first // SP.NBLK == e[2] and r.starts_mid_image for r in rs)
    assert any(r.first < SP.NBLK * e[3] < r.first + r.items for r in rs)
