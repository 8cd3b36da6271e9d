"""CPU: the case lists of tests/_resize_paths.py reach every path of csrc/preproc.hip (asserted from the twins of the two
launchers alone), and the numpy oracle equals Pillow's hashes of every case (tests/golden/ref_resize_paths.json, written
by tools/gen_resize_paths_fixture.py) and, where Pillow imports, Pillow itself."""
import numpy as np
import pytest

import _resize_paths as RP
from _util import oracle_views, sha
from oracle import pil_resize as PR
from scale_imagenet_amd import preprocess


def test_uniform_cases_reach_every_path():
    plans = {c.key: c.plan() for c in RP.UNIFORM_CASES}
    assert all(p.accepted for p in plans.values())
    insts = {p.inst for p in plans.values()}
    assert insts == {0, 1, 3, 5, 7, 9}, insts
    zero = [p for p in plans.values() if p.inst == 0]
    assert any(p.ksh == p.ksv and p.ksh > 9 for p in zero), "<0,0> by a count above 9"
    assert any(p.ksh > p.ksv for p in zero) and any(p.ksh < p.ksv for p in zero), "<0,0> by unequal counts, both ways"
    for c in RP.UNIFORM_CASES:                              # the instantiation the case's name promises
        want = {"u1": 1, "u7": 7, "u9": 9, "u11": 0, "u17": 0, "umix": 0, "urows": 7, "ubig": 0}.get(c.case)
        assert want is None or c.plan().inst == want, c.key
    assert sum(p.partial_piece for p in plans.values()) >= 2, "the buffer's last partial piece"
    assert any(p.partial_piece and c.n > 1 for c, p in zip(RP.UNIFORM_CASES, plans.values()))
    assert any(p.chunk < RP.RS_CHUNK for p in plans.values()), "a chunk below 16 rows"
    assert {p.last_tile_rows for p in plans.values()} >= {4, 8, 16}, "last tiles shorter than 16 rows"
    assert any(p.inst == 7 and p.last_tile_rows == 4 for p in plans.values())
    assert any(c.n > 1 and (c.h * c.w * 3) % 16 for c in RP.UNIFORM_CASES), "an image that starts off a 16-byte boundary"
    assert len({(c.resize, c.crop) for c in RP.UNIFORM_CASES}) >= 5


def test_uniform_lds_bound_from_both_sides():
    """include/ttnet.h: 2592 x 3888 is accepted, 2848 x 4288 is not (resize 256 / crop 224; the bound is 160 KiB of LDS)."""
    big = [c for c in RP.UNIFORM_CASES if c.case == "ubig"]
    assert [(c.h, c.w) for c in big] == [(2592, 3888)]
    p = big[0].plan()
    assert p.accepted and p.lds == 159216 <= RP.LDS_LIMIT and p.chunk == 3 and (p.ksh, p.ksv) == (23, 23)
    refused = {(c.h, c.w): c.plan() for c in RP.UNIFORM_REFUSED}
    assert sorted(refused) == [(2700, 4050), (2848, 4288)]
    assert not any(p.accepted for p in refused.values())
    assert [refused[k].lds for k in sorted(refused)] == [165456, 175248]
    assert min(p.lds for p in refused.values()) - RP.LDS_LIMIT < 2000          # the nearer one misses by under 2 KB


def test_ragged_pairs_reach_every_path():
    plans = {}
    for resize, crop in RP.RAGGED_PAIRS:
        sizes = RP.ragged_sizes(resize)
        plans[(resize, crop)] = p = RP.ragged_center_plan(max(s[0] for s in sizes), max(s[1] for s in sizes), resize, crop)
        assert p.accepted and p.items <= RP.RG_ITEMS
        assert [RP.taps(h, w, resize) for h, w in sizes] == [(3, 3), (5, 5), (7, 7), (5, 7), (1, 1)], (resize, sizes)
        assert all(min(PR.resized_size(h, w, resize)) >= crop for h, w in sizes)
        assert sum(h * w * 3 for h, w in sizes) % 16 != 0, "the last image ends an unaligned buffer"
    assert not plans[(360, 340)].wide and plans[(360, 340)].owq == 255           # the last crop that is not WIDE
    p = plans[(360, 344)]                                                         # the first that is
    assert p.wide and (p.owq, p.ncol, p.ty, p.last_col_threads) == (258, 2, 8, 2)
    assert all(plans[k].wide and (plans[k].ncol, plans[k].ty) == (2, 8) for k in [(438, 384), (512, 448)])
    p = plans[(730, 684)]
    assert p.wide and (p.ncol, p.ty, p.items, p.last_tile_rows, p.last_col_threads) == (3, 5, 15, 4, 1)
    assert {p.ncol for p in plans.values() if p.wide} == {2, 3}
    assert any(p.last_tile_rows < p.ty for p in plans.values() if p.wide), "rows_out < ty under WIDE"
    assert any(p.last_tile_rows < p.ty for p in plans.values() if not p.wide and p.tiles > 1)
    assert any(p.last_col_threads < RP.RG_THREADS for p in plans.values() if p.wide), "a partly filled last column"
    assert set(RP.VIEW_PAIRS) <= set(RP.RAGGED_PAIRS) and all(plans[k].wide for k in RP.VIEW_PAIRS)
    assert {plans[k].ncol for k in RP.VIEW_PAIRS} == {2, 3}


def test_view_boxes_are_valid_and_end_on_the_last_byte():
    for resize, crop in RP.VIEW_PAIRS:
        sizes = RP.ragged_sizes(resize)
        boxes = RP.view_boxes(resize, crop)
        views = preprocess.make_views(boxes, sizes, crop)                       # raises on an invalid record
        p = RP.ragged_plan(crop, views.max_scale)
        assert p.accepted and p.wide
        image, flags, bx, by, bw, bh, nw, nh, x0, y0 = boxes[0]
        assert image == len(sizes) - 1 and (by + bh, bx + bw) == sizes[-1] and (x0 + crop, y0 + crop) == (nw, nh)
        assert any(d[1] & 1 for d in boxes) and any(not d[1] & 1 for d in boxes)
        assert any(d[4] == d[6] for d in boxes) and any(d[5] == d[7] for d in boxes)      # a skipped pass on either axis
        # the ten-crop family's bottom-right window of the last image (no resampling) holds its last pixel too
        rec = preprocess.eval_views_host(sizes[-1:], "ten", resize, crop).records()
        assert any(d[8] + crop == d[6] == sizes[-1][1] and d[9] + crop == d[7] == sizes[-1][0] for d in rec)


def test_ragged_bound_from_both_sides():
    """launch_ragged at resize 256 / crop 224, max_h = max_w = m.  A staged row must fit the 6 x 256 pieces a workgroup
    stages: with smax = m / 255, cw_max = ceil(225 * smax) + 4 and row_q_max = (3 * cw_max + 30) // 16 <= 1536, i.e.
    3 * cw_max + 30 <= 24591, cw_max <= 8187, ceil(225 * m / 255) <= 8183, m <= 8183 * 255 / 225 = 9274.07: 9274 is
    accepted and 9275 is refused (the LDS, about 110 KB there, is not the binding bound)."""
    m = RP.largest_accepted_side(256, 224)
    assert m == (8183 * 255) // 225 == 9274
    ok, no = RP.ragged_center_plan(m, m, 256, 224), RP.ragged_center_plan(m + 1, m + 1, 256, 224)
    assert ok.accepted and ok.row_q_max == RP.RG_STAGE_Q and ok.lds <= RP.LDS_LIMIT
    assert not no.accepted and no.row_q_max == RP.RG_STAGE_Q + 1 and no.lds <= RP.LDS_LIMIT
    assert RP.ragged_center_plan(8192, 8192, 256, 224).accepted          # preprocess.MAX_SIDE
    assert preprocess.MAX_SIDE <= m


def _fixture_uniform():
    return {(e["case"], e["h"], e["w"], e["resize"], e["crop"], e["n"]): e for e in RP.fixture()["uniform"]}


@pytest.mark.parametrize("c", RP.UNIFORM_CASES + RP.UNIFORM_REFUSED, ids=lambda c: c.key)
def test_oracle_equals_the_pillow_fixture_uniform(c):
    e = _fixture_uniform()[tuple(c)]
    assert e["seed"] == c.seed
    assert [sha(a) for a in RP.uniform_oracle(c)] == e["sha256"]


def test_fixture_lists_the_cases_in_order():
    fx = RP.fixture()
    assert [(e["case"], e["h"], e["w"], e["resize"], e["crop"], e["n"]) for e in fx["uniform"]] == \
        [tuple(c) for c in RP.UNIFORM_CASES + RP.UNIFORM_REFUSED]
    assert [(e["resize"], e["crop"]) for e in fx["ragged"]] == RP.RAGGED_PAIRS
    assert [(e["resize"], e["crop"]) for e in fx["views"]] == RP.VIEW_PAIRS
    for e in fx["ragged"]:
        assert [(i["h"], i["w"]) for i in e["images"]] == RP.ragged_sizes(e["resize"])
        assert [i["seed"] for i in e["images"]] == [RP.ragged_seed(e["resize"], k) for k in range(len(e["images"]))]
    for e in fx["views"]:
        assert [tuple(d) for d in e["boxes"]["desc"]] == RP.view_boxes(e["resize"], e["crop"])
        assert len(e["ten"]) == 10 * len(RP.ragged_sizes(e["resize"]))


@pytest.mark.parametrize("resize,crop", RP.RAGGED_PAIRS)
def test_oracle_equals_the_pillow_fixture_ragged(resize, crop):
    e = [e for e in RP.fixture()["ragged"] if (e["resize"], e["crop"]) == (resize, crop)][0]
    assert [sha(a) for a in RP.ragged_oracle(resize, crop)] == [i["sha256"] for i in e["images"]]


@pytest.mark.parametrize("resize,crop", RP.VIEW_PAIRS)
def test_oracle_equals_the_pillow_fixture_views(resize, crop):
    e = [e for e in RP.fixture()["views"] if (e["resize"], e["crop"]) == (resize, crop)][0]
    ims = RP.ragged_images(resize)
    got = []
    for x in ims:
        got += [sha(a) for a in oracle_views(x, preprocess.eval_views_host([x.shape[:2]], "ten", resize, crop).records(), crop)]
    assert got == e["ten"]
    boxes = e["boxes"]["desc"]
    assert [sha(oracle_views(ims[d[0]], [d], crop)[0]) for d in boxes] == e["boxes"]["sha256"]


@pytest.mark.parametrize("c", [c for c in RP.UNIFORM_CASES if c.case != "ubig"], ids=lambda c: c.key)
def test_oracle_equals_pillow_directly(c):
    Image = pytest.importorskip("PIL.Image")
    nh, nw = PR.resized_size(c.h, c.w, c.resize)
    top, left = int(round((nh - c.crop) / 2.0)), int(round((nw - c.crop) / 2.0))
    for x, want in zip(c.images(), RP.uniform_oracle(c)):
        im = Image.fromarray(np.asarray(x))
        if (nh, nw) != (c.h, c.w):
            im = im.resize((nw, nh), Image.BILINEAR)
        assert np.array_equal(np.asarray(im)[top:top + c.crop, left:left + c.crop], want)
