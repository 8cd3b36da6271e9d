"""CPU: the definitions of rule support (``scale_imagenet_amd.rules``) on the numpy twin -- against a brute-force triple loop
over functions, cubes and patterns, the identities that hold for every cover, the edges of ``keep_by_support``,
``care_after_prune`` against an explicit loop, the report's rows and the command line's flags."""
import numpy as np
import pytest

from _minimise_util import random_functions
from scale_imagenet_amd import minimise as M, report, rules as R


def brute_force(covers, usage, rows, n, keep=None):
    """The definitions of include/ttnet.h, one test per (function, cube, pattern)."""
    size = 1 << n
    out = dict(hits=[], first=[], sole=[], totals=np.zeros((len(covers), 4), dtype=np.int64),
               lost=np.zeros((len(covers), size), dtype=bool))
    for f, keys in enumerate(covers):
        kept = [True] * len(keys) if keep is None else [bool(k) for k in keep[f]]
        hits, first, sole = ([0] * len(keys) for _ in range(3))
        u = usage[rows[f]]
        for p in range(size):
            holders = [c for c, key in enumerate(keys) if p & (int(key) >> 16) == int(key) & 0xFFFF]
            mine = [c for c in holders if kept[c]]
            for c in mine:
                hits[c] += int(u[p])
            if mine:
                first[mine[0]] += int(u[p])
                out["totals"][f, 0] += u[p]
                if len(mine) == 1:
                    sole[mine[0]] += int(u[p])
            elif holders:
                out["totals"][f, 1] += u[p]
                out["totals"][f, 3] += 1
                out["lost"][f, p] = True
            out["totals"][f, 2] += u[p] > 0
        for key, v in (("hits", hits), ("first", first), ("sole", sole)):
            out[key].append(np.array(v, dtype=np.int64))
    return out


def assert_matches(got, want, n, tag):
    for key in ("hits", "first", "sole"):
        for f, (a, b) in enumerate(zip(got[key], want[key])):
            assert np.array_equal(a, b), f"{tag}: {key} of function {f}: {a.tolist()} against {b.tolist()}"
    assert np.array_equal(got["totals"], want["totals"]), tag
    assert np.array_equal(M.unpack_bits(got["lost_bits"], n), want["lost"]), tag


def usage_rows(seed, rows, n, high=50):
    rng = np.random.default_rng(seed)
    u = rng.integers(1, high, size=(rows, 1 << n), dtype=np.int64)
    u[rng.random(u.shape) < 0.4] = 0
    return u


def keep_flags(seed, covers, share=0.6):
    rng = np.random.default_rng(seed)
    return [rng.random(len(c)) < share for c in covers]


def all_functions(n):
    flags = (np.arange(1 << (1 << n))[:, None] >> np.arange(1 << n)[None, :]) & 1
    return M.pack_bits(flags.astype(bool))


def test_twin_against_brute_force_every_function_of_three_inputs():
    n = 3
    on = all_functions(n)
    covers = [M.minimise_cpu(o, None, n) for o in on]
    rows = np.arange(len(covers)) % 4
    usage = usage_rows(3, 4, n)
    for keep in (None, keep_flags(3, covers)):
        got = R.cover_support_cpu(covers, usage, rows, n, keep, lost_bits=True)
        assert_matches(got, brute_force(covers, usage, rows, n, keep), n, "n=3")
    assert got["bad_rows"] == 0 and got["n"] == n


def test_twin_against_brute_force_random_functions_of_six_inputs():
    n = 6
    on, dc = random_functions(606, n, 12)
    covers = [M.minimise_cpu(on[i], dc[i], n, rounds=i % 3) for i in range(len(on))]
    rows = np.arange(len(covers)) // 4
    usage = usage_rows(6, 3, n, high=1 << 40)
    for keep in (None, keep_flags(6, covers), keep_flags(7, covers, share=0.2)):
        got = R.cover_support_cpu(covers, usage, rows, n, keep, lost_bits=True)
        assert_matches(got, brute_force(covers, usage, rows, n, keep), n, "n=6")


def test_identities():
    n = 6
    on, dc = random_functions(616, n, 10)
    covers = [M.minimise_cpu(on[i], dc[i], n) for i in range(len(on))]
    rows = np.arange(len(covers)) // 2
    usage = usage_rows(61, 5, n)
    full = R.cover_support_cpu(covers, usage, rows, n)
    for keep in (None, keep_flags(61, covers)):
        res = R.cover_support_cpu(covers, usage, rows, n, keep, lost_bits=True)
        for f, keys in enumerate(covers):
            kept = np.ones(len(keys), bool) if keep is None else keep[f]
            u = usage[rows[f]]
            covered, lost = (int(v) for v in res["totals"][f, :2])
            assert int(res["first"][f].sum()) == covered
            assert (res["sole"][f] <= res["first"][f]).all() and (res["first"][f] <= res["hits"][f]).all()
            holders = np.zeros(1 << n, dtype=np.int64)                   # kept cubes holding each pattern
            for c, pts in enumerate(M.cube_patterns(keys, n)):
                holders[pts] += kept[c]
            assert int(res["hits"][f].sum()) == int((u * holders).sum())
            assert covered + lost == int(full["totals"][f, 0])           # the mass under the full list
            assert not res["hits"][f][~kept].any() and not res["first"][f][~kept].any() and not res["sole"][f][~kept].any()
            assert res["totals"][f, 2] == np.count_nonzero(u)
            assert res["row_total"][f] == u.sum()


def test_a_row_index_out_of_range_gives_zeros_and_is_counted():
    n = 4
    on, dc = random_functions(40, n, 4)
    covers = [M.minimise_cpu(on[i], dc[i], n) for i in range(4)]
    res = R.cover_support_cpu(covers, usage_rows(4, 2, n), [0, 2, -1, 1], n, lost_bits=True)
    assert res["bad_rows"] == 2
    for f in (1, 2):
        assert not res["totals"][f].any() and not res["hits"][f].any() and res["row_total"][f] == 0 and not res["lost_bits"][f].any()
    with pytest.raises(ValueError):
        R.cover_support_cpu(covers, usage_rows(4, 2, n), [0, 1, 1], n)
    with pytest.raises(ValueError):
        R.cover_support_cpu(covers, usage_rows(4, 2, n + 1), [0, 1, 1, 0], n)
    with pytest.raises(ValueError, match="malformed"):
        R.cover_support_cpu([np.array([0x00010003], dtype=np.uint32)], usage_rows(4, 1, n), [0], n)


def test_keep_by_support_edges():
    n = 6
    on, dc = random_functions(626, n, 6)
    covers = [M.minimise_cpu(on[i], dc[i], n) for i in range(len(on))]
    rows = [0, 0, 1, 1, 2, 2]
    usage = usage_rows(62, 3, n)
    usage[2] = 0                                                     # a row without a lookup: every share is 0
    full = R.cover_support_cpu(covers, usage, rows, n)
    every = R.keep_by_support(full, min_share=0.0)
    assert all(k.all() for k in every)
    none = R.keep_by_support(full, min_share=1.0000001)
    assert not any(k.any() for k in none)
    res = R.cover_support_cpu(covers, usage, rows, n, none, lost_bits=True)
    assert np.array_equal(res["totals"][:, 1], full["totals"][:, 0]) and not res["totals"][:, 0].any()
    for f, keys in enumerate(covers):
        union = np.zeros(1 << n, dtype=bool)
        for pts in M.cube_patterns(keys, n):
            union[pts] = True
        assert np.array_equal(M.unpack_bits(res["lost_bits"][f], n), union)
        assert res["totals"][f, 3] == union.sum()
    some = R.keep_by_support(full, min_share=0.05)
    for f in range(4):
        assert np.array_equal(some[f], full["hits"][f] / usage[rows[f]].sum() >= 0.05)
    assert not some[4].any() and not some[5].any() and every[4].all()
    by_hits = R.keep_by_support(full, min_hits=30)
    assert all(np.array_equal(k, h >= 30) for k, h in zip(by_hits, full["hits"]))
    both = R.keep_by_support(full, min_hits=30, min_share=0.05)
    assert all(np.array_equal(k, a & b) for k, a, b in zip(both, by_hits, some))
    with pytest.raises(ValueError):
        R.keep_by_support(full)
    with pytest.raises(ValueError):
        R.keep_by_support(full, min_share=-0.1)


@pytest.mark.parametrize("n", [3, 5, 7])
def test_care_after_prune_against_an_explicit_loop(n):
    groups, per = 3, 4
    rng = np.random.default_rng(n)
    lost = rng.random((groups * per, 1 << n)) < 0.1
    base = rng.random((groups, 1 << n)) < 0.7
    want = np.ones((groups, 1 << n), dtype=bool)
    for f in range(groups * per):
        for p in range(1 << n):
            if lost[f, p]:
                want[f // per, p] = False
    got = R.care_after_prune(M.pack_bits(lost), groups, per, n=n)
    assert got.dtype == np.uint32 and got.shape == (groups, M.n_words(n))
    assert np.array_equal(M.unpack_bits(got, n), want)
    assert np.array_equal(got, M.pack_bits(want)), "unused high bits must be zero"
    with_base = R.care_after_prune(M.pack_bits(lost), groups, per, M.pack_bits(base))
    assert np.array_equal(with_base, M.pack_bits(want & base))
    with pytest.raises(ValueError):
        R.care_after_prune(M.pack_bits(lost), groups + 1, per, n=n)
    with pytest.raises(ValueError):
        R.care_after_prune(M.pack_bits(lost), groups, per, M.pack_bits(base)[:2])
    if n < 5:
        with pytest.raises(ValueError, match="pass n"):
            R.care_after_prune(M.pack_bits(lost), groups, per)


def test_report_rows():
    n = 6
    on, dc = random_functions(636, n, 4)
    covers = [M.minimise_cpu(on[i], dc[i], n) for i in range(4)]
    usage, rows = usage_rows(63, 2, n), [0, 0, 1, 1]
    block = R.cover_support_cpu(covers, usage, rows, n)
    block.update(cubes=covers, form="dnf")
    keep = R.keep_by_support(block, min_share=0.1)
    pruned = R.cover_support_cpu(covers, usage, rows, n, keep, lost_bits=True)
    pruned["keep"] = keep
    head, row = report.rule_support_rows({"b": block})
    assert head == report.RULE_FIELDS and len(row) == len(head)
    first = np.sort(np.concatenate(block["first"]))[::-1]
    assert row[:6] == ["b", n, "dnf", 4, sum(len(c) for c in covers), sum(M.literal_total(c) for c in covers)]
    assert float(row[6]) == first[: max(1, len(first) // 100)].sum() / first.sum()
    assert float(row[7]) == first[: len(first) // 10].sum() / first.sum() and float(row[6]) <= float(row[7]) <= 1.0
    assert row[8] == sum(int((h == 0).sum()) for h in block["hits"])
    head, row = report.rule_support_rows({"b": block}, {"b": pruned})
    assert head == report.RULE_FIELDS + report.RULE_PRUNED_FIELDS
    assert row[9] == sum(int(k.sum()) for k in keep) and row[10] == sum(M.literal_total(c[k]) for c, k in zip(covers, keep))
    assert float(row[11]) == pruned["totals"][:, 1].sum() / (2 * usage.sum()) and row[12] == pruned["totals"][:, 3].sum()


def test_command_line_flags_and_refusals():
    from scale_imagenet_amd import main as cli
    parser = cli.build_parser()
    a = parser.parse_args([])
    assert a.rule_support is None and a.rule_form is None and a.rule_min_share is None
    a = parser.parse_args(["--table_usage", "u.npz", "--rule_support", "r.csv", "--rule_form", "cnf", "--rule_min_share", "0.001",
                           "--table_gates_rounds", "2"])
    assert (a.rule_support, a.rule_form, a.rule_min_share, a.table_gates_rounds) == ("r.csv", "cnf", 0.001, 2)
    cli.check_rule_flags(a)
    with pytest.raises(SystemExit):
        parser.parse_args(["--rule_form", "sop"])
    for argv, text in ((["--rule_form", "cnf"], "--rule_form needs --rule_support"),
                       (["--rule_min_share", "0.1"], "--rule_min_share needs --rule_support"),
                       (["--rule_support", "r.csv"], "--rule_support needs --table_usage or --care_from"),
                       (["--rule_support", "r.csv", "--table_usage", "u.npz", "--rule_min_share", "-1"], "--rule_min_share must be"),
                       (["--table_gates_rounds", "2"], "--table_gates_rounds needs --table_gates or --rule_support")):
        with pytest.raises(SystemExit, match=text):
            cli.main(argv)
