"""CPU: what surrounds the truth-table usage counters -- don't-care-aware export, the coverage report, the .npz files, the
sum across ranks and evaluate()'s refusal of a model without counters.  (The counters themselves are a device feature:
tests/test_gpu_table_usage.py.)"""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import ROOT, spec_and_state
from scale_imagenet_amd import export as E
from scale_imagenet_amd import report


def xsmall_table():
    from oracle import ttnet_bits as OB
    spec, st = spec_and_state("xsmall")
    table, _ = OB.build_lut(st, spec.blocks[0].conv1)               # [64 groups][16][1], n = 4
    return table


def read_dir(d):
    return {n: open(os.path.join(d, n)).read() for n in sorted(os.listdir(d))}


def evaluate_text(text, n):
    """Value of an expression string on every one of the 2^n patterns (x_0 = MSB)."""
    from sympy import symbols
    from sympy.parsing.sympy_parser import parse_expr
    names = {f"x_{i}": symbols(f"x_{i}") for i in range(n)}
    expr = parse_expr(text, local_dict=names)
    out = []
    for idx in range(1 << n):
        bits = {names[f"x_{i}"]: bool((idx >> (n - 1 - i)) & 1) for i in range(n)}
        out.append(bool(expr.subs(bits)))
    return np.array(out)


def non_constant_filters(table, k):
    return [f for f in range(table.shape[0]) if 0 < table[f, :, 0].sum() < table.shape[1]][:k]


def test_all_seen_usage_changes_no_expression(tmp_path):
    table = xsmall_table()
    usage = np.arange(1, table.shape[0] * 16 + 1, dtype=np.int64).reshape(table.shape[0], 16)      # every pattern seen
    filters = non_constant_filters(table, 6)
    assert len(filters) == 6
    a = E.export_block(table, str(tmp_path / "a"), 0, 0, filters=filters)
    b = E.export_block(table, str(tmp_path / "b"), 0, 0, filters=filters, usage=usage)
    fa, fb = read_dir(tmp_path / "a"), read_dir(tmp_path / "b")
    assert sorted(fa) == sorted(fb)
    for name in fa:
        if not name.endswith(".csv"):
            assert fa[name] == fb[name], name                       # DNF, CNF, table_output: the same text
    for f in filters:
        assert (a[f]["dnf"], a[f]["cnf"], a[f]["cnf_with_y"]) == (b[f]["dnf"], b[f]["cnf"], b[f]["cnf_with_y"])
        assert b[f]["dnf_literals"] == E.literal_count(b[f]["dnf"]) == a[f]["dnf_literals"] > 0


def test_unseen_patterns_are_dont_cares(tmp_path):
    table = xsmall_table()
    rng = np.random.default_rng(7)
    checked = 0
    for f in non_constant_filters(table, 8):
        col = table[f, :, 0].astype(bool)
        counts = rng.integers(1, 1000, size=16).astype(np.int64)
        counts[rng.choice(16, size=6, replace=False)] = 0
        seen = counts > 0
        if len(np.unique(col[seen])) < 2:
            continue
        usage = np.ones((table.shape[0], 16), dtype=np.int64)
        usage[f] = counts
        plain = E.export_block(table, str(tmp_path / f"p{f}"), 2, 1, filters=[f])[f]
        got = E.export_block(table, str(tmp_path / f"u{f}"), 2, 1, filters=[f], usage=usage)[f]
        for form in ("dnf", "cnf"):                                 # brute force over the 2^n patterns
            assert np.array_equal(evaluate_text(got[form], 4)[seen], col[seen]), (f, form)
            assert got[f"{form}_literals"] <= plain[f"{form}_literals"], (f, form)
            assert got[f"{form}_literals"] == E.literal_count(got[form])
        rows = list(csv.reader(open(got["csv"])))
        assert rows[0][-1] == "count" and [int(r[-1]) for r in rows[1:]] == counts.tolist()
        assert rows[0][:-1] == list(csv.reader(open(plain["csv"])))[0]          # the other columns are what they were
        assert [r[:-1] for r in rows[1:]] == list(csv.reader(open(plain["csv"])))[1:]
        checked += 1
    assert checked >= 4


def test_constant_on_seen_is_written_as_a_constant(tmp_path):
    column = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0], dtype=np.uint8)
    counts = np.where(column == 1, 5, 0).astype(np.int64)          # only patterns with output 1 were ever looked up
    out = E.export_filter(column, 4, 3, str(tmp_path), 1, 0, usage=counts)
    assert out["cnf_with_y"] == "1.0" and out["dnf"] is None and out["csv"] is None
    assert read_dir(tmp_path) == {"table_outputblock_1_filter_3_coefdefault_1.0.txt": "1.0"}
    with pytest.raises(ValueError):
        E.export_filter(column, 4, 3, str(tmp_path), 1, 0, usage=counts[:8])
    with pytest.raises(ValueError):
        E.export_block(column.reshape(1, 16, 1), str(tmp_path), 1, 0, usage=np.ones((2, 16), dtype=np.int64))


def test_coverage_numbers_on_a_hand_made_array():
    usage = {"b": np.zeros((3, 256), dtype=np.int64)}
    usage["b"][0, [0, 255]] = [90, 10]                              # group 0: two entries, 90 % on one
    usage["b"][1, :100] = 1                                          # group 1: 100 entries, uniform
    tables = {"b": np.zeros((3, 256, 2), dtype=np.uint8)}           # group 2: never looked up
    tables["b"][0, 255, 1] = 1                                       # group 0 varies on what it saw
    tables["b"][1, 100:, 0] = 1                                      # group 1 varies only on unseen entries
    head, row = report.coverage_rows(usage, tables)
    assert head == ["block", "groups", "inputs", "entries", "seen", "share_seen", "constant_groups", "top1pct_share"]
    assert row[:5] == ["b", 3, 8, 768, 102]
    assert float(row[5]) == 102 / 768
    assert row[6] == 2                                               # groups 1 and 2
    assert float(row[7]) == (90 + 10 + 2) / 200                     # 1 % of 256 entries = the 2 most used per group
    assert report.coverage_rows(usage)[1][6] == ""                  # no tables: the column stays empty


def test_npz_round_trip_and_coverage_file(tmp_path):
    rng = np.random.default_rng(1)
    usage = {"features.4.Block_conv1": rng.integers(0, 2 ** 40, size=(4, 16)).astype(np.int64),
             "features.4.Block_convf": rng.integers(0, 9, size=(2, 65536)).astype(np.int64)}
    path = str(tmp_path / "u.npz")
    report.save_table_usage(path, usage)
    back = report.load_table_usage(path)
    assert list(back) == list(usage)
    for k in usage:
        assert back[k].dtype == np.int64 and np.array_equal(back[k], usage[k])
    assert os.listdir(tmp_path) == ["u.npz"]                        # (no temporary file left)
    report.write_coverage_csv(str(tmp_path / "c.csv"), usage)
    rows = list(csv.reader(open(tmp_path / "c.csv")))
    assert [r[0] for r in rows] == ["block"] + list(usage) and rows[2][3] == str(2 * 65536)


_WORKER = r'''
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch.distributed as dist
from scale_imagenet_amd.dist import init_from_env, all_reduce_table_usage
rank, world, _ = init_from_env("gloo")
rng = np.random.default_rng(rank)
mine = {{"b.conv1": rng.integers(0, 2 ** 40, size=(3, 16)).astype(np.int64), "a.convf": rng.integers(0, 5, size=(2, 256)).astype(np.int64)}}
total = all_reduce_table_usage(mine)
assert list(total) == list(mine)
np.savez({out!r} + str(rank) + ".npz", **total)
dist.barrier()
dist.destroy_process_group()
'''


def test_all_reduce_table_usage_two_ranks_gloo(tmp_path):
    out = str(tmp_path / "sum")
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29655", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    parts = [{"b.conv1": np.random.default_rng(r).integers(0, 2 ** 40, size=(3, 16)).astype(np.int64)} for r in range(2)]
    for r in range(2):
        got = report.load_table_usage(out + f"{r}.npz")
        assert got["b.conv1"].dtype == np.int64
        assert np.array_equal(got["b.conv1"], parts[0]["b.conv1"] + parts[1]["b.conv1"])      # exact beyond 2^32
        assert got["a.convf"].shape == (2, 256) and got["a.convf"].sum() > 0
    from scale_imagenet_amd.dist import all_reduce_table_usage
    assert all_reduce_table_usage(parts[0]) is parts[0]             # a single process returns its input


def test_evaluate_refuses_a_model_without_counters():
    from scale_imagenet_amd.evaluate import evaluate

    class Stub(torch.nn.Module):
        def forward(self, x):
            return torch.zeros((x.shape[0], 10))

    batches = [(torch.zeros((2, 3, 4, 4)), torch.zeros(2, dtype=torch.int64))]
    with pytest.raises(RuntimeError, match="table_usage.*Stub.*count_table_usage"):
        evaluate(Stub(), batches, torch.device("cpu"), table_usage=True)
    res = evaluate(Stub(), batches, torch.device("cpu"))
    assert res.table_usage is None and res.images == 2


def test_main_flags():
    from scale_imagenet_amd.main import build_parser, main
    args = build_parser().parse_args(["--table_usage", "u.npz", "--table_coverage", "c.csv"])
    assert (args.table_usage, args.table_coverage) == ("u.npz", "c.csv")
    assert build_parser().parse_args([]).table_usage is None
    with pytest.raises(SystemExit, match="--table_coverage needs --table_usage"):
        main(["--table_coverage", "c.csv"])
