"""CPU: what surrounds the care-set misses -- the bitmaps of ``minimise.care_masks`` against the don't-cares of
``pack_functions``, the accuracy bracket, the two CSV files, ``evaluate(care=)`` on a stub model, the gather across
ranks and the flags of ``main``.  (The misses themselves are a device feature: tests/test_gpu_table_care.py.)"""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import ROOT
from scale_imagenet_amd import minimise, report
from scale_imagenet_amd.evaluate import CareResult, care_bounds, evaluate


@pytest.mark.parametrize("n,groups,cout_g", [(4, 5, 3), (16, 2, 2)])
def test_care_masks_complement_pack_functions_dc(n, groups, cout_g):
    rng = np.random.default_rng(n)
    size = 1 << n
    table = rng.integers(0, 2, size=(groups, size, cout_g)).astype(np.uint8)
    usage = rng.integers(0, 3, size=(groups, size)).astype(np.int64) * rng.integers(0, 2, size=(groups, size))
    assert (usage == 0).any() and (usage > 0).any()
    masks = minimise.care_masks({"b": usage})
    m = masks["b"]
    words = max(1, size // 32)
    assert list(masks) == ["b"] and m.dtype == np.uint32 and m.shape == (groups, words)
    valid = np.uint32(0xFFFFFFFF if n >= 5 else (1 << size) - 1)
    assert not (m & ~valid).any()                                    # unused high bits are zero (n = 4: 16 of 32)
    _, dc = minimise.pack_functions(table, usage)
    assert dc.shape == (groups * cout_g, words)
    assert np.array_equal(dc[::cout_g], ~m & valid)                  # dc before its repeat over cout_g = the complement
    assert np.array_equal(dc, np.repeat(~m & valid, cout_g, axis=0))
    assert np.array_equal(minimise.unpack_bits(m, n), usage >= 1)
    for t in (2, 3):                                                 # the same set through both, at every threshold
        _, dct = minimise.pack_functions(table, usage, t)
        assert np.array_equal(dct[::cout_g], ~minimise.care_masks({"b": usage}, t)["b"] & valid)


def test_care_masks_thresholds_on_a_hand_made_array():
    usage = np.array([[0, 1, 2, 3, 0, 5, 1, 2, 3, 0, 0, 1, 9, 2, 3, 1],
                      [3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 2]], dtype=np.int64)
    assert minimise.care_masks({"x": usage})["x"].tolist() == [[0b1111100111101110], [0xFFFF]]
    assert minimise.care_masks({"x": usage}, 2)["x"].tolist() == [[0b0111000110101100], [0xFFFF]]
    assert minimise.care_masks({"x": usage}, 3)["x"].tolist() == [[0b0101000100101000], [0x7FFF]]
    assert minimise.care_masks({"x": usage}, 10)["x"].tolist() == [[0], [0]]


def test_care_masks_shape_and_threshold_errors():
    with pytest.raises(ValueError, match="shape"):
        minimise.care_masks({"x": np.zeros(16, dtype=np.int64)})
    with pytest.raises(ValueError, match="shape"):
        minimise.care_masks({"x": np.zeros((2, 12), dtype=np.int64)})
    with pytest.raises(ValueError, match="min_count"):
        minimise.care_masks({"x": np.zeros((2, 16), dtype=np.int64)}, 0)
    with pytest.raises(ValueError, match="shape"):
        minimise.pack_functions(np.zeros((2, 16, 1), dtype=np.uint8), np.zeros((3, 16), dtype=np.int64), 2)


def test_min_count_default_gives_the_bytes_of_today():
    rng = np.random.default_rng(2)
    table = rng.integers(0, 2, size=(3, 256, 2)).astype(np.uint8)
    usage = rng.integers(0, 4, size=(3, 256)).astype(np.int64)
    on, dc = minimise.pack_functions(table, usage)
    on1, dc1 = minimise.pack_functions(table, usage, 1)
    col = np.transpose(table != 0, (0, 2, 1)).reshape(6, 256)        # the rule as it was: count 0 = don't-care
    unseen = np.repeat(usage == 0, 2, axis=0)
    assert on.tobytes() == on1.tobytes() == minimise.pack_bits(col & ~unseen).tobytes()
    assert dc.tobytes() == dc1.tobytes() == minimise.pack_bits(unseen).tobytes()
    on2, dc2 = minimise.pack_functions(table, usage, 2)
    assert not (on2 & dc2).any() and (dc2 & dc).tobytes() == dc.tobytes() and dc2.tobytes() != dc.tobytes()
    # gate counts on the CPU twin: the default is the old call, a higher threshold never needs more literals here
    rows = [minimise.gate_count_row(*minimise.pack_functions(table, usage, t), 8, "cpu", None, 0) for t in (1, 2)]
    old = minimise.gate_count_row(on, dc, 8, "cpu", None, 0)
    assert rows[0] == old


def test_export_block_min_count(tmp_path):
    from scale_imagenet_amd import export as E
    rng = np.random.default_rng(5)
    table = rng.integers(0, 2, size=(2, 16, 1)).astype(np.uint8)
    usage = rng.integers(1, 4, size=(2, 16)).astype(np.int64)
    a = E.export_block(table, str(tmp_path / "a"), 0, 0, usage=usage, minimiser="cpu")
    b = E.export_block(table, str(tmp_path / "b"), 0, 0, usage=usage, minimiser="cpu", min_count=1)
    assert a == {f: {k: (v.replace("/b/", "/a/") if isinstance(v, str) else v) for k, v in r.items()} for f, r in b.items()}
    c = E.export_block(table, str(tmp_path / "c"), 0, 0, usage=usage, minimiser="cpu", min_count=3)
    d = E.export_block(table, str(tmp_path / "d"), 0, 0, usage=np.where(usage >= 3, usage, 0), minimiser="cpu")
    for f in c:
        assert (c[f]["dnf"], c[f]["cnf"]) == (d[f]["dnf"], d[f]["cnf"])


def test_bounds_arithmetic():
    rows = np.array([[0, 0, 0], [0, 2, 0], [0, 0, 0], [1, 0, 7], [0, 0, 0], [0, 0, 0]], dtype=np.int32)
    hits = np.array([[1, 1], [1, 1], [0, 1], [0, 0], [0, 0], [1, 1]], dtype=bool)
    care = CareResult(["a", "b", "c"], rows, hits)
    assert care.covered.tolist() == [True, False, True, False, True, True] and care.covered_images == 4
    assert dict(care.images_with_misses) == {"a": 1, "b": 1, "c": 1} and dict(care.misses) == {"a": 1, "b": 2, "c": 7}
    assert care.top1_bounds == (100.0 * 2 / 6, 100.0 * 4 / 6)       # h = 2 covered hits, N - C = 2 may go either way
    assert care.top5_bounds == (100.0 * 3 / 6, 100.0 * 5 / 6)
    assert care.line() == "Care.. 4/6 top1 [33.333, 66.667] top5 [50.000, 83.333]"
    none = CareResult(["a"], np.ones((4, 1), dtype=np.int32), np.array([[1, 1]] * 4, dtype=bool))
    assert none.covered_images == 0 and none.top1_bounds == (0.0, 100.0)            # nothing covered: no statement
    every = CareResult(["a"], np.zeros((4, 1), dtype=np.int32), np.array([[1, 1], [0, 1], [0, 0], [1, 1]], dtype=bool))
    assert every.top1_bounds == (50.0, 50.0) and every.top5_bounds == (75.0, 75.0)  # all covered: the network's accuracy
    assert care_bounds(np.zeros(0, dtype=bool), np.zeros(0, dtype=bool)) == (0.0, 0.0)
    unlabelled = CareResult(["a"], rows[:, :1].copy())
    assert unlabelled.top1_bounds is None and unlabelled.line() == "Care.. 5/6"
    with pytest.raises(ValueError):
        care_bounds(np.zeros(3, dtype=bool), np.zeros(4, dtype=bool))


def test_csv_writers_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    rows = (rng.integers(0, 50, size=(9, 4)) * rng.integers(0, 2, size=(9, 1))).astype(np.int32)
    care = CareResult(["f.4.conv1", "f.4.conv2", "f.4.conv3", "f.4.convf"], rows)
    path = str(tmp_path / "r.csv")
    report.write_care_rows_csv(path, care)
    text = list(csv.reader(open(path)))
    assert text[0] == ["index", "covered"] + care.blocks and len(text) == 10
    blocks, covered, back = report.read_care_rows_csv(path)
    assert blocks == care.blocks and back.dtype == np.int32 and np.array_equal(back, rows)
    assert np.array_equal(covered, ~(rows != 0).any(axis=1)) and 0 < covered.sum() < 9
    lookups = {"f.4.conv1": 100, "f.4.conv2": 90, "f.4.conv3": 10, "f.4.convf": 4}
    summary = report.care_summary_rows(care, lookups)
    assert summary[0] == ["block", "lookups", "misses", "images_with_misses"]
    assert summary[1] == ["f.4.conv1", 900, int(rows[:, 0].sum()), int((rows[:, 0] != 0).sum())]
    assert summary[-1] == ["total", 9 * 204, int(rows.sum()), int(9 - covered.sum())]
    report.write_care_summary_csv(str(tmp_path / "s.csv"), care, lookups)
    assert list(csv.reader(open(tmp_path / "s.csv"))) == [[str(v) for v in r] for r in summary]
    assert sorted(os.listdir(tmp_path)) == ["r.csv", "s.csv"]       # (no temporary file left)


class CareStub(torch.nn.Module):
    """Logits and care rows keyed to the image index, which every image carries in its first pixel."""
    care_blocks = ["a", "b", "c"]

    def __init__(self):
        super().__init__()
        self.installed = None

    def forward(self, x):
        self.index = x[:, 0, 0, 0].to(torch.int64)
        return torch.nn.functional.one_hot(self.index % 7, 10).float() * 3 + torch.arange(10).float() * 0.01

    def set_care(self, care, min_count=1):
        self.installed = (care, min_count)

    def care_misses(self, lane=0):
        i = self.index.to(torch.int32)
        return torch.stack([i * (i % 3 == 0), i * 0, (i + 1) * (i % 4 == 1)], dim=1).to(torch.int32)


def stub_batches(sizes):
    out, first = [], 0
    for n in sizes:
        idx = torch.arange(first, first + n)
        out.append((idx.float().reshape(n, 1, 1, 1).expand(n, 3, 2, 2).contiguous(), (idx % 5).to(torch.int64)))
        first += n
    return out


def test_evaluate_care_on_a_stub_rows_in_dataset_order(capsys):
    m = CareStub()
    batches = stub_batches((4, 4, 4, 3))
    plain = evaluate(CareStub(), batches, torch.device("cpu"), inflight=2)
    assert plain.care is None and plain.predictions is None
    out0 = capsys.readouterr().out
    res = evaluate(m, batches, torch.device("cpu"), inflight=2, care={"a": "masks"}, care_min_count=2)
    assert m.installed == ({"a": "masks"}, 2)
    assert (res.loss, res.top1, res.top5, res.images) == (plain.loss, plain.top1, plain.top5, 15)
    assert res.predictions is None                                  # the internal top-5 is not handed out unasked
    i = np.arange(15)
    want = np.stack([i * (i % 3 == 0), i * 0, (i + 1) * (i % 4 == 1)], axis=1).astype(np.int32)
    care = res.care
    assert care.blocks == ["a", "b", "c"] and care.rows.dtype == np.int32 and np.array_equal(care.rows, want)
    assert np.array_equal(care.covered, ~(want != 0).any(axis=1)) and care.covered_images == int(care.covered.sum())
    top1 = (i % 7) == (i % 5)
    assert np.array_equal(care.hits[:, 0], top1)
    assert care.top1_bounds == care_bounds(care.covered, top1)
    assert abs(res.top1 - 100.0 * top1.mean()) < 1e-4 and care.top1_bounds[0] <= res.top1 + 1e-4 <= care.top1_bounds[1] + 2e-4
    lines = capsys.readouterr().out.splitlines()
    assert lines[:-1] == out0.splitlines() and lines[-1] == care.line() and lines[-2].startswith("Acc..")
    with_k = evaluate(m, batches, torch.device("cpu"), care={}, topk=2)
    assert with_k.predictions.k == 2 and np.array_equal(with_k.care.rows, want)
    unlabelled = evaluate(m, [(x, None) for x, _ in batches], torch.device("cpu"), care={}, topk=1)
    assert unlabelled.care.hits is None and np.array_equal(unlabelled.care.rows, want)


def test_evaluate_refuses_a_model_without_care_sets():
    class Stub(torch.nn.Module):
        def forward(self, x):
            return torch.zeros((x.shape[0], 10))

    batches = [(torch.zeros((2, 3, 4, 4)), torch.zeros(2, dtype=torch.int64))]
    with pytest.raises(RuntimeError, match="care=.*Stub.*set_care"):
        evaluate(Stub(), batches, torch.device("cpu"), care={})
    assert evaluate(Stub(), batches, torch.device("cpu")).care is None


_WORKER = r'''
import sys
sys.path.insert(0, {root!r})
import numpy as np, torch.distributed as dist
from scale_imagenet_amd.dist import init_from_env, all_gather_care
from scale_imagenet_amd.evaluate import CareResult
rank, world, _ = init_from_env("gloo")
n = (5, 3)[rank]
rng = np.random.default_rng(rank)
rows = rng.integers(0, 1 << 20, size=(n, 4)).astype(np.int32)
hits = rng.integers(0, 2, size=(n, 2)).astype(bool)
whole = all_gather_care(CareResult(list("abcd"), rows, hits if {labelled} else None))
np.savez({out!r} + str(rank) + ".npz", rows=whole.rows, hits=np.zeros(0) if whole.hits is None else whole.hits)
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.parametrize("labelled", [True, False])
def test_all_gather_care_two_ranks_gloo(tmp_path, labelled):
    out = str(tmp_path / "care")
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=out, labelled=labelled))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29657" if labelled else "29658", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    rngs = [np.random.default_rng(r) for r in range(2)]
    rows = [rngs[r].integers(0, 1 << 20, size=((5, 3)[r], 4)).astype(np.int32) for r in range(2)]
    hits = [rngs[r].integers(0, 2, size=((5, 3)[r], 2)).astype(bool) for r in range(2)]
    for r in range(2):
        with np.load(out + f"{r}.npz") as z:
            assert z["rows"].dtype == np.int32 and np.array_equal(z["rows"], np.concatenate(rows))      # rank order
            assert np.array_equal(z["hits"], np.concatenate(hits)) if labelled else z["hits"].size == 0
    from scale_imagenet_amd.dist import all_gather_care
    one = CareResult(["a"], rows[0][:, :1])
    assert all_gather_care(one) is one                              # a single process returns its input


def test_main_flag_errors(tmp_path):
    from scale_imagenet_amd import predict
    from scale_imagenet_amd.main import build_parser, main
    args = build_parser().parse_args(["--care_from", "u.npz", "--care_min_count", "3", "--care_rows", "r.csv", "--care_summary", "s.csv"])
    assert (args.care_from, args.care_min_count, args.care_rows, args.care_summary) == ("u.npz", 3, "r.csv", "s.csv")
    none = build_parser().parse_args([])
    assert (none.care_from, none.care_min_count, none.care_rows, none.care_summary) == (None, 1, None, None)
    with pytest.raises(SystemExit, match="--care_rows needs --care_from"):
        main(["--care_rows", "r.csv"])
    with pytest.raises(SystemExit, match="--care_summary needs --care_from"):
        main(["--care_summary", "s.csv"])
    with pytest.raises(SystemExit, match="--care_min_count needs --care_from"):
        main(["--care_min_count", "2"])
    with pytest.raises(SystemExit, match="--care_from: .* does not exist"):
        main(["--care_from", str(tmp_path / "missing.npz")])
    with pytest.raises(SystemExit, match="--care_min_count must be at least 1"):
        main(["--care_from", "u.npz", "--care_min_count", "0"])
    assert predict.build_parser().parse_args(["--care_from", "u.npz"]).care_from == "u.npz"
    with pytest.raises(SystemExit, match="--care_from: .* does not exist"):
        predict.main(["--care_from", str(tmp_path / "missing.npz")])
