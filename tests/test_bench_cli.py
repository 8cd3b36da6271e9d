"""CPU: bench.py's options and its output dump (no device needed: the dump takes any tensor)."""
import os

import numpy as np
import torch

import bench


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2
    assert a.full is False and a.dump_outputs is None and a.windows == 0
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert b.full is True and b.dump_outputs == "out"


def test_dump_writes_float32_logits(tmp_path):
    y = torch.arange(12 * 1000, dtype=torch.float32).reshape(12, 1000) / 7.0
    (tmp_path / "logits_rows.npy").write_bytes(b"stale")          # left by an earlier, larger run
    bench.dump_outputs(str(tmp_path), y)
    got = np.load(tmp_path / "logits.npy")
    assert got.dtype == np.float32 and np.array_equal(got, y.numpy())
    assert sorted(os.listdir(tmp_path)) == ["logits.npy"]


def test_dump_beyond_the_limit_keeps_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64_000)
    y = torch.randn(100, 1000, generator=torch.Generator().manual_seed(3))
    outs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), y)
        rows = np.load(d / "logits_rows.npy")
        got = np.load(d / "logits.npy")
        assert rows.dtype == np.float64 and got.dtype == np.float32
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000
        idx = rows.astype(np.int64)
        assert len(idx) > 1 and np.all(np.diff(idx) > 0) and idx[-1] < 100
        assert np.array_equal(got, y.numpy()[idx])
        outs.append(idx)
    assert np.array_equal(outs[0], outs[1])
