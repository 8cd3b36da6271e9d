"""CPU: what the folder evaluation adds around the device kernel -- the default path of evaluate() is what it was, the
dataset is sharded without padding and four sums cross the ranks, and the command parses, documents and refuses as
it should without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _util import ROOT, golden_npz, spec_and_state
from oracle import ttnet_float as OF
from scale_imagenet_amd import synth
from scale_imagenet_amd.dist import ShardedSampler, all_reduce_metrics
from scale_imagenet_amd.evaluate import DeviceMetrics, EvalResult, evaluate

REFERENCE_FLAGS = ["--data_dir", "--eval_batch_size", "--num_workers", "--nfilter", "--tfilter", "--layers", "--groups",
                   "--gpu", "--log_interval"]


class _OracleModel(torch.nn.Module):
    """Stands in for the device model on CPU (the product has no CPU path)."""

    def __init__(self, variant):
        super().__init__()
        self.spec, st = spec_and_state(variant)
        self.sd = OF.to_torch_state(st)

    def forward(self, x):
        return OF.forward(x, self.sd, self.spec)


def _xsmall_batches():
    n = int(golden_npz("xsmall")["n_images"])
    x = torch.from_numpy(synth.synth_images(n))
    t = torch.from_numpy(synth.synth_targets(n))
    return n, [(x[:5], t[:5]), (x[5:], t[5:])]


def test_default_path_is_what_it_was(capsys):
    g = golden_npz("xsmall")
    n, batches = _xsmall_batches()
    model = _OracleModel("xsmall")
    res = evaluate(model, batches, torch.device("cpu"))
    out = capsys.readouterr().out
    assert isinstance(res, EvalResult) and res.images == n
    assert abs(res.loss - float(g["loss"])) < 1e-5
    hit1 = float((g["argmax"] == synth.synth_targets(n)).mean() * 100)
    hit5 = float((g["top5_idx"] == synth.synth_targets(n)[:, None]).any(1).mean() * 100)
    assert abs(res.top1 - hit1) < 1e-9 and abs(res.top5 - hit5) < 1e-9
    assert out == f"Acc.. {res.top1} {res.top5}\n"                # main.py:284 and nothing else
    # the keywords spelled out are the same call
    again = evaluate(model, batches, torch.device("cpu"), forward=None, metrics="torch")
    assert again == res and capsys.readouterr().out == out
    # the metrics of the parent commit's loop, restated: float32 batch means, size-weighted on the host
    loss = top1 = top5 = 0.0
    for x, t in batches:
        y = model(x)
        hits = y.topk(5, dim=1).indices.eq(t.reshape(-1, 1))
        loss += torch.nn.functional.cross_entropy(y, t).item() * len(t)
        top1 += 100.0 * hits[:, :1].any(dim=1).float().mean().item() * len(t)
        top5 += 100.0 * hits[:, :5].any(dim=1).float().mean().item() * len(t)
    assert res == EvalResult(loss / n, top1 / n, top5 / n, n)


def test_device_metrics_need_a_device():
    _, batches = _xsmall_batches()
    with pytest.raises(RuntimeError, match="HIP device"):
        evaluate(_OracleModel("xsmall"), batches, torch.device("cpu"), metrics="device")
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceMetrics(torch.device("cpu"), 2)
    with pytest.raises(ValueError):
        evaluate(_OracleModel("xsmall"), batches, torch.device("cpu"), metrics="fused")


@pytest.mark.parametrize("n", [1, 10, 50000])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_sharded_sampler_partitions_the_dataset(n, world):
    shards = [ShardedSampler(n, r, world) for r in range(world)]
    assert sum(len(s) for s in shards) == n
    assert [i for s in shards for i in s] == list(range(n))       # contiguous, in order, no padding, no duplicates
    assert max(len(s) for s in shards) - min(len(s) for s in shards) <= 1


_WORKER = r'''
import json, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import torch, torch.distributed as dist
from test_eval_device_metrics_cpu import _OracleModel, _xsmall_batches
from scale_imagenet_amd.dist import init_from_env, all_reduce_metrics
from scale_imagenet_amd.evaluate import evaluate
rank, world, _ = init_from_env("gloo")
torch.set_num_threads(2)
_, batches = _xsmall_batches()
part = evaluate(_OracleModel("xsmall"), [batches[rank]], torch.device("cpu"))      # rank 0: 5 images, rank 1: 3
res = all_reduce_metrics(part)
with open({out!r} + str(rank), "w") as f:
    json.dump([res.loss, res.top1, res.top5, res.images, part.images], f)
dist.barrier()
dist.destroy_process_group()
'''


def test_all_reduce_metrics_two_gloo_ranks(tmp_path):
    import json
    from scale_imagenet_amd.launch import spawn_ranks
    n, batches = _xsmall_batches()
    single = evaluate(_OracleModel("xsmall"), batches, torch.device("cpu"))
    assert all_reduce_metrics(single) is single                   # world size 1 returns its input
    out = str(tmp_path / "res")
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, out=out))
    assert spawn_ranks([str(script)], 2, timeout_s=600) == 0
    got = [json.load(open(out + str(r))) for r in range(2)]
    assert got[0][:4] == got[1][:4]                               # every rank returns the same result
    assert [got[0][4], got[1][4]] == [5, 3]
    loss, top1, top5, images = got[0][:4]
    assert images == n
    assert abs(top1 - single.top1) < 1e-9 and abs(top5 - single.top5) < 1e-9
    assert abs(loss - single.loss) < 1e-5


def _cli(*argv, **kw):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "-m", "scale_imagenet_amd.main", *argv], capture_output=True, text=True,
                          timeout=600, env=env, **kw)


def test_cli_help_lists_the_reference_flags(tmp_path):
    r = _cli("--help", cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    for flag in REFERENCE_FLAGS + ["--variant", "--ckpt", "--input", "--inflight", "--gpus", "--synthetic-ckpt"]:
        assert flag in r.stdout, flag
    assert "cannot be fetched" in " ".join(r.stdout.split())
    assert os.listdir(tmp_path) == []
    # the reference's training flags are accepted
    from scale_imagenet_amd.main import build_parser
    a = build_parser().parse_args(["--lr", "0.2", "--max_epochs", "3", "--pretrain", "--dist-url", "tcp://x:1"])
    assert (a.eval_batch_size, a.num_workers, a.nfilter, a.tfilter, a.layers, a.groups, a.gpu, a.log_interval) == \
        (100, 6, 8, 8, 1, "1,None,4,None", None, 40)


def test_cli_import_parses_nothing_and_creates_nothing(tmp_path):
    code = ("import sys, os; sys.argv = ['x', '--no-such-flag']; import scale_imagenet_amd.main as m; "
            "assert callable(m.main); print(sorted(os.listdir('.')))")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get("PYTHONPATH")) if p))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "[]"


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_cli_self_launch_fails_in_the_parent_without_a_gpu(tmp_path):
    (tmp_path / "val" / "a").mkdir(parents=True)
    r = _cli("--gpus", "2", "--data_dir", str(tmp_path), "--synthetic-ckpt", cwd=str(tmp_path))
    assert r.returncode != 0
    assert "no HIP device" in r.stderr and "no rank was started" in r.stderr
    assert "Traceback" not in r.stderr                            # the parent's own message, not a rank's crash
