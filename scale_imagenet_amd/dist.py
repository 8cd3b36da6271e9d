"""Batch sharding across GPUs: one process per GPU, RCCL (torch.distributed "nccl") over xGMI.

The path shards by image: eval-mode BatchNorm uses running statistics and nothing in the
forward crosses samples.  Every rank builds its own tables from the same
state_dict (no parameter broadcast, unlike DataParallel.replicate / the DDP constructor,
main.py:181-192); the only exchange is the gather of logits that
``torch.nn.DataParallel.gather`` performs on GPU 0 in the reference (main.py:192), here one
all-gather of ``[B/world, 1000]`` fp32.

Evaluating a dataset needs less still: every rank evaluates its ``ShardedSampler`` slice and one
``all_reduce_metrics`` sums four numbers (loss sum, images, top-1 hits, top-5 hits).  Per-image predictions are
joined in rank order (``all_gather_predictions``), per-class counters summed (``all_reduce_counts``), truth-table
usage counters summed (``all_reduce_table_usage``), the care-set rows joined (``all_gather_care``).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.distributed as dist


def shard_bounds(n_total: int, rank: int, world: int) -> Tuple[int, int]:
    """(first image, count) of ``rank``'s contiguous shard; earlier ranks take the remainder."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world {world}")
    base, rem = divmod(n_total, world)
    count = base + (1 if rank < rem else 0)
    first = rank * base + min(rank, rem)
    return first, count


def init_from_env(backend: Optional[str] = None) -> Tuple[int, int, int]:
    """Join the job described by RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* (torchrun).
    Returns (rank, world, local_rank).  Single process when WORLD_SIZE is unset or 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("TTNET_DIST_BACKEND", backend)     # rehearsal on one GPU: "gloo"
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend, rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, local_rank


def all_gather_logits(local: torch.Tensor, n_total: int, group=None) -> torch.Tensor:
    """Gather per-rank logits ``[count_r, C]`` (shards from ``shard_bounds``) into ``[n_total, C]``
    in image order on every rank.  Ragged shards are padded to the largest and trimmed."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        if local.shape[0] != n_total:
            raise ValueError("single process must hold the whole batch")
        return local
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    first, count = shard_bounds(n_total, rank, world)
    if local.shape[0] != count:
        raise ValueError(f"rank {rank}: expected {count} rows, got {local.shape[0]}")
    width = shard_bounds(n_total, 0, world)[1]
    if count < width:
        pad = torch.zeros((width - count, local.shape[1]), dtype=local.dtype, device=local.device)
        local = torch.cat([local, pad])
    if local.is_cuda and dist.get_backend(group) == "gloo":     # rehearsal path: gloo gathers on the host
        host = torch.empty((world * width, local.shape[1]), dtype=local.dtype)
        dist.all_gather_into_tensor(host, local.cpu().contiguous(), group=group)
        out = host.to(local.device)
    else:
        out = torch.empty((world * width, local.shape[1]), dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, local.contiguous(), group=group)
    if n_total == world * width:
        return out
    rows = [out[r * width: r * width + shard_bounds(n_total, r, world)[1]] for r in range(world)]
    return torch.cat(rows)


class ShardedSampler(torch.utils.data.Sampler):
    """``rank``'s contiguous ``shard_bounds`` slice of a dataset of ``n`` samples, in order: the shards partition
    ``range(n)`` -- no padding, no duplicates, so the summed metrics are those of the dataset.  (The reference's DDP
    path gives every rank the full validation set, main.py:214; ``DistributedSampler`` pads with repeats.)"""

    def __init__(self, n: int, rank: int, world: int):
        self.first, self.count = shard_bounds(int(n), rank, world)

    def __iter__(self):
        return iter(range(self.first, self.first + self.count))

    def __len__(self) -> int:
        return self.count


def all_reduce_metrics(part, group=None):
    """Sum the evaluation of every rank's shard: one ``all_reduce(SUM)`` of ``[loss_sum, images, hits1, hits5]``
    (float64 / int64 carried in one float64 tensor: the counts are far below 2^53, so their sum is exact).  ``part``
    is this rank's ``EvalResult`` (or ``EvalParts``); every rank returns the same ``EvalResult``.  Host tensors under
    gloo, device tensors under nccl.  A single process returns its input."""
    from .evaluate import EvalParts, EvalResult
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return part
    p = part.to_parts() if isinstance(part, EvalResult) else part
    v = torch.tensor([p.loss_sum, float(p.images), float(p.hits1), float(p.hits5)], dtype=torch.float64)
    if dist.get_backend(group) != "gloo":
        v = v.to(torch.device("cuda", torch.cuda.current_device()))
    dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
    loss_sum, images, hits1, hits5 = v.cpu().tolist()
    return EvalParts(loss_sum, int(round(images)), int(round(hits1)), int(round(hits5))).result()


def _wire(t: torch.Tensor, group=None) -> torch.Tensor:
    """Where a collective wants its tensor: the host under gloo, this rank's device under nccl."""
    return t if dist.get_backend(group) == "gloo" else t.to(torch.device("cuda", torch.cuda.current_device()))


def all_gather_predictions(pred, group=None):
    """Every rank's ``Predictions`` joined in rank order, which is dataset order for ``ShardedSampler`` shards
    (contiguous, earlier ranks first).  The shards may differ in length: two collectives, one of the lengths and one
    of the 16-byte records padded to the longest.  Every rank returns the whole; a single process returns its input."""
    from .evaluate import Predictions
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return pred
    world = dist.get_world_size(group)
    counts = _wire(torch.zeros(world, dtype=torch.int64), group)
    dist.all_gather_into_tensor(counts, _wire(torch.tensor([len(pred)], dtype=torch.int64), group), group=group)
    counts = counts.cpu().tolist()
    width = max(max(counts), 1)
    local = torch.zeros((width, pred.k, 2), dtype=torch.int64)
    local[:len(pred)] = torch.from_numpy(pred.to_records())
    out = _wire(torch.empty((world * width, pred.k, 2), dtype=torch.int64), group)
    dist.all_gather_into_tensor(out, _wire(local, group), group=group)
    out = out.cpu().numpy()
    return Predictions.join([Predictions.from_records(out[r * width: r * width + counts[r]]) for r in range(world)])


def all_gather_care(care, group=None):
    """Every rank's ``evaluate.CareResult`` joined in rank order (dataset order for ``ShardedSampler`` shards), as
    ``all_gather_predictions`` joins the predictions: the int32 rows, with the two hit flags of a labelled run as two more
    columns, padded to the longest shard.  Every rank returns the whole; a single process returns its input."""
    from .evaluate import CareResult
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return care
    import numpy as np
    world = dist.get_world_size(group)
    n, b = care.rows.shape
    counts = _wire(torch.zeros(world, dtype=torch.int64), group)
    dist.all_gather_into_tensor(counts, _wire(torch.tensor([n], dtype=torch.int64), group), group=group)
    counts = counts.cpu().tolist()
    width = max(max(counts), 1)
    local = torch.zeros((width, b + 2), dtype=torch.int32)
    local[:n, :b] = torch.from_numpy(np.ascontiguousarray(care.rows, dtype=np.int32))
    local[:n, b:] = -1 if care.hits is None else torch.from_numpy(np.ascontiguousarray(care.hits, dtype=np.int32))
    out = _wire(torch.empty((world * width, b + 2), dtype=torch.int32), group)
    dist.all_gather_into_tensor(out, _wire(local, group), group=group)
    out = np.concatenate([out.cpu().numpy()[r * width: r * width + counts[r]] for r in range(world)])
    return CareResult(list(care.blocks), out[:, :b].copy(), None if care.hits is None else out[:, b:] == 1)


def all_reduce_counts(counts, confusion=None, group=None):
    """Sum the per-class counters (and the confusion matrix, when there is one) of every rank: one
    ``all_reduce(SUM)`` of one int64 tensor.  numpy in, numpy out; a single process returns its input."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return counts, confusion
    import numpy as np
    flat = [torch.from_numpy(np.ascontiguousarray(counts)).reshape(-1)]
    if confusion is not None:
        flat.append(torch.from_numpy(np.ascontiguousarray(confusion)).reshape(-1))
    v = _wire(torch.cat(flat), group)
    dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
    v = v.cpu().numpy()
    n = counts.size
    return v[:n].reshape(counts.shape).copy(), None if confusion is None else v[n:].reshape(confusion.shape).copy()


def all_reduce_table_usage(usage, group=None):
    """Sum the truth-table usage counters of every rank (``EvalResult.table_usage``: ``{Block_TT name: int64 [groups,
    2^n]}``): one ``all_reduce(SUM)`` per block, in name order, so that no more than one block's counters (268 MB for
    the largest of TT-small p = 64) is on the wire at a time.  Integer sums: the result does not depend on how the
    images were sharded.  numpy in, numpy out; every rank must hold the same blocks; a single process returns its input."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return usage
    import numpy as np
    out = {}
    for name in sorted(usage):
        a = np.ascontiguousarray(usage[name], dtype=np.int64)
        v = _wire(torch.from_numpy(a.copy()).reshape(-1), group)
        dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
        out[name] = v.cpu().numpy().reshape(a.shape)
    return {name: out[name] for name in usage}
