"""Evaluation loop: the caller of the hot path (counterpart of ``test()``, main.py:242-284).

Reproduces the reference's metric definitions -- cross-entropy loss, top-1 / top-5 running
means weighted by batch size (utils/bar_show.py:110-148), the final ``Acc..`` line
(main.py:284) -- around the forward.  The whole input pipeline is in scope: a batch may be a
float tensor (``model(x)``), uint8 HWC images of the model's input size (``model.forward_u8``), decoded images of
mixed sizes (``RaggedU8`` -> ``preprocess.imgnet_eval_forward``) or compressed files
(``RaggedJpeg`` -> ``jpeg.jpeg_eval_forward``); ``forward=`` overrides the choice.  TensorBoard
and the terminal progress bar of the reference stay out of scope.

Two ways to the metrics:

``metrics="torch"`` (default)  ``F.cross_entropy`` + ``topk`` per batch, three scalars read back
    per batch, float32 batch means accumulated on the host as the reference does.
``metrics="device"``  ``DeviceMetrics``: one ``ttnet_eval_metrics`` call per batch on the lane's
    stream adds the batch to a 64-byte accumulator on the device; nothing is read back until
    the end (or a ``log_every`` line).  ``loss`` is then ``loss_sum / images`` with every
    per-image loss and the sum in float64, so it differs from the ``"torch"`` path in the last
    digits (float32 batch means there); ``top1`` / ``top5`` are ``100 * hits / images`` from
    exact integer counts and equal the ``"torch"`` path's whenever no target's logit is tied
    across the k-th place (ties go to the lower class index here, include/ttnet.h).

Beyond the four numbers, the same loop answers *what did it say about each image* and *which classes fail*:
``topk=k`` adds ``Predictions`` (the k best classes of every image, their logits and float64 log-probabilities, in
dataset order) from one ``ttnet_topk_rows`` call per batch, whose ``n * k * 16`` bytes are the only thing copied back;
``per_class`` / ``confusion`` add per-class counters and a confusion matrix that ``ttnet_class_counts`` keeps on the
device until the end.  A batch ``(inputs, None)`` has no labels: forward and top-k only.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib


class RunningMean:
    """Batch-size weighted running mean (``AverageMeter``, utils/bar_show.py:127-148)."""

    def __init__(self, name: str = ""):
        self.name = name
        self.total = 0.0
        self.count = 0
        self.last = 0.0

    def update(self, value: float, n: int = 1):
        self.last = float(value)
        self.total += float(value) * n
        self.count += n

    @property
    def avg(self) -> float:
        return self.total / self.count if self.count else 0.0


def topk_percent(logits: torch.Tensor, targets: torch.Tensor, ks=(1, 5)):
    """Percent of rows whose target is among the k largest logits (utils/bar_show.py:110-124)."""
    order = logits.topk(max(ks), dim=1).indices
    hits = order.eq(targets.reshape(-1, 1))
    return [100.0 * hits[:, :k].any(dim=1).float().mean().item() for k in ks]


@dataclass
class EvalParts:
    """The sums an evaluation is made of: what crosses ranks (``dist.all_reduce_metrics``)."""
    loss_sum: float
    images: int
    hits1: int
    hits5: int

    def result(self) -> "EvalResult":
        n = self.images
        res = EvalResult(self.loss_sum / n if n else 0.0, 100.0 * self.hits1 / n if n else 0.0,
                         100.0 * self.hits5 / n if n else 0.0, n)
        res.parts = self
        return res


@dataclass
class EvalResult:
    loss: float
    top1: float
    top5: float
    images: int
    parts = None        # (not a field) the exact sums behind the four numbers, when the device metrics produced them
    predictions = None  # (not a field) ``Predictions`` in dataset order, with ``topk=k``
    per_class = None    # (not a field) int64 [n_classes, 4] {images, hits1, hits5, predicted}, with ``per_class=True``
    confusion = None    # (not a field) int64 [n_classes, n_classes] indexed [target][top-1 class], with ``confusion=True``
    table_usage = None  # (not a field) {Block_TT name: int64 [groups, 2^n]} lookups per table entry, with ``table_usage=True``
    care = None         # (not a field) ``CareResult``: per-image care-set misses in dataset order, with ``care=``

    def to_parts(self) -> EvalParts:
        """The sums behind this result: exact when ``parts`` is set, otherwise recovered from the means (the hit
        counts exactly, ``loss_sum`` to the last digit of ``loss * images``)."""
        if self.parts is not None:
            return self.parts
        return EvalParts(self.loss * self.images, self.images, int(round(self.top1 * self.images / 100.0)),
                         int(round(self.top5 * self.images / 100.0)))


@dataclass
class Predictions:
    """The k best classes of N images, best first (the rules of ``ttnet_topk_rows``, include/ttnet.h): larger logit
    first, equal logits by lower class index; a row with a NaN holds class -1, logit NaN, logprob NaN in every slot."""
    classes: np.ndarray     # int32 [N, k]
    logit: np.ndarray       # float32 [N, k]
    logprob: np.ndarray     # float64 [N, k]: log softmax of the row at that class

    def __len__(self) -> int:
        return self.classes.shape[0]

    @property
    def k(self) -> int:
        return self.classes.shape[1]

    @staticmethod
    def from_records(rec: np.ndarray) -> "Predictions":
        """From ``[N, k]`` records of 16 bytes ``{int32 class; float32 logit; double logprob}`` given as int64 [N, k, 2]."""
        rec = np.ascontiguousarray(rec, dtype=np.int64)
        n, k = rec.shape[:2]
        w = rec.view(np.int32).reshape(n, k, 4)
        return Predictions(w[:, :, 0].copy(), w[:, :, 1].copy().view(np.float32), rec[:, :, 1].copy().view(np.float64))

    def to_records(self) -> np.ndarray:
        """The inverse of ``from_records``: what crosses the ranks (``dist.all_gather_predictions``)."""
        rec = np.empty((len(self), self.k, 2), dtype=np.int64)
        w = rec.view(np.int32).reshape(len(self), self.k, 4)
        w[:, :, 0] = self.classes
        w[:, :, 1] = np.ascontiguousarray(self.logit, dtype=np.float32).view(np.int32)
        rec[:, :, 1] = np.ascontiguousarray(self.logprob, dtype=np.float64).view(np.int64)
        return rec

    @staticmethod
    def join(parts: "List[Predictions]") -> "Predictions":
        """Shards in dataset order -> one ``Predictions`` (``ShardedSampler`` shards are contiguous: rank order)."""
        return Predictions(np.concatenate([p.classes for p in parts]), np.concatenate([p.logit for p in parts]),
                           np.concatenate([p.logprob for p in parts]))


def care_bounds(covered: np.ndarray, hits: np.ndarray) -> Tuple[float, float]:
    """The bracket, in percent, on the accuracy of ANY circuit that agrees with the network's tables on the care sets:
    ``covered`` bool [N] (no miss in any block: that image's logits are the network's, bit for bit), ``hits`` bool [N]
    (the network is right on that image).  With C covered images of which h are hits, ``h / N <= accuracy <=
    (h + N - C) / N``: a covered image counts as it does for the network, an uncovered one may go either way."""
    covered, hits = np.asarray(covered, dtype=bool), np.asarray(hits, dtype=bool)
    n = covered.size
    if hits.shape != covered.shape:
        raise ValueError(f"care_bounds: {covered.size} covered flags but hits of shape {tuple(hits.shape)}")
    if n == 0:
        return 0.0, 0.0
    h, c = int((covered & hits).sum()), int(covered.sum())
    return 100.0 * h / n, 100.0 * (h + n - c) / n


@dataclass
class CareResult:
    """Care-set misses of an evaluation (``evaluate(care=)``): ``rows[i][b]`` = lookups of image i (dataset order) in
    ``Block_TT`` ``blocks[b]`` that fell outside its care set."""
    blocks: List[str]
    rows: np.ndarray                    # int32 [N, B]
    hits: Optional[np.ndarray] = None   # bool [N, 2]: the target is the network's best class / among its 5 best (labelled runs)

    @property
    def covered(self) -> np.ndarray:
        """bool [N]: no miss in any block."""
        return ~(self.rows != 0).any(axis=1)

    @property
    def covered_images(self) -> int:
        return int(self.covered.sum())

    @property
    def images_with_misses(self) -> "OrderedDict[str, int]":
        return OrderedDict(zip(self.blocks, (self.rows != 0).sum(axis=0).tolist()))

    @property
    def misses(self) -> "OrderedDict[str, int]":
        return OrderedDict(zip(self.blocks, self.rows.astype(np.int64).sum(axis=0).tolist()))

    @property
    def top1_bounds(self) -> Optional[Tuple[float, float]]:
        return None if self.hits is None else care_bounds(self.covered, self.hits[:, 0])

    @property
    def top5_bounds(self) -> Optional[Tuple[float, float]]:
        return None if self.hits is None else care_bounds(self.covered, self.hits[:, 1])

    def line(self) -> str:
        """``Care.. covered/N top1 [lo, hi] top5 [lo, hi]`` (the bounds only for a labelled run)."""
        text = f"Care.. {self.covered_images}/{len(self.rows)}"
        if self.hits is not None:
            text += " top1 [%.3f, %.3f] top5 [%.3f, %.3f]" % (self.top1_bounds + self.top5_bounds)
        return text


def _check_k(k: int, n_classes: int):
    if not (1 <= k <= min(n_classes, _lib.TOPK_MAX)):
        raise ValueError(f"topk must be in [1, min(n_classes, {_lib.TOPK_MAX})], got {k} for {n_classes} classes")


def topk_rows(logits: torch.Tensor, k: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``ttnet_topk_rows`` on the current stream: float32 HIP logits ``[n, n_classes]`` -> the records, int64
    ``[n, k, 2]`` on the device (``Predictions.from_records`` unpacks them on the host).  Asynchronous, capturable."""
    if (not logits.is_cuda) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise RuntimeError(f"expected float32 HIP logits [n, n_classes], got {logits.dtype} {tuple(logits.shape)} on "
                           f"{logits.device}: ttnet_topk_rows has no CPU path")
    n, n_classes = logits.shape
    _check_k(k, n_classes)
    logits = logits.contiguous()
    if out is None:
        out = torch.empty((n, k, 2), dtype=torch.int64, device=logits.device)
    elif out.device != logits.device or out.dtype != torch.int64 or tuple(out.shape) != (n, k, 2) or not out.is_contiguous():
        raise RuntimeError(f"expected contiguous int64 records [{n}, {k}, 2] on {logits.device}")
    with torch.cuda.device(logits.device):
        stream = torch.cuda.current_stream(logits.device).cuda_stream
        _lib.check(_lib.load().ttnet_topk_rows(C.c_void_p(logits.data_ptr()), n, n_classes, k, C.c_void_p(out.data_ptr()),
                                               C.c_void_p(stream)))
    return out


def topk_rows_host(logits: torch.Tensor, k: int) -> Predictions:
    """The same rules for logits on the CPU (a stub model in a test; the product has no CPU path): a stable descending
    sort puts equal logits in index order, the log-probabilities are float64."""
    n, n_classes = logits.shape
    _check_k(k, n_classes)
    x = logits.detach().to(torch.float32)
    order = torch.sort(x, dim=1, descending=True, stable=True).indices[:, :k]
    logprob = torch.log_softmax(x.double(), dim=1).gather(1, order)
    classes, logit = order.to(torch.int32), x.gather(1, order)
    nan = torch.isnan(x).any(dim=1)
    classes[nan], logit[nan], logprob[nan] = -1, float("nan"), float("nan")
    return Predictions(classes.numpy(), logit.numpy(), logprob.numpy())


class DeviceMetrics:
    """Loss / top-1 / top-5 accumulated on the device by ``ttnet_eval_metrics`` (csrc/metrics.hip): one 64-byte
    accumulator per lane, added to by ``update`` on the current stream, read back once by ``result``."""

    def __init__(self, device, lanes: int = 1, confusion: bool = False):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"DeviceMetrics needs a HIP device, got {device}: the device metrics have no CPU path "
                               "(use metrics=\"torch\")")
        if lanes < 1:
            raise ValueError("lanes must be positive")
        self.device, self.lanes = device, int(lanes)
        self.acc = torch.zeros((self.lanes, 8), dtype=torch.int64, device=device)      # ttnet_eval_acc [lanes]
        assert self.acc.element_size() * 8 == C.sizeof(_lib.EvalAcc)
        self.want_confusion = bool(confusion)
        self.counts = self.confusion = None               # shared by the lanes (integer atomics): made by the first
                                                          # per_class update, which knows n_classes

    def _counters(self, n_classes: int):
        if self.counts is None:
            self.counts = torch.zeros((n_classes, 4), dtype=torch.int64, device=self.device)
            if self.want_confusion:
                self.confusion = torch.zeros((n_classes, n_classes), dtype=torch.int64, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()     # once: zeroed before any other lane's stream adds
        elif self.counts.shape[0] != n_classes:
            raise RuntimeError(f"per-class counters were made for {self.counts.shape[0]} classes, got {n_classes}")

    def update(self, logits: torch.Tensor, targets: torch.Tensor, lane: int = 0, per_image: bool = False, *,
               topk: Optional[torch.Tensor] = None, per_class: bool = False):
        """Add a batch (float32 ``[n, n_classes]`` logits, int64 ``[n]`` targets, both on the device) to ``lane``'s
        accumulator: asynchronous on the current stream, capturable.  ``per_image=True`` returns the per-image
        ``(loss float64 [n], rank int32 [n])`` (rank -1: target out of range; INT32_MAX: a NaN in the row).

        ``per_class=True`` also adds the batch to ``counts`` (and ``confusion``, when the object was made with it) by
        one ``ttnet_class_counts`` call; it needs the batch's ``topk_rows`` records, passed as ``topk`` (computed here
        with k = 1 when absent).  The return value is what it is without these arguments."""
        if not (0 <= lane < self.lanes):
            raise RuntimeError(f"lane {lane} outside [0, {self.lanes})")
        if (not logits.is_cuda) or logits.dtype != torch.float32 or logits.dim() != 2:
            raise RuntimeError(f"expected float32 HIP logits [n, n_classes], got {logits.dtype} {tuple(logits.shape)} on "
                               f"{logits.device}")
        n, n_classes = logits.shape
        if targets.device != logits.device or targets.dtype != torch.int64 or tuple(targets.shape) != (n,):
            raise RuntimeError(f"expected int64 targets [{n}] on {logits.device}, got {targets.dtype} "
                               f"{tuple(targets.shape)} on {targets.device}")
        logits, targets = logits.contiguous(), targets.contiguous()
        rec = torch.empty((n, 2), dtype=torch.int64, device=logits.device)               # {double loss; int32 rank, 0}
        with torch.cuda.device(logits.device):
            stream = torch.cuda.current_stream(logits.device).cuda_stream
            _lib.check(_lib.load().ttnet_eval_metrics(
                C.c_void_p(logits.data_ptr()), C.c_void_p(targets.data_ptr()), n, n_classes,
                C.c_void_p(self.acc[lane].data_ptr()), C.c_void_p(rec.data_ptr()), C.c_void_p(stream)))
            if per_class:
                if topk is None:
                    topk = topk_rows(logits, 1)
                elif topk.device != logits.device or topk.dtype != torch.int64 or topk.dim() != 3 or topk.shape[0] != n \
                        or topk.shape[2] != 2 or not topk.is_contiguous():
                    raise RuntimeError(f"expected the contiguous int64 [{n}, k, 2] records of topk_rows on {logits.device}")
                self._counters(n_classes)
                _lib.check(_lib.load().ttnet_class_counts(
                    C.c_void_p(targets.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_void_p(topk.data_ptr()), n,
                    topk.shape[1], n_classes, C.c_void_p(self.counts.data_ptr()),
                    C.c_void_p(self.confusion.data_ptr()) if self.confusion is not None else None, C.c_void_p(stream)))
        if per_image:
            return rec[:, 0].view(torch.float64), rec.view(torch.int32)[:, 2]
        return None

    def class_counts(self) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """Synchronise once and read the counters back: ``(counts int64 [n_classes, 4], confusion or None)``;
        ``(None, None)`` when no ``per_class`` update was made."""
        if self.counts is None:
            return None, None
        torch.cuda.synchronize(self.device)
        return self.counts.cpu().numpy(), self.confusion.cpu().numpy() if self.confusion is not None else None

    def parts(self, check: bool = True) -> EvalParts:
        """Synchronise the device once and sum the lanes in lane order."""
        torch.cuda.synchronize(self.device)
        host = self.acc.cpu()
        loss = host[:, 0].view(torch.float64).tolist()
        ints = host[:, 1:5].tolist()
        bad = sum(r[3] for r in ints)
        if check and bad:
            raise RuntimeError(f"evaluate: {bad} target(s) were outside [0, n_classes): they count as no hit and are "
                               "left out of the loss, so the metrics are not those of the dataset")
        loss_sum = 0.0
        for v in loss:
            loss_sum += v
        return EvalParts(loss_sum, sum(r[0] for r in ints), sum(r[1] for r in ints), sum(r[2] for r in ints))

    def result(self) -> EvalResult:
        """``EvalResult`` of everything added so far; raises, naming the count, if any target was out of range."""
        return self.parts().result()


class _TorchMetrics:
    """``metrics="torch"``: ``F.cross_entropy`` + ``topk`` per batch on the batch's stream; the three scalars are read
    back when the batch retires and accumulated as float32 batch means, as the reference does."""
    logs = "retired"

    def __init__(self):
        self.loss, self.top1, self.top5 = RunningMean("Loss"), RunningMean("Acc@1"), RunningMean("Acc@5")

    def add(self, outputs, targets, lane):
        loss = F.cross_entropy(outputs, targets)
        order = outputs.topk(5, dim=1).indices
        hits = order.eq(targets.reshape(-1, 1))
        return loss, hits[:, :1].any(dim=1).float().mean(), hits[:, :5].any(dim=1).float().mean()

    def add_with_topk(self, outputs, targets, lane, topk):
        return self.add(outputs, targets, lane)           # (the records are of no use to the torch metrics)

    def retire(self, batch, n):
        loss, hits1, hits5 = batch
        self.loss.update(loss.item(), n)
        self.top1.update(100.0 * hits1.item(), n)
        self.top5.update(100.0 * hits5.item(), n)

    def running(self):
        return self.loss.avg, self.top1.avg, self.top5.avg

    def result(self) -> EvalResult:
        return EvalResult(self.loss.avg, self.top1.avg, self.top5.avg, self.loss.count)


class _OnDeviceMetrics:
    """``metrics="device"``: ``DeviceMetrics.update`` per batch on the batch's stream; nothing is read back when a batch
    retires, a log line reads the accumulators (one synchronisation, no range check), ``result`` reads them once."""
    logs = "issued"

    def __init__(self, device, lanes, streams, per_class=False, confusion=False):
        self.dm = DeviceMetrics(device, lanes, confusion=confusion)
        self.per_class = per_class
        # add(outputs, targets, lane): nothing to keep for retire
        self.add = self.add_with_topk if per_class else self.dm.update
        for s in streams:                                 # the accumulators were zeroed on the current stream
            s.wait_stream(torch.cuda.current_stream(device))

    def add_with_topk(self, outputs, targets, lane, topk=None):
        """``add`` for a batch whose ``topk_rows`` records exist already: the per-class counters read their first slot."""
        return self.dm.update(outputs, targets, lane, topk=topk, per_class=self.per_class)

    def retire(self, batch, n):
        pass

    def running(self):
        p = self.dm.parts(check=False).result()
        return p.loss, p.top1, p.top5

    def result(self) -> EvalResult:
        res = self.dm.result()                            # (one synchronisation; raises on a target out of range)
        res.per_class, res.confusion = self.dm.class_counts()
        return res


class _Care:
    """``care=``: ``model.care_misses(lane)`` after every forward on the batch's stream, its ``n * B * 4`` bytes copied to
    the lane's pinned buffer on that stream and collected when the batch retires, as ``_TopK`` does with its records."""

    def __init__(self, lanes: int):
        self.pinned = [None] * lanes
        self.rows: List[np.ndarray] = []
        self.hits: List[np.ndarray] = []

    def add(self, model, lane: int, asynchronous: bool):
        rows = model.care_misses(lane)
        if not rows.is_cuda:                              # (a stub model in a test)
            return rows
        n = rows.shape[0]
        if self.pinned[lane] is None or self.pinned[lane].shape[0] < n:
            self.pinned[lane] = torch.empty((n, rows.shape[1]), dtype=torch.int32, pin_memory=True)
        host = self.pinned[lane][:n]
        host.copy_(rows, non_blocking=asynchronous)
        return host

    def retire(self, host, pred: "Predictions", targets):
        self.rows.append(host.numpy().copy())
        if targets is not None:
            t = targets.cpu().numpy().reshape(-1, 1)
            eq = pred.classes[:, :5] == t
            self.hits.append(np.stack([eq[:, 0], eq.any(axis=1)], axis=1))

    def result(self, blocks) -> CareResult:
        rows = np.concatenate(self.rows) if self.rows else np.empty((0, len(blocks)), np.int32)
        return CareResult(list(blocks), rows.astype(np.int32, copy=False), np.concatenate(self.hits) if self.hits else None)


class _TopK:
    """``topk=k``: one ``ttnet_topk_rows`` call per batch on the batch's stream, its ``n * k * 16`` bytes copied to the
    lane's pinned buffer on that stream and collected when the batch retires (by then the lane's event has passed).
    Logits on the CPU (a stub model) go through ``topk_rows_host``."""

    def __init__(self, k: int, lanes: int):
        self.k = k
        self.pinned = [None] * lanes
        self.parts: List[Predictions] = []

    def add(self, outputs, lane: int, asynchronous: bool):
        """Returns ``(what retire() needs, the records on the device or None)``."""
        if not outputs.is_cuda:
            return topk_rows_host(outputs, self.k), None
        rec = topk_rows(outputs, self.k)
        n = rec.shape[0]
        if self.pinned[lane] is None or self.pinned[lane].shape[0] < n:
            self.pinned[lane] = torch.empty((n, self.k, 2), dtype=torch.int64, pin_memory=True)
        host = self.pinned[lane][:n]
        host.copy_(rec, non_blocking=asynchronous)
        return host, rec

    def retire(self, kept):
        self.parts.append(kept if isinstance(kept, Predictions) else Predictions.from_records(kept.numpy()))

    def result(self) -> Predictions:
        if not self.parts:
            return Predictions(np.empty((0, self.k), np.int32), np.empty((0, self.k), np.float32), np.empty((0, self.k), np.float64))
        return Predictions.join(self.parts)


@torch.no_grad()
def evaluate(model: torch.nn.Module, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]],
             device: torch.device, log_every: int = 0, inflight: int = 1, *,
             forward: Optional[Callable] = None, metrics: str = "torch", topk: int = 0, per_class: bool = False,
             confusion: bool = False, table_usage: bool = False, care=None, care_min_count: int = 1,
             views: Optional[str] = None) -> EvalResult:
    """main.py:242-284: ``model.eval()``, no_grad, per batch loss / top-1 / top-5.

    ``inflight`` > 1 keeps that many batches in flight on separate HIP streams and model lanes
    (``model.set_lanes``): the loss / top-k of a batch stay on the device until its lane comes
    round again, instead of the reference's ``.item()`` after every batch, so the ramp and tail
    of one batch's kernels overlap the next batch.  The metrics are the same numbers in the same
    order of accumulation.

    A batch is ``(inputs, targets)``; ``inputs`` is moved with ``.to(device, non_blocking=True)`` on the lane's
    stream and its type selects the forward: float tensor -> ``model(x)``; uint8 ``[n,H,W,3]`` at the model's input size
    (224 x 224 crops; the 32 x 32 CIFAR bytes of ``cifar.device_batches`` for the vAlexnet model) -> ``model.forward_u8``; ``RaggedU8`` -> ``preprocess.imgnet_eval_forward``; ``RaggedJpeg`` ->
    ``jpeg.jpeg_eval_forward``.  ``forward(model, inputs, lane)`` replaces that choice.  After the loop the sticky
    error counts of the pipeline are checked (``check_range``, and ``check_ragged`` / ``check_jpeg`` when such
    batches were seen): a corrupt file or an overflow raises instead of returning metrics.

    ``metrics="device"`` reduces loss and hits on the device (``DeviceMetrics``): nothing is read back per batch, a
    lane is reused after its event, and ``log_every`` reads the accumulators -- one synchronisation -- only on the
    batches it logs.  See the module docstring for how its numbers relate to the default ``"torch"`` path.

    ``topk=k`` (1 .. 32): the result's ``predictions`` are the k best classes of every image, in dataset order
    whatever ``inflight`` is.  ``per_class`` / ``confusion`` (device metrics only): its ``per_class`` / ``confusion``
    are the counters of ``ttnet_class_counts``, read back once at the end.  With the defaults nothing changes.  A batch
    ``(inputs, None)`` is unlabelled: forward and top-k only; the result then has ``loss = top1 = top5 = None`` and no
    ``Acc..`` line is printed.  Labelled and unlabelled batches do not mix.

    ``table_usage=True``: the result's ``table_usage`` says how often the evaluation read every entry of every truth
    table (``{Block_TT name: int64 [groups, 2^n]}``, canonical order; include/ttnet.h).  The counters are enabled and
    zeroed first and ``model.add_table_usage(lane)`` follows every forward on the batch's stream, whatever the input
    type and ``inflight``; nothing is read back before the end.  Size the plan first (``model.reserve``): a plan that has
    to grow for a larger batch would start its counters again, which raises here.

    ``care=``: care-set bitmaps or usage counts, as ``model.set_care(care, care_min_count)`` takes them.  The result's
    ``care`` (``CareResult``) holds, for every image in dataset order whatever ``inflight`` is, the lookups of every
    ``Block_TT`` that fell outside its care set, which images are covered (no miss anywhere: a circuit minimised with the
    other entries as don't-cares classifies them exactly as the network does) and, for a labelled run, the bracket that
    puts on the circuit's top-1 / top-5 accuracy (``care_bounds``).  The bounds come from per-image top-5 records, so the
    evaluation keeps at least 5 predictions per image internally; ``predictions`` is returned only for ``topk > 0``, with
    the k asked for.  The care set stays installed afterwards (``model.clear_care()``).

    ``views="flip" | "five" | "ten"``: multi-crop evaluation, torchvision's ``Resize(256)`` -> ``FiveCrop(224)`` /
    ``TenCrop(224)`` (or centre crop + its flip) -> ``outputs.view(n, V, -1).mean(1)``.  ``RaggedU8`` and ``RaggedJpeg``
    batches go through ``preprocess.imgnet_views_forward`` / ``jpeg.jpeg_views_forward``: every image is uploaded (and
    decoded) once, its V crops are cut on the device, ``n * V`` crops are forwarded -- size the plan for that
    (``model.reserve``) -- and the V rows of logits are averaged on the device (``ttnet_mean_views``).  Metrics, top-k and
    per-class counters see ``[n, n_classes]`` as ever.  ``table_usage=True`` then counts the lookups of ALL ``n * V``
    crops: that is how more views widen what a usage run sees.  ``care=`` with ``views`` raises ValueError (the miss rows
    would be per crop, not per image), and so does a float or already-cropped uint8 tensor batch (RuntimeError: there is
    no image left to cut other views from); ``forward=`` with ``views`` raises ValueError as well, since a forward of
    the caller's own decides its views itself.  ``views=None``: nothing changes."""
    if views is not None and views not in ("flip", "five", "ten"):
        raise ValueError(f"views must be None, \"flip\", \"five\" or \"ten\", got {views!r}")
    if views is not None and care is not None:
        raise ValueError("evaluate(care=, views=): the care-set misses are counted per forwarded crop, V rows per image; "
                         "evaluate the care set with views=None")
    if views is not None and forward is not None:
        raise ValueError("evaluate(forward=, views=): a forward of the caller's own decides its views itself")
    if topk < 0 or topk > _lib.TOPK_MAX:
        raise ValueError(f"topk must be in [0, {_lib.TOPK_MAX}], got {topk}")
    per_class = per_class or confusion
    if per_class and (metrics != "device" or device.type != "cuda"):
        raise RuntimeError(f"evaluate(per_class / confusion) needs metrics=\"device\" on a HIP device, got metrics={metrics!r} on "
                           f"{device}: the per-class counters are kept by the device metrics, which have no CPU path")
    if metrics not in ("torch", "device"):
        raise ValueError(f"metrics must be \"torch\" or \"device\", got {metrics!r}")
    if metrics == "device" and device.type != "cuda":
        raise RuntimeError(f"evaluate(metrics=\"device\") needs a HIP device, got {device}: the device metrics have no "
                           "CPU path (use metrics=\"torch\")")
    model.eval()
    inner = getattr(model, "module", model)              # (nn.DataParallel wrapper, main.py:192)
    if table_usage and not all(hasattr(inner, a) for a in ("count_table_usage", "add_table_usage", "table_usage")):
        raise RuntimeError(f"evaluate(table_usage=True): {type(inner).__name__} keeps no truth-table usage counters (it needs "
                           "count_table_usage / add_table_usage / table_usage, as the TTNet models have)")
    if care is not None and not all(hasattr(inner, a) for a in ("set_care", "care_misses", "care_blocks")):
        raise RuntimeError(f"evaluate(care=): {type(inner).__name__} keeps no care sets (it needs set_care / care_misses / "
                           "care_blocks, as the TTNet models have)")
    use_lanes = inflight > 1 and device.type == "cuda" and hasattr(model, "set_lanes")
    lanes = inflight if use_lanes else 1
    if use_lanes:
        model.set_lanes(inflight)
    streams = [torch.cuda.Stream(device) for _ in range(lanes)] if use_lanes else []
    acc = _OnDeviceMetrics(device, lanes, streams, per_class, confusion) if metrics == "device" else _TorchMetrics()
    asked_k = topk
    if care is not None:
        topk = max(topk, 5)                                # (the hits behind the bounds are read from the records)
        inner.set_care(care, care_min_count)
        cares = _Care(lanes)
    top = _TopK(topk, lanes) if topk else None
    usage_plan = None
    if table_usage:
        inner.count_table_usage(True)
        if getattr(inner, "_plans", None):               # (a plan made later starts from zeroed counters)
            inner.reset_table_usage()
            usage_plan = inner._any_plan()
        for s in streams:                                 # zeroed on the current stream before any lane's stream adds
            s.wait_stream(torch.cuda.current_stream(device))
    labelled = None                                        # True / False once the first batch has been seen
    seen = set()                                           # "ragged", "jpeg": which sticky counts to check at the end

    def run(inputs, lane: Optional[int]):
        """The forward the batch type asks for; ``lane`` None: the model is called as ``model(x)``."""
        if forward is not None:
            return forward(model, inputs, lane or 0)
        if isinstance(inputs, torch.Tensor):
            if views is not None:
                raise RuntimeError(f"evaluate(views={views!r}) needs RaggedU8 or RaggedJpeg batches (whole images to cut the "
                                   f"views from), got a {inputs.dtype} tensor {tuple(inputs.shape)}")
            if inputs.dtype == torch.uint8:
                return model.forward_u8(inputs, lane=lane or 0)
            return model(inputs) if lane is None else model(inputs, lane=lane)
        from . import jpeg, preprocess                    # (not needed by the float path)
        if isinstance(inputs, jpeg.RaggedJpeg):
            seen.update(("jpeg", "ragged"))
            if views is not None:
                return jpeg.jpeg_views_forward(model, inputs, views, lane=lane or 0)
            return jpeg.jpeg_eval_forward(model, inputs, lane=lane or 0)
        if isinstance(inputs, preprocess.RaggedU8):
            seen.add("ragged")
            if views is not None:
                return preprocess.imgnet_views_forward(model, inputs, views, lane=lane or 0)
            return preprocess.imgnet_eval_forward(model, inputs, lane=lane or 0)
        raise RuntimeError(f"evaluate: no forward for a batch of type {type(inputs).__name__}; pass forward=")

    def log(index: int, when: str):
        if acc.logs == when and index % log_every == 0:
            print("Loss: %.3f | Acc1: %.3f%% Acc5: %.3f%% " % acc.running(), flush=True)

    pending = []                                           # batches in flight, oldest first: (index, event, metrics, images)

    def retire():
        index, event, batch, n, kept, care_kept = pending.pop(0)
        if event is not None:
            event.synchronize()
        if labelled:
            acc.retire(batch, n)
        if top is not None:
            top.retire(kept)
        if care is not None:
            cares.retire(care_kept[0], top.parts[-1], care_kept[1])
        if log_every and labelled:
            log(index, "retired")

    for i, (inputs, targets) in enumerate(batches):
        lane = i % lanes
        if len(pending) == lanes:                          # this lane's previous batch still owns its workspace
            retire()
        with torch.cuda.stream(streams[lane]) if use_lanes else contextlib.nullcontext():
            if labelled is None:
                labelled = targets is not None
                if not labelled and top is None:
                    raise ValueError("evaluate: batches without targets need topk > 0 (there is nothing else to compute)")
                if not labelled and per_class:
                    raise ValueError("evaluate: per_class / confusion need targets")
            elif labelled != (targets is not None):
                raise ValueError(f"evaluate: batch {i} mixes labelled and unlabelled batches")
            inputs = inputs.to(device, non_blocking=True)
            if labelled:
                targets = targets.to(device, non_blocking=True)
            outputs = run(inputs, lane if use_lanes else None)
            if table_usage:
                inner.add_table_usage(lane)
                if usage_plan is None:
                    usage_plan = inner._any_plan()
                elif usage_plan is not inner._any_plan():
                    raise RuntimeError("evaluate(table_usage=True): the plan was rebuilt for a larger batch and its counters "
                                       "started again; call model.reserve(<largest batch>) first")
            batch = kept = care_kept = None
            if care is not None:
                care_kept = (cares.add(inner, lane, use_lanes), targets if labelled else None)
            if top is None:
                batch = acc.add(outputs, targets, lane)
            else:
                kept, rec = top.add(outputs, lane, use_lanes)
                if labelled:
                    batch = acc.add_with_topk(outputs, targets, lane, rec)
            event = torch.cuda.Event() if use_lanes else None
            if use_lanes:
                event.record(streams[lane])
        pending.append((i, event, batch, inputs.size(0) if isinstance(inputs, torch.Tensor) else len(inputs), kept,
                        care_kept))
        if not use_lanes:                                  # nothing in flight: read the batch now, as the reference does
            retire()
        if log_every and labelled:
            log(i, "issued")
    while pending:
        retire()
    # the range flag of the split operands is reported on the next call of a plan: without this, an overflow in the
    # last (or only) batch would end in silently invalid metrics
    if hasattr(inner, "check_range"):
        inner.check_range()
    if "jpeg" in seen:                                    # likewise: a corrupt file decodes as zeros and is only counted
        from . import jpeg
        jpeg.check_jpeg(device)
    if "ragged" in seen:
        from . import preprocess
        preprocess.check_ragged(device)
    if labelled is False:                                  # no labels: the predictions are the result
        res = EvalResult(None, None, None, sum(len(p) for p in top.parts))
    else:
        res = acc.result()
    if asked_k:
        res.predictions = top.result()
        if asked_k < topk:
            pr = res.predictions
            res.predictions = Predictions(pr.classes[:, :asked_k], pr.logit[:, :asked_k], pr.logprob[:, :asked_k])
    if care is not None:
        res.care = cares.result(inner.care_blocks)
    if table_usage:
        res.table_usage = inner.table_usage()             # (synchronises the device)
    if labelled is not False:
        print("Acc..", res.top1, res.top5)
    if care is not None:
        print(res.care.line())
    return res
