"""Rule support: which cubes of a cover the data uses, and what it costs to drop the rest.

A cover (``minimise.minimise_device``: uint32 keys ``mask << 16 | value``, in order) says WHAT a function computes;
``model.table_usage()`` says how often every pattern was looked up.  Joined, with ``u[p]`` the lookups of pattern p and the
cubes that are kept taken in their order (``include/ttnet.h``, ``ttnet_cover_support``):

  ``hits[c]``   the lookups cube c holds;
  ``first[c]``  the lookups for which c is the first kept cube that holds them: a partition of the covered lookups;
  ``sole[c]``   the lookups that c alone holds: exactly those whose output bit changes if c is removed;
  ``totals``    per function ``covered, lost, used_patterns, lost_patterns``: the lookups some kept cube holds, the lookups
                only dropped cubes hold, the patterns with a lookup, the patterns only dropped cubes hold (looked up or not);
  ``lost_bits`` the bitmap of those lost patterns (``minimise.pack_bits``).

It exists twice with the same integers: ``cover_support`` (the HIP kernel of ``csrc/rules.hip``, all functions of a batch
in one launch) and ``cover_support_cpu`` (numpy, on ``minimise.cube_patterns``: slow, for tests and tools, never a fallback).
``keep_by_support`` turns hits into keep flags, ``care_after_prune`` turns the lost patterns of a pruned block into the care
sets ``model.set_care`` takes: an image without a miss on them gets the same logits from the pruned covers as from the
tables.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import minimise

TOTALS = ("covered", "lost", "used_patterns", "lost_patterns")     # the columns of ``totals``


def _check_inputs(cubes, usage_shape, usage_row_of, n: int, keep):
    minimise._check_n(n)
    if len(usage_shape) != 2 or usage_shape[1] != 1 << n:
        raise ValueError(f"usage_rows has shape {tuple(usage_shape)}, expected [rows, {1 << n}]")
    if len(cubes) < 1 or len(usage_row_of) != len(cubes):
        raise ValueError(f"{len(cubes)} covers (at least one is needed), {len(usage_row_of)} usage row indices")
    if keep is not None:
        if len(keep) != len(cubes) or any(len(k) != len(c) for k, c in zip(keep, cubes)):
            raise ValueError("keep must hold one flag per cube of every cover")


def _result(hits, first, sole, totals, lost, bad_rows, row_total, usage_row_of, n):
    return dict(hits=hits, first=first, sole=sole, totals=totals, lost_bits=lost, bad_rows=int(bad_rows),
                row_total=row_total, usage_row_of=np.asarray(usage_row_of, dtype=np.int32), n=int(n))


def _row_totals(sums: np.ndarray, usage_row_of) -> np.ndarray:
    """All lookups of every function's usage row (``sums``: per row), 0 for a row index out of range."""
    return np.array([sums[r] if 0 <= r < len(sums) else 0 for r in np.asarray(usage_row_of).tolist()], dtype=np.int64)


def cover_support_cpu(cubes: Sequence[np.ndarray], usage_rows, usage_row_of, n: int, keep=None, lost_bits: bool = False) -> dict:
    """The numpy twin of ``cover_support``: the same arguments (no device) and the same result, integer for integer."""
    usage_rows = np.asarray(usage_rows, dtype=np.int64)
    _check_inputs(cubes, usage_rows.shape, usage_row_of, n, keep)
    size = 1 << n
    hits, first, sole = [], [], []
    totals = np.zeros((len(cubes), 4), dtype=np.int64)
    lost = np.zeros((len(cubes), minimise.n_words(n)), dtype=np.uint32) if lost_bits else None
    bad = 0
    for f, keys in enumerate(cubes):
        keys = np.asarray(keys, dtype=np.uint32)
        h, fi, so = (np.zeros(len(keys), dtype=np.int64) for _ in range(3))
        hits.append(h), first.append(fi), sole.append(so)
        row = int(usage_row_of[f])
        if not 0 <= row < usage_rows.shape[0]:
            bad += 1
            continue
        if ((keys & 0xFFFF) & ~(keys >> 16)).any() or (keys >> 16 >= size).any():
            raise ValueError(f"cover {f} has a malformed key for n = {n}")
        u = usage_rows[row]
        kept = np.ones(len(keys), dtype=bool) if keep is None else np.asarray(keep[f]) != 0
        times = np.zeros(size, dtype=np.int64)                       # kept cubes that hold the pattern
        held = np.zeros(size, dtype=bool)                            # some cube of the full list holds it
        lead = np.full(size, -1, dtype=np.int64)                     # its first kept cube
        for c, pts in enumerate(minimise.cube_patterns(keys, n)):
            held[pts] = True
            if not kept[c]:
                continue
            h[c] = u[pts].sum()
            lead[pts[times[pts] == 0]] = c
            times[pts] += 1
        np.add.at(fi, lead[times > 0], u[times > 0])
        np.add.at(so, lead[times == 1], u[times == 1])
        gone = held & (times == 0)
        totals[f] = (u[times > 0].sum(), u[gone].sum(), np.count_nonzero(u > 0), np.count_nonzero(gone))
        if lost is not None:
            lost[f] = minimise.pack_bits(gone)
    return _result(hits, first, sole, totals, lost, bad, _row_totals(usage_rows.sum(axis=1, dtype=np.int64), usage_row_of), usage_row_of, n)


def launch_cover_support(cubes_t, counts_t, keep_t, usage_t, rows_t, n: int, hits_t, first_t, sole_t, totals_t, lost_t, work_t):
    """One ``ttnet_cover_support`` on the current stream of the tensors' device: every argument a tensor already there (``keep_t``
    and ``lost_t`` may be None), nothing allocated, nothing synchronised, so a graph can capture it.  ``cubes_t`` is
    ``[functions, cube_cap]``; the caller has checked the counts against the cap."""
    import torch

    from . import _lib
    lib = _lib.load()
    ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())             # noqa: E731
    _lib.check(lib.ttnet_cover_support(ptr(cubes_t), ptr(counts_t), cubes_t.shape[1], ptr(keep_t), ptr(usage_t), ptr(rows_t),
                                       usage_t.shape[0], n, cubes_t.shape[0], ptr(hits_t), ptr(first_t), ptr(sole_t), ptr(totals_t),
                                       ptr(lost_t), ptr(work_t), work_t.numel() * work_t.element_size(),
                                       C.c_void_p(torch.cuda.current_stream(cubes_t.device).cuda_stream)))


def cover_support(cubes: Sequence[np.ndarray], usage_rows, usage_row_of, n: int, keep=None, device=None,
                  lost_bits: bool = False) -> dict:
    """What every cube of every cover carries, by ``ttnet_cover_support``, one launch for the batch.

    ``cubes``: F arrays of uint32 keys, as ``minimise.minimise_device`` returns them.  ``usage_rows``: int64 ``[R, 2^n]``
    lookup counts (numpy, or a tensor on the device), ``usage_row_of``: F row indices -- function f is weighed with row
    ``usage_row_of[f]``; the ``cout_g`` filters of a group share theirs.  ``keep``: F arrays of flags, one per cube (None: every
    cube is kept).  Returns ``{hits, first, sole}`` (lists of F int64 arrays, one value per cube; 0 for a dropped cube),
    ``totals`` int64 ``[F, 4]`` (``TOTALS``), ``lost_bits`` uint32 ``[F, words]`` when asked for (else None), ``row_total`` int64
    ``[F]`` (all lookups of the function's row), ``bad_rows`` (functions whose row index is out of range: their outputs are
    zero) and ``usage_row_of`` / ``n`` as given."""
    import torch

    from . import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if isinstance(usage_rows, torch.Tensor):
        usage_t = usage_rows.to(dev).contiguous()
        if usage_t.dtype != torch.int64:
            raise ValueError(f"usage_rows must be int64, got {usage_t.dtype}")
    else:
        usage_t = torch.from_numpy(np.ascontiguousarray(usage_rows, dtype=np.int64)).to(dev)
    _check_inputs(cubes, tuple(usage_t.shape), usage_row_of, n, keep)
    total = len(cubes)
    counts = np.array([len(c) for c in cubes], dtype=np.int32)
    cap = max(int(counts.max()), 1)                                  # counts <= cap by construction: the check the C call leaves to us
    packed = np.zeros((total, cap), dtype=np.uint32)
    flags = None if keep is None else np.zeros((total, cap), dtype=np.uint8)
    for f, keys in enumerate(cubes):
        packed[f, : counts[f]] = np.asarray(keys, dtype=np.uint32)
        if flags is not None:
            flags[f, : counts[f]] = np.asarray(keep[f]) != 0
    rows = np.ascontiguousarray(usage_row_of, dtype=np.int32)
    with torch.cuda.device(dev):
        cubes_t = torch.from_numpy(packed.view(np.int32)).to(dev)
        counts_t = torch.from_numpy(counts).to(dev)
        keep_t = None if flags is None else torch.from_numpy(flags).to(dev)
        rows_t = torch.from_numpy(rows).to(dev)
        out = torch.empty((3, total, cap), dtype=torch.int64, device=dev)
        totals_t = torch.empty((total, 4), dtype=torch.int64, device=dev)
        lost_t = torch.empty((total, minimise.n_words(n)), dtype=torch.int32, device=dev) if lost_bits else None
        work = torch.empty(_lib.check(lib.ttnet_cover_support_workspace(n, total)), dtype=torch.uint8, device=dev)
        launch_cover_support(cubes_t, counts_t, keep_t, usage_t, rows_t, n, out[0], out[1], out[2], totals_t, lost_t, work)
        got = out.cpu().numpy()
        bad = int(work[:8].cpu().numpy().view(np.int64)[0])
        row_total = _row_totals(usage_t.sum(dim=1).cpu().numpy(), rows)
    per = [[got[k, f, : counts[f]].copy() for f in range(total)] for k in range(3)]
    lost = None if lost_t is None else np.ascontiguousarray(lost_t.cpu().numpy()).view(np.uint32)
    return _result(per[0], per[1], per[2], totals_t.cpu().numpy(), lost, bad, row_total, rows, n)


def keep_by_support(support: dict, min_hits: Optional[int] = None, min_share: Optional[float] = None) -> List[np.ndarray]:
    """Keep flags (one bool array per function) from the ``hits`` of a support result: a cube stays iff it holds at least
    ``min_hits`` lookups and at least the share ``min_share`` of all lookups of its function's usage row (``hits / row_total``;
    a row without a lookup gives every cube the share 0).  A share of 0 keeps every cube, a share above 1 none."""
    if min_hits is None and min_share is None:
        raise ValueError("keep_by_support needs min_hits or min_share")
    if min_share is not None and not min_share >= 0:
        raise ValueError(f"min_share must be >= 0, got {min_share!r}")
    out = []
    for h, total in zip(support["hits"], support["row_total"]):
        h = np.asarray(h, dtype=np.int64)
        flags = np.ones(len(h), dtype=bool)
        if min_hits is not None:
            flags &= h >= int(min_hits)
        if min_share is not None:
            flags &= (h / float(total) if total > 0 else np.zeros(len(h))) >= float(min_share)
        out.append(flags)
    return out


def prune_by_share(block: dict, usage_rows, min_share: float, device=None) -> dict:
    """One block of ``model.rule_support`` pruned: the cubes below ``min_share`` (``keep_by_support``) dropped and the support
    of the rest measured again, with the lost patterns; ``cover_support``'s result with the flags under ``keep``."""
    keep = keep_by_support(block, min_share=min_share)
    out = cover_support(block["cubes"], usage_rows, block["usage_row_of"], block["n"], keep, device, lost_bits=True)
    out["keep"] = keep
    return out


def care_after_prune(lost_bits, groups: int, outputs_per_group: int, base_care=None, n: Optional[int] = None) -> np.ndarray:
    """The care set of one block after its covers were pruned: uint32 ``[groups, words]`` (the format of ``model.set_care``) in
    which an entry is kept iff no output function of its group lost it.  ``lost_bits``: uint32 ``[groups * outputs_per_group,
    words]`` from ``cover_support(.., keep=.., lost_bits=True)``, function f = group ``f // outputs_per_group`` as in
    ``minimise.pack_functions``.  ``base_care`` (``minimise.care_masks(usage)[name]``) is ANDed in: needed when the covers were
    made with don't-cares, which they are free to get wrong.  ``n``: the inputs, needed only for n < 5 without ``base_care``
    (one word then holds fewer than 32 patterns)."""
    lost = np.asarray(lost_bits, dtype=np.uint32)
    if lost.ndim != 2 or lost.shape[0] != groups * outputs_per_group:
        raise ValueError(f"lost_bits has shape {tuple(lost.shape)}, expected [{groups * outputs_per_group}, words]")
    words = lost.shape[1]
    any_lost = np.bitwise_or.reduce(lost.reshape(groups, outputs_per_group, words), axis=1)
    if words > 1:
        valid = np.uint32(0xFFFFFFFF)
    elif n is not None:
        valid = np.uint32(0xFFFFFFFF if n >= 5 else (1 << (1 << n)) - 1)
    elif base_care is not None:
        valid = np.uint32(0xFFFFFFFF)                                # (the base's unused bits are zero)
    else:
        raise ValueError("one-word bitmaps: pass n or base_care")
    care = ~any_lost & valid
    if base_care is not None:
        base = np.asarray(base_care, dtype=np.uint32)
        if base.shape != care.shape:
            raise ValueError(f"base_care has shape {tuple(base.shape)}, expected {tuple(care.shape)}")
        care = care & base
    return np.ascontiguousarray(care, dtype=np.uint32)


def block_covers(table_bits: np.ndarray, usage: Optional[np.ndarray], n: int, form: str = "dnf", rounds: int = 0, min_count: int = 1,
                 device=None) -> List[np.ndarray]:
    """The covers ``model.rule_support`` measures: of every filter of a ``get_table`` array (``form`` "dnf"), or of its
    complement ("cnf": every cube a clause, ``minimise.cnf_text``); ``usage`` None: no don't-cares."""
    if form not in ("dnf", "cnf"):
        raise ValueError(f"form {form!r}: 'dnf' or 'cnf'")
    on, dc = minimise.pack_functions(table_bits, usage, min_count)
    if form == "cnf":
        on = minimise.complement(on, dc, n)
    return minimise.minimise_device(on, dc, n, device, rounds=rounds)
