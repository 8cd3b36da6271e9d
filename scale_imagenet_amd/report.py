"""The files the commands write: per-image predictions (CSV), per-class counters (CSV), the confusion matrix (.npy).

Formats (fixed: tests and users' scripts read them):
  predictions  ``path,target,class_1,logprob_1,...,class_K,logprob_K``; ``target`` is empty for an unlabelled image;
               floats are written with ``repr()`` and so read back to the same bits; with class names ``target`` and
               ``class_i`` are names, otherwise indices (a row with a NaN has class -1, whatever the names).
  per class    ``class,images,hits1,hits5,predicted,acc1,acc5`` from the int64 ``[n_classes, 4]`` counters of
               ``ttnet_class_counts``; ``acc`` in percent, empty for a class without images.
  confusion    ``numpy.save`` of the int64 ``[n_classes, n_classes]`` matrix, indexed ``[target][top-1 class]``.
  table usage  ``numpy.savez_compressed``: one int64 ``[groups, 2^n]`` array per ``Block_TT`` name (``EvalResult.table_usage``).
  coverage     ``block,groups,inputs,entries,seen,share_seen,constant_groups,top1pct_share`` per ``Block_TT``
               (``coverage_rows``).
  gates        ``block,inputs,filters,constant,dnf_cubes,dnf_literals,cnf_cubes,cnf_literals,constant_seen,dnf_cubes_seen,
               dnf_literals_seen,cnf_cubes_seen,cnf_literals_seen`` per binarised ``Block_TT`` (``gate_rows``): the counts of
               ``model.gate_counts()`` on the full care set and, under ``*_seen``, with the entries the run never read as
               don't-cares.  Prime, irredundant covers, not minimum ones.
  care rows    ``index,covered,<one column per Block_TT>``: per image in dataset order, whether it is covered (1: no miss
               in any block) and its care-set misses per block (``evaluate.CareResult.rows``).
  care summary ``block,lookups,misses,images_with_misses`` per ``Block_TT`` and a last row ``total`` whose
               ``images_with_misses`` is the number of images that are not covered (``care_summary_rows``).
  rule support ``block,inputs,form,functions,cubes,literals,top1pct_first_share,top10pct_first_share,unused_cubes`` per binarised
               ``Block_TT`` (``rule_support_rows``), from ``model.rule_support``; with a pruning share also ``kept_cubes,
               kept_literals,lost_share,lost_patterns``.
Every file is written to a temporary name beside its own and then renamed, so a reader never sees half of one.
"""
from __future__ import annotations

import contextlib
import csv
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np


def read_class_names(path: str) -> List[str]:
    """One name per line (the line's text without its line end; empty lines at the end of the file are dropped)."""
    with open(path, encoding="utf-8") as f:
        names = [line.rstrip("\r\n") for line in f]
    while names and not names[-1]:
        names.pop()
    return names


@contextlib.contextmanager
def replacing(path: Optional[str], mode: str = "w"):
    """A file that becomes ``path`` when the block ends well; ``path`` None: standard output."""
    if path is None:
        yield sys.stdout.buffer if "b" in mode else sys.stdout
        sys.stdout.flush()
        return
    tmp = f"{path}.tmp{os.getpid()}"
    kw = {} if "b" in mode else {"newline": "", "encoding": "utf-8"}
    try:
        with open(tmp, mode, **kw) as f:
            yield f
        os.replace(tmp, path)
    except BaseException:
        with contextlib.suppress(OSError):
            os.remove(tmp)
        raise


def write_csv(path: Optional[str], rows):
    """``rows`` (header first) as CSV (``path`` None: standard output); written to a temporary name and renamed."""
    with replacing(path) as f:
        csv.writer(f, lineterminator="\n").writerows(rows)


def _name(index: int, names: Optional[Sequence[str]]) -> str:
    if names is None or index < 0:
        return str(int(index))
    if index >= len(names):
        raise ValueError(f"class {index} has no name: the class list has {len(names)} lines")
    return names[index]


def write_predictions_csv(path: Optional[str], paths: Sequence[str], targets: Optional[Sequence[int]], pred,
                          names: Optional[Sequence[str]] = None, covered=None):
    """``pred``: ``evaluate.Predictions`` of ``len(paths)`` images in the order of ``paths``; ``targets`` None: unlabelled.
    ``covered`` (bool per image, ``evaluate.CareResult.covered``) adds a last column ``covered`` of 0 / 1."""
    if len(pred) != len(paths) or (targets is not None and len(targets) != len(paths)):
        raise ValueError(f"{len(paths)} paths, {len(pred)} predictions, {None if targets is None else len(targets)} targets")
    if covered is not None and len(covered) != len(paths):
        raise ValueError(f"{len(paths)} paths, {len(covered)} covered flags")
    k = pred.k
    with replacing(path) as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["path", "target"] + [c for i in range(1, k + 1) for c in (f"class_{i}", f"logprob_{i}")] +
                   (["covered"] if covered is not None else []))
        for n, p in enumerate(paths):
            row = [p, "" if targets is None else _name(int(targets[n]), names)]
            for i in range(k):
                row += [_name(int(pred.classes[n, i]), names), repr(float(pred.logprob[n, i]))]
            if covered is not None:
                row.append(int(bool(covered[n])))
            w.writerow(row)


def write_care_rows_csv(path: Optional[str], care):
    """``care``: ``evaluate.CareResult``."""
    rows, covered = np.asarray(care.rows), care.covered
    with replacing(path) as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["index", "covered"] + list(care.blocks))
        for i in range(rows.shape[0]):
            w.writerow([i, int(covered[i])] + rows[i].tolist())


def read_care_rows_csv(path: str) -> Tuple[List[str], np.ndarray, np.ndarray]:
    """``(blocks, covered bool [N], rows int32 [N, B])`` as written."""
    with open(path, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    head, lines = lines[0], lines[1:]
    if head[:2] != ["index", "covered"] or [r[0] for r in lines] != [str(i) for i in range(len(lines))]:
        raise ValueError(f"{path}: not a care rows file (header {head})")
    blocks = head[2:]
    rows = np.array([[int(v) for v in r[2:]] for r in lines], dtype=np.int32).reshape(len(lines), len(blocks))
    return blocks, np.array([r[1] == "1" for r in lines], dtype=bool), rows


def care_summary_rows(care, lookups_per_image) -> List[list]:
    """The rows of the care summary, header first.  ``lookups_per_image``: ``{Block_TT name: groups * Ho * Wo}``
    (``model.care_lookups()``), the lookups one image makes in that block."""
    n = len(care.rows)
    out = [["block", "lookups", "misses", "images_with_misses"]]
    misses, images = care.misses, care.images_with_misses
    for name in care.blocks:
        out.append([name, n * int(lookups_per_image[name]), misses[name], images[name]])
    out.append(["total", sum(r[1] for r in out[1:]), sum(r[2] for r in out[1:]), n - care.covered_images])
    return out


def write_care_summary_csv(path: Optional[str], care, lookups_per_image):
    write_csv(path, care_summary_rows(care, lookups_per_image))


def read_predictions_csv(path: str) -> Tuple[List[str], List[str], List[List[str]], np.ndarray]:
    """``(paths, targets, classes, logprob)``: targets and classes as written (names or indices, "" for no target),
    ``logprob`` float64 ``[N, K]`` with the bits that were written."""
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    head, rows = rows[0], rows[1:]
    if head[-1:] == ["covered"]:                          # (the optional last column of a run with a care set)
        head, rows = head[:-1], [r[:-1] for r in rows]
    k = (len(head) - 2) // 2
    if head != ["path", "target"] + [c for i in range(1, k + 1) for c in (f"class_{i}", f"logprob_{i}")]:
        raise ValueError(f"{path}: not a predictions file (header {head})")
    logprob = np.array([[float(r[3 + 2 * i]) for i in range(k)] for r in rows], dtype=np.float64).reshape(len(rows), k)
    return [r[0] for r in rows], [r[1] for r in rows], [[r[2 + 2 * i] for i in range(k)] for r in rows], logprob


def per_class_rows(counts: np.ndarray, names: Optional[Sequence[str]] = None) -> List[list]:
    """The rows of the per-class file, header first."""
    rows = [["class", "images", "hits1", "hits5", "predicted", "acc1", "acc5"]]
    for c, (images, hits1, hits5, predicted) in enumerate(np.asarray(counts, dtype=np.int64).tolist()):
        acc = [repr(100.0 * h / images) if images else "" for h in (hits1, hits5)]
        rows.append([_name(c, names), images, hits1, hits5, predicted] + acc)
    return rows


def write_per_class_csv(path: Optional[str], counts: np.ndarray, names: Optional[Sequence[str]] = None):
    write_csv(path, per_class_rows(counts, names))


def write_confusion(path: str, confusion: np.ndarray):
    with replacing(path, "wb") as f:
        np.save(f, np.ascontiguousarray(confusion, dtype=np.int64))


def save_table_usage(path: str, usage) -> None:
    """``{Block_TT name: int64 [groups, 2^n]}`` -> a compressed ``.npz`` with one array per block name."""
    with replacing(path, "wb") as f:
        np.savez_compressed(f, **{k: np.ascontiguousarray(v, dtype=np.int64) for k, v in usage.items()})


def load_table_usage(path: str):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def coverage_rows(usage, tables=None) -> List[list]:
    """The rows of the coverage file, header first; one row per ``Block_TT`` of ``usage``:
      entries          table entries of the block (groups x 2^n)
      seen             entries looked up at least once
      share_seen       seen / entries
      constant_groups  groups whose output never varies on the entries seen (a group without a lookup counts); needs
                       ``tables`` (``{name: model.get_table(name)}``, [groups, 2^n, cout_g]), empty without
      top1pct_share    share of all lookups that fall on the 1 % most used entries of their group (at least one entry per
                       group), summed over the groups: 1.0 for a block whose every group reads a single entry"""
    rows = [["block", "groups", "inputs", "entries", "seen", "share_seen", "constant_groups", "top1pct_share"]]
    for name, u in usage.items():
        u = np.asarray(u, dtype=np.int64)
        groups, size = u.shape
        seen = u > 0
        k = max(1, size // 100)
        top = np.sort(u, axis=1)[:, size - k:].sum()
        total = int(u.sum())
        constant = ""
        if tables is not None and name in tables:
            t = np.asarray(tables[name])
            constant = 0
            for g in range(groups):
                used = t[g][seen[g]]
                constant += int(len(used) == 0 or bool((used == used[0]).all()))
        rows.append([name, groups, int(size).bit_length() - 1, groups * size, int(seen.sum()),
                     repr(float(seen.sum()) / (groups * size)), constant, repr(float(top) / total) if total else ""])
    return rows


def write_coverage_csv(path: Optional[str], usage, tables=None):
    write_csv(path, coverage_rows(usage, tables))


GATE_FIELDS = ["constant", "dnf_cubes", "dnf_literals", "cnf_cubes", "cnf_literals"]


def gate_rows(full, seen, inputs) -> List[list]:
    """The rows of the gates file, header first.  ``full`` / ``seen``: ``model.gate_counts()`` /
    ``model.gate_counts(usage)``; ``inputs``: ``{block name: n}``."""
    rows = [["block", "inputs", "filters"] + GATE_FIELDS + [f + "_seen" for f in GATE_FIELDS]]
    for name, a in full.items():
        rows.append([name, int(inputs[name]), int(a["filters"])] + [int(a[f]) for f in GATE_FIELDS] + [int(seen[name][f]) for f in GATE_FIELDS])
    return rows


def write_gates_csv(path: Optional[str], full, seen, inputs):
    write_csv(path, gate_rows(full, seen, inputs))


RULE_FIELDS = ["block", "inputs", "form", "functions", "cubes", "literals", "top1pct_first_share", "top10pct_first_share", "unused_cubes"]
RULE_PRUNED_FIELDS = ["kept_cubes", "kept_literals", "lost_share", "lost_patterns"]


def rule_support_rows(support, pruned=None) -> List[list]:
    """The rows of the rule support file, header first; one row per block of ``support`` (``model.rule_support``):
      functions             filters of the block, each with a cover of its own
      cubes, literals       of all those covers (a constant filter has no cube, or the one cube without a literal)
      top1pct_first_share   share of the covered lookups decided by the 1 % of the block's cubes with the largest ``first``
                            (at least one cube): read as decision lists, so few rules settle that much of the data; empty for
                            a block without a covered lookup
      top10pct_first_share  the same for the top 10 %
      unused_cubes          cubes with ``hits == 0``: only patterns that were never looked up justify them
    and, with ``pruned`` (``{block: rules.prune_by_share(..)}``):
      kept_cubes, kept_literals  what stays of the covers
      lost_share            lookups that only dropped cubes hold / all lookups of the block's functions
      lost_patterns         table entries that only dropped cubes hold, summed over the functions (looked up or not)"""
    from . import minimise
    rows = [RULE_FIELDS + (RULE_PRUNED_FIELDS if pruned is not None else [])]
    for name, s in support.items():
        first = np.sort(np.concatenate([np.asarray(a, dtype=np.int64) for a in s["first"]] + [np.zeros(0, dtype=np.int64)]))[::-1]
        covered = int(first.sum())
        shares = [repr(float(first[: max(1, len(first) // d)].sum()) / covered) if covered else "" for d in (100, 10)]
        row = [name, int(s["n"]), s.get("form", "dnf"), len(s["cubes"]), int(sum(len(c) for c in s["cubes"])),
               int(sum(minimise.literal_total(c) for c in s["cubes"])), shares[0], shares[1],
               int(sum(int((np.asarray(h) == 0).sum()) for h in s["hits"]))]
        if pruned is not None:
            p = pruned[name]
            kept = [np.asarray(c, dtype=np.uint32)[np.asarray(k, dtype=bool)] for c, k in zip(s["cubes"], p["keep"])]
            lookups = int(np.asarray(s["row_total"], dtype=np.int64).sum())
            row += [int(sum(len(c) for c in kept)), int(sum(minimise.literal_total(c) for c in kept)),
                    repr(float(int(p["totals"][:, 1].sum())) / lookups) if lookups else "", int(p["totals"][:, 3].sum())]
        rows.append(row)
    return rows


def write_rule_support_csv(path: Optional[str], support, pruned=None):
    write_csv(path, rule_support_rows(support, pruned))
