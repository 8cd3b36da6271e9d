"""Truth-table export: the files the reference writes for one ``Block_TT`` filter.

Counterpart of ``Block_TT.get_TT_block_1filter`` / ``for_1_filter`` / ``save_cnf_dnf`` /
``get_expresion_methode1`` and ``get_exp_with_y`` (models/TT_FHE_SMALL.py:251-275, :344-431), fed
from the truth tables the plan built on the GPU (``model.get_table``, canonical order: pattern =
index read MSB first over (c, kh, kw), TT_FHE_SMALL.py:330-334) instead of a float forward over
all 2^n patterns.  For every non-constant filter:

    Truth_Table_block{B}_filter_{f}_coefdefault_{v}_sousblock_{S}.csv   index, the n input bits, the filter's column
    DNF_expression_block{B}_filter_{f}_coefdefault_{v}_sousblock_{S}.txt   minimal sum of products (sympy SOPform)
    CNF_expression_block{B}_filter_{f}_coefdefault_{v}_sousblock_{S}.txt   minimal product of sums (sympy POSform)
    table_outputblock_{B}_filter_{f}_coefdefault_{v}.txt                    CNF of (y <-> filter), the SAT-solver form

Expressions are produced for n <= ``max_expr_bits`` inputs (the reference: n in {4, 8, 9} only);
for the 16-input tables of TT-small only the CSV is practical.  Unlike the reference's exporter,
grouped blocks (several input channels per group) work too: the table of group g is used for
its filters.  Host-side Python (pandas + sympy), not a hot path.

Don't-care terms: with ``usage`` (the lookup counts of ``model.table_usage()`` / ``evaluate(..., table_usage=True)``,
int64 [2^n] per group, canonical order) a pattern that no image produced (count 0) is a don't-care of the
minimisation: it goes to ``SOPform`` / ``POSform`` as ``dontcares``, so the expressions agree with the table on every
pattern seen and are free elsewhere, which makes them smaller.  The CSV gains a ``count`` column, and a filter that is
constant on the patterns seen is written as that constant.  ``dnf_literals`` / ``cnf_literals`` of the returned record
are the literal counts of the two forms, to report the saving.  With ``usage=None`` every file is what it was.

Minimiser: ``minimiser="sympy"`` (the default) is the path above and writes what it always wrote.  ``"device"`` and ``"cpu"``
take the expressions from ``scale_imagenet_amd.minimise`` instead -- the HIP kernel, or its numpy twin -- for every
n <= 16, so the 16-input tables of TT-small get their DNF / CNF / SAT-form files too; ``export_block`` minimises all its
filters, both forms, in ONE device call.  Those covers are prime and irredundant, not minimum: an expression can carry more
literals than sympy's for the same function (``profiles/minimise_bench.txt`` has the measured ratio).  ``rounds`` (0 .. 8,
default 0: what it always was) adds that many reduce / expand rounds to "device" and "cpu", which shrink the covers
(``profiles/minimise_rounds_bench.txt``: ratios and times per round count); "sympy" ignores it.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, List, Optional

import numpy as np


def pattern_frame(n: int):
    """Index column + the n input bits of every pattern, MSB first (TT_FHE_SMALL.py:330-332)."""
    import pandas as pd
    idx = np.arange(2 ** n, dtype=np.int64)
    bits = ((idx[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.int64)
    return pd.DataFrame(bits).reset_index()


def minimal_forms(minterms: List[int], n: int, dontcares: Optional[List[int]] = None):
    """(DNF, CNF) of the function that is 1 exactly on ``minterms`` (TT_FHE_SMALL.py:405-427); on ``dontcares`` either
    form may take either value."""
    from sympy import symbols
    from sympy.logic import POSform, SOPform
    xs = symbols(", ".join(f"x_{i}" for i in range(n)))
    xs = list(xs) if n > 1 else [xs]
    if dontcares:
        return SOPform(xs, minterms=minterms, dontcares=dontcares), POSform(xs, minterms=minterms, dontcares=dontcares)
    return SOPform(xs, minterms=minterms), POSform(xs, minterms=minterms)


def cnf_with_output(dnf, cnf) -> str:
    """CNF of ``y <-> f`` in the reference's text format (TT_FHE_SMALL.py:251-275): one clause
    ``(y | ~l1 | ~l2 ...)`` per DNF term (term -> y) and ``(clause | ~y)`` per CNF clause."""
    def lits(text: str, sep: str) -> List[str]:
        return [t for t in text.replace("(", "").replace(")", "").split(sep) if t]

    dnf_s, cnf_s = str(dnf).replace(" ", ""), str(cnf).replace(" ", "")
    clauses = []
    for term in dnf_s.split("|"):
        neg = [l[1:] if l.startswith("~") else "~" + l for l in lits(term, "&")]
        clauses.append("(y | " + " | ".join(neg) + ")")
    for clause in cnf_s.split("&"):
        clauses.append("(" + " | ".join(lits(clause, "|")) + " | ~y)")
    return " & ".join(clauses)


def export_filter(column: np.ndarray, n: int, filter_index: int, out_dir: str, block: int, sub_block: int,
                  max_expr_bits: int = 9, usage: Optional[np.ndarray] = None, minimiser: str = "sympy", device=None,
                  forms=None, rounds: int = 0, min_count: int = 1) -> Dict[str, Optional[str]]:
    """Files for one filter.  ``column``: its 2^n table entries (0/1), canonical order.  ``usage``: the lookup counts of
    the filter's group, int64 [2^n] (module docstring).  ``minimiser``: module docstring; ``forms``: this filter's
    ``(DNF text, CNF text)`` when ``export_block`` has minimised it already.  ``rounds``: module docstring (ignored by
    "sympy").  ``min_count``: an entry looked up fewer times than this is a don't-care (default 1: the entries never read)."""
    import pandas as pd
    if minimiser not in ("sympy", "device", "cpu"):
        raise ValueError(f"minimiser {minimiser!r}: 'sympy', 'device' or 'cpu'")
    os.makedirs(out_dir, exist_ok=True)
    col = np.asarray(column).astype(np.float32)
    uniq = np.unique(col)
    prefix = os.path.join(out_dir, "")
    out: Dict[str, Optional[str]] = {"dnf": None, "cnf": None, "cnf_with_y": None, "csv": None, "dnf_literals": 0,
                                     "cnf_literals": 0}
    counts = dontcares = None
    if usage is not None:
        counts = np.asarray(usage, dtype=np.int64).reshape(-1)
        if counts.shape != col.shape:
            raise ValueError(f"usage has {counts.size} counts, the filter has {col.size} entries")
        seen = counts >= max(1, int(min_count))
        dontcares = np.flatnonzero(~seen).tolist()
        on_seen = np.unique(col[seen]) if seen.any() else uniq[:1]       # (never looked up: any constant will do)
        if len(on_seen) == 1:
            uniq = on_seen
    if len(uniq) == 1:                                   # constant filter: the value only (:351-361)
        with open(f"{prefix}table_outputblock_{block}_filter_{filter_index}_coefdefault_{uniq[0]}.txt", "w") as f:
            f.write(str(uniq[0]))
        out["cnf_with_y"] = str(uniq[0])
        return out
    for value in uniq[1:]:
        answer = col == value
        frame = pd.concat([pattern_frame(n), pd.DataFrame(answer, columns=[f"Filter_{filter_index}_Value_{int(value)}"])], axis=1)
        if counts is not None:
            frame["count"] = counts
        csv = f"{prefix}Truth_Table_block{block}_filter_{filter_index}_coefdefault_{value}_sousblock_{sub_block}.csv"
        frame.to_csv(csv)
        out["csv"] = csv
        if n <= (max_expr_bits if minimiser == "sympy" else 16):
            if minimiser == "sympy":
                minterms = frame["index"].values[answer if counts is None else answer & seen].tolist()
                dnf, cnf = minimal_forms(minterms, n, dontcares)
            else:
                dnf, cnf = forms if forms is not None else _cover_forms(answer[None, :, None], n, None if counts is None else counts[None],
                                                                        minimiser, device, rounds, min_count)[0]
            y = cnf_with_output(dnf, cnf)
            out.update(dnf=str(dnf), cnf=str(cnf), cnf_with_y=y, dnf_literals=literal_count(str(dnf)),
                       cnf_literals=literal_count(str(cnf)))
            with open(f"{prefix}table_outputblock_{block}_filter_{filter_index}_coefdefault_{value}.txt", "w") as f:
                f.write(y)
            with open(f"{prefix}CNF_expression_block{block}_filter_{filter_index}_coefdefault_{value}_sousblock_{sub_block}.txt", "w") as f:
                f.write(str(cnf))
            with open(f"{prefix}DNF_expression_block{block}_filter_{filter_index}_coefdefault_{value}_sousblock_{sub_block}.txt", "w") as f:
                f.write(str(dnf))
    return out


def export_block(table: np.ndarray, out_dir: str, block: int, sub_block: int, filters: Optional[Iterable[int]] = None,
                 max_expr_bits: int = 9, usage: Optional[np.ndarray] = None, minimiser: str = "sympy",
                 device=None, rounds: int = 0, min_count: int = 1) -> Dict[int, Dict[str, Optional[str]]]:
    """``table``: [groups][2^n][cout_g] bits as returned by ``model.get_table(name)`` (or by the
    oracle's ``build_lut``).  Filter f = output channel f of the block = (group f // cout_g,
    output f % cout_g).  ``usage``: int64 [groups][2^n] lookup counts of the block (module docstring).
    ``minimiser`` "device" / "cpu": all filters asked for are minimised at once (``device``: a torch device, default the
    current one), with ``rounds`` reduce / expand rounds (module docstring; ignored by "sympy").  ``min_count``: the entries
    looked up fewer times than this are the don't-cares (the complement of ``minimise.care_masks(usage, min_count)``)."""
    g, size, cout_g = table.shape
    n = int(size).bit_length() - 1
    assert 2 ** n == size
    todo = range(g * cout_g) if filters is None else filters
    if usage is not None and tuple(np.shape(usage)) != (g, size):
        raise ValueError(f"usage has shape {tuple(np.shape(usage))}, the table has {g} groups of {size} entries")
    todo = list(todo)
    forms = {}
    if minimiser in ("device", "cpu") and n <= 16 and todo:
        from . import minimise
        on, dc = minimise.pack_functions(np.asarray(table) == 1, usage, min_count)
        forms = dict(zip(todo, _texts(minimise.minimal_covers(on[todo], dc[todo], n, minimiser, device, rounds), n)))
    return {f: export_filter(table[f // cout_g, :, f % cout_g], n, f, out_dir, block, sub_block, max_expr_bits,
                             None if usage is None else usage[f // cout_g], minimiser, device, forms.get(f), rounds, min_count) for f in todo}


def _texts(covers, n: int):
    from . import minimise
    return [(minimise.dnf_text(d, n), minimise.cnf_text(c, n)) for d, c in covers]


def _cover_forms(table: np.ndarray, n: int, usage, minimiser: str, device, rounds: int = 0, min_count: int = 1):
    """``(DNF text, CNF text)`` of every filter of a ``[G, 2^n, cout_g]`` 0/1 table from ``minimise`` (one call)."""
    from . import minimise
    on, dc = minimise.pack_functions(table, usage, min_count)
    return _texts(minimise.minimal_covers(on, dc, n, minimiser, device, rounds), n)


def literal_count(expr_text: Optional[str]) -> int:
    """Number of literals of an expression string (a gate-count proxy: one input per literal)."""
    return 0 if not expr_text else expr_text.count("x_")
