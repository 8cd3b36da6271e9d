"""Two-level minimisation of truth tables with don't-cares: prime, irredundant covers (not minimum ones).

The algorithm -- expand every ON minterm to a prime, order the primes by size, keep those that cover something new, drop
the redundant ones in reverse -- is stated in ``include/ttnet.h`` (``ttnet_minimise_covers``), and so are the optional
``rounds`` on top of it (``ttnet_minimise_covers_rounds``): each reduces every cube of the cover to the patterns only it
holds, expands it again in another order of the variables and runs the last two steps once more; the smallest cover
met goes out.  It exists twice and both give the same cubes in the same order for every ``rounds``:

  ``minimise_device``  the HIP kernel of ``csrc/minimise.hip``, all functions of a batch in one launch;
  ``minimise_cpu``     its twin in numpy, with no device: the comparison in tests and benchmarks, never a fallback.

A function of n inputs is two bitmaps over its 2^n patterns, uint32 ``[max(1, 2^n / 32)]``, bit ``i % 32`` of word
``i // 32`` = pattern i in the canonical order of ``model.get_table`` (variable ``x_j`` is index bit ``n-1-j``): ``on``
where it must be 1, ``dc`` where it may take either value.  A cube is the uint32 key ``mask << 16 | value``.
``check_cover`` verifies a cover exhaustively on the host; ``dnf_text`` / ``cnf_text`` print covers the way sympy prints
its forms, so ``export.cnf_with_output`` and ``export.literal_count`` take them unchanged.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np


def n_words(n: int) -> int:
    return max(1, (1 << n) // 32)


def _check_n(n: int):
    if not 1 <= n <= 16:
        raise ValueError(f"n = {n}: functions of 1 .. 16 inputs are served")


def pack_bits(flags: np.ndarray) -> np.ndarray:
    """bool ``[..., 2^n]`` -> uint32 ``[..., max(1, 2^n / 32)]`` bitmaps (unused high bits zero)."""
    flags = np.asarray(flags, dtype=bool)
    size = flags.shape[-1]
    if size < 32:
        flags = np.concatenate([flags, np.zeros(flags.shape[:-1] + (32 - size,), dtype=bool)], axis=-1)
    packed = np.packbits(flags, axis=-1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u4").astype(np.uint32, copy=False)


def unpack_bits(words: np.ndarray, n: int) -> np.ndarray:
    """uint32 ``[..., words]`` bitmaps -> bool ``[..., 2^n]``."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.uint32).astype("<u4", copy=False))
    bits = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")
    return bits[..., : 1 << n].astype(bool)


def _kept(usage: np.ndarray, min_count: int) -> np.ndarray:
    """bool, the shape of ``usage``: the entries looked up at least ``min_count`` times (the care set)."""
    if int(min_count) != min_count or min_count < 1:
        raise ValueError(f"min_count must be an integer >= 1, got {min_count!r}")
    return np.asarray(usage) >= int(min_count)


def care_masks(usage, min_count: int = 1) -> "dict":
    """The care sets of a ``table_usage()`` dict: ``{Block_TT name: uint32 [G, words]}`` bitmaps (``pack_bits``; the format
    of ``ttnet_plan_set_care``) in which an entry is kept iff its count is at least ``min_count``.  The complement is the
    ``dc`` of ``pack_functions(table, usage, min_count)`` before its repeat over ``cout_g``."""
    out = {}
    for name, u in usage.items():
        u = np.asarray(u)
        size = u.shape[-1] if u.ndim == 2 else 0
        if u.ndim != 2 or size < 2 or size & (size - 1) or size > 1 << 16:
            raise ValueError(f"usage[{name!r}] has shape {tuple(u.shape)}, expected [groups, 2^n] with 1 <= n <= 16")
        out[name] = pack_bits(_kept(u, min_count))
    return out


def pack_functions(table_bits: np.ndarray, usage: Optional[np.ndarray] = None, min_count: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """``(on, dc)`` bitmaps, uint32 ``[G * cout_g, words]``, of every filter of a ``get_table`` array ``[G, 2^n, cout_g]``
    (filter f = group ``f // cout_g``, output ``f % cout_g``, as in ``export.export_block``).  With ``usage``
    (``[G, 2^n]`` lookup counts) a pattern with count 0 is a don't-care, the rule of ``export.export_filter``; ``min_count``
    raises that to every pattern looked up fewer than ``min_count`` times (the complement of ``care_masks``)."""
    t = np.asarray(table_bits)
    g, size, cout_g = t.shape
    col = np.transpose(t != 0, (0, 2, 1)).reshape(g * cout_g, size)
    if usage is None:
        return pack_bits(col), np.zeros((g * cout_g, max(1, size // 32)), dtype=np.uint32)
    u = np.asarray(usage)
    if tuple(u.shape) != (g, size):
        raise ValueError(f"usage has shape {tuple(u.shape)}, the table has {g} groups of {size} entries")
    unseen = np.repeat(~_kept(u, min_count), cout_g, axis=0)
    return pack_bits(col & ~unseen), pack_bits(unseen)


def complement(on: np.ndarray, dc: np.ndarray, n: int) -> np.ndarray:
    """The ON set of the complement, ``~on & ~dc``: minimised with the same ``dc`` it gives the CNF (``cnf_text``)."""
    valid = np.uint32(0xFFFFFFFF if n >= 5 else (1 << (1 << n)) - 1)
    return (~(np.asarray(on, dtype=np.uint32) | np.asarray(dc, dtype=np.uint32))) & valid


# ---- the CPU twin ---------------------------------------------------------------------------------------------------------

def _implicant_flags(not_off: np.ndarray, n: int) -> np.ndarray:
    """bool ``(3,) * n``: digit j of an index is the state of x_j, 0 / 1 = literal, 2 = free; True iff that cube holds
    no OFF pattern.  One vectorised pass per variable, ``flag[.., 2, ..] = flag[.., 0, ..] & flag[.., 1, ..]``, from the
    last variable to the first so that every pass appends contiguous rows (43 M flags at n = 16)."""
    flag = np.ascontiguousarray(not_off, dtype=bool).reshape((2,) * n)
    for j in range(n - 1, -1, -1):
        head = (slice(None),) * j
        flag = np.concatenate([flag, flag[head + (slice(0, 1),)] & flag[head + (slice(1, 2),)]], axis=j)
    return flag


def _expand(keys: np.ndarray, flag: np.ndarray, n: int, order: Sequence[int]) -> np.ndarray:
    """Steps 1 and 7 for all cubes at once: every literal of x_j, j in ``order``, is dropped iff the sibling half of the
    cube as it then is holds no OFF pattern (``flag`` of ``_implicant_flags``); the grown keys."""
    flat = flag.reshape(-1)
    pow3 = 3 ** np.arange(n - 1, -1, -1, dtype=np.int64)           # weight of digit j
    shifts = np.arange(n - 1, -1, -1)[None, :]
    mask = (keys >> 16).astype(np.int64)
    value = (keys & 0xFFFF).astype(np.int64)
    digits = np.where((mask[:, None] >> shifts) & 1, (value[:, None] >> shifts) & 1, 2)
    idx = (digits * pow3[None, :]).sum(axis=1)
    for j in order:
        b = digits[:, j]
        literal = b != 2
        drop = literal & flat[np.where(literal, idx + (1 - 2 * b) * pow3[j], 0)]                   # the sibling half
        idx = np.where(drop, idx + (2 - b) * pow3[j], idx)
        bit = 1 << (n - 1 - j)
        mask = np.where(drop, mask & ~bit, mask)
        value = np.where(drop, value & ~bit, value)
    return ((mask << 16) | value).astype(np.uint32)


_POPCOUNT16 = np.unpackbits(np.arange(1 << 16, dtype="<u2").view(np.uint8).reshape(-1, 2), axis=1).sum(axis=1).astype(np.int64)


@functools.lru_cache(maxsize=1 << 14)
def _subset_sums(free_bits: int) -> np.ndarray:
    """Every subset of the set bits of ``free_bits``, as an int64 array (shared: callers do not write to it)."""
    out = np.zeros(1, dtype=np.int64)
    b = 1
    while b <= free_bits:
        if free_bits & b:
            out = np.concatenate([out, out | b])
        b <<= 1
    return out


def _cover_points(key: int, n: int, on_b: np.ndarray, on_idx: np.ndarray) -> np.ndarray:
    """The ON patterns of a cube, ascending or not: whichever of the cube and the ON set is cheaper to enumerate."""
    mask, value = key >> 16, key & 0xFFFF
    if (1 << (n - bin(mask).count("1"))) <= len(on_idx):
        pts = value | _subset_sums(~mask & ((1 << n) - 1))
        return pts[on_b[pts]]
    return on_idx[(on_idx & mask) == value]


def _cover_irredundant(ordered: List[int], n: int, on_b: np.ndarray, on_idx: np.ndarray):
    """Steps 3 and 4 on keys in step-2 order: ``(kept keys, their ON patterns, cover count of every pattern)``."""
    covered = np.zeros(1 << n, dtype=bool)
    count = np.zeros(1 << n, dtype=np.int32)
    kept: List[Tuple[int, np.ndarray]] = []
    tried = set()
    for key in ordered:                                              # step 3 (a repeated cube covers nothing new)
        if key in tried:
            continue
        tried.add(key)
        pts = _cover_points(key, n, on_b, on_idx)
        if np.count_nonzero(covered[pts]) == len(pts):
            continue
        covered[pts] = True
        count[pts] += 1
        kept.append((key, pts))
    alive = [True] * len(kept)
    for k in range(len(kept) - 1, -1, -1):                           # step 4
        pts = kept[k][1]
        if count[pts].min() >= 2:
            count[pts] -= 1
            alive[k] = False
    kept = [kp for kp, a in zip(kept, alive) if a]
    return [k for k, _ in kept], [p for _, p in kept], count


def minimise_cpu(on: np.ndarray, dc: Optional[np.ndarray], n: int, rounds: int = 0) -> np.ndarray:
    """The cover of one function (bitmaps, module docstring) as uint32 keys, by the steps of ``include/ttnet.h``: the four
    of ``ttnet_minimise_covers`` and, for ``rounds`` in 1 .. 8, the reduce / expand rounds of
    ``ttnet_minimise_covers_rounds``, of which the cover with the fewest (literals, cubes) is returned."""
    _check_n(n)
    rounds = _check_rounds(rounds)
    on_b = unpack_bits(on, n)
    dc_b = np.zeros_like(on_b) if dc is None else unpack_bits(dc, n) & ~on_b
    on_idx = np.flatnonzero(on_b)
    if len(on_idx) == 0:
        return np.zeros(0, dtype=np.uint32)
    if bool((on_b | dc_b).all()):
        return np.zeros(1, dtype=np.uint32)
    flag = _implicant_flags(on_b | dc_b, n)
    full = (1 << n) - 1
    keys = _expand((full << 16) | on_idx.astype(np.uint32), flag, n, range(n))
    free = n - _POPCOUNT16[keys >> 16]
    order = np.lexsort((on_idx, -free))                              # step 2
    cover, points, count = _cover_irredundant(keys[order].tolist(), n, on_b, on_idx)
    best = cover
    for r in range(1, int(rounds) + 1 if len(cover) > 1 else 0):
        cover = list(cover)                                          # (``best`` may be this list)
        for k in range(len(cover) - 1, -1, -1):                      # step 6 (step 5: ``count`` is what step 4 left)
            pts = points[k]
            lone = pts[count[pts] == 1]
            assert len(lone), "an irredundant cover: every cube holds an ON pattern that no other cube holds"
            agree = ~(int(np.bitwise_or.reduce(lone)) ^ int(np.bitwise_and.reduce(lone))) & full
            value = int(lone[0]) & agree
            count[pts[(pts & agree) != value]] -= 1
            cover[k] = (agree << 16) | value
        grown = _expand(np.array(cover, dtype=np.uint32), flag, n, range(n - 1, -1, -1) if r % 2 else range(n))       # step 7
        order = np.argsort(_POPCOUNT16[grown >> 16], kind="stable")                                                 # step 8
        cover, points, count = _cover_irredundant(grown[order].tolist(), n, on_b, on_idx)
        if (literal_total(cover), len(cover)) < (literal_total(best), len(best)):                  # step 9
            best = cover
    return np.array(best, dtype=np.uint32)


# ---- the device ------------------------------------------------------------------------------------------------------------

def _check_rounds(rounds: int) -> int:
    if not 0 <= int(rounds) <= 8:
        raise ValueError(f"rounds = {rounds}: 0 .. 8 rounds are served")
    return int(rounds)


def minimise_device(on, dc, n: int, device=None, cube_cap: Optional[int] = None, rounds: int = 0) -> List[np.ndarray]:
    """Covers of a batch of functions by ``ttnet_minimise_covers`` (``rounds`` = 0) or ``ttnet_minimise_covers_rounds``
    (1 .. 8): ``on`` / ``dc`` uint32 ``[F, words]`` (numpy, or torch
    tensors on the device; ``dc`` None: no don't-cares) -> F arrays of uint32 keys.  One launch for the whole batch; the
    functions whose cover has more cubes than the first cap (``cube_cap``; by default what 256 MB of keys allow the batch, at
    least 1024 and at most 2^n, which never overflows) go through one more launch with the cap they need."""
    import torch

    from . import _lib
    _check_n(n)
    rounds = _check_rounds(rounds)
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def to_dev(a):
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint32)).view(np.int32))
        a = a.to(dev).contiguous()
        if a.dim() != 2 or a.shape[1] != n_words(n) or a.element_size() != 4:
            raise ValueError(f"bitmaps must be 32-bit [functions, {n_words(n)}], got {tuple(a.shape)} of {a.dtype}")
        return a

    on_t, dc_t = to_dev(on), to_dev(dc)
    if dc_t is not None and dc_t.shape != on_t.shape:
        raise ValueError("on and dc differ in shape")
    total = on_t.shape[0]
    out: List[Optional[np.ndarray]] = [None] * total

    def run(sel: Optional[torch.Tensor], cap: int) -> Tuple[np.ndarray, np.ndarray]:
        a = on_t if sel is None else on_t[sel].contiguous()
        b = dc_t if (sel is None or dc_t is None) else dc_t[sel].contiguous()
        f = a.shape[0]
        with torch.cuda.device(dev):
            sizer = lib.ttnet_minimise_rounds_workspace if rounds else lib.ttnet_minimise_workspace
            work = torch.empty(_lib.check(sizer(n, f)), dtype=torch.uint8, device=dev)
            cubes = torch.empty((f, max(cap, 1)), dtype=torch.int32, device=dev)
            counts = torch.empty(f, dtype=torch.int32, device=dev)
            head = (C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr() if b is not None else None), n, f)
            tail = (C.c_void_p(cubes.data_ptr()), cubes.shape[1], C.c_void_p(counts.data_ptr()), C.c_void_p(work.data_ptr()),
                    work.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            _lib.check(lib.ttnet_minimise_covers_rounds(*head, rounds, *tail) if rounds else lib.ttnet_minimise_covers(*head, *tail))
            got = counts.cpu().numpy()
            width = int(min(cap, max(int(got.max()), 1)))                # only the columns some cover reaches come back
            return got, np.ascontiguousarray(cubes[:, :width].cpu().numpy()).view(np.uint32)

    budget = 1 << 26                                                 # cube slots per launch (256 MB)
    cap = min(1 << n, max(1024, budget // max(total, 1))) if cube_cap is None else int(cube_cap)
    step = max(1, budget // max(cap, 1))
    pending = [(None, cap)] if total <= step else [(torch.arange(lo, min(total, lo + step), device=dev), cap)
                                                   for lo in range(0, total, step)]
    while pending:
        sel, cap = pending.pop()
        ids = np.arange(total) if sel is None else sel.cpu().numpy()
        counts, cubes = run(sel, cap)
        over = []
        for row, f in enumerate(ids.tolist()):
            if counts[row] <= cap:
                out[f] = cubes[row, : counts[row]].copy()
            else:
                over.append((f, int(counts[row])))
        if over:
            need = max(c for _, c in over)
            step = max(1, budget // need)
            for lo in range(0, len(over), step):
                pending.append((torch.tensor([f for f, _ in over[lo:lo + step]], device=dev), need))
    return out  # type: ignore[return-value]


# ---- checking and printing ---------------------------------------------------------------------------------------------------

def cube_patterns(keys: np.ndarray, n: int) -> List[np.ndarray]:
    """The patterns of every cube, int64 arrays."""
    full = (1 << n) - 1
    return [(int(k) & 0xFFFF) | _subset_sums(~(int(k) >> 16) & full) for k in np.asarray(keys, dtype=np.uint32).tolist()]


def check_cover(on: np.ndarray, dc: Optional[np.ndarray], n: int, cubes: Sequence[int]) -> None:
    """Exhaustive check of a cover, by enumeration of every cube's patterns; raises AssertionError naming what fails:
    the cover equals the function on every care pattern; every cube is well formed, an implicant of ON u DC and prime
    (no single literal can be dropped); no cube is removable (each holds an ON pattern no other cube holds)."""
    _check_n(n)
    on_b = unpack_bits(on, n)
    dc_b = np.zeros_like(on_b) if dc is None else unpack_bits(dc, n) & ~on_b
    off_b = ~(on_b | dc_b)
    keys = np.asarray(cubes, dtype=np.uint32)
    full = (1 << n) - 1
    assert len(set(keys.tolist())) == len(keys), "a cube appears twice"
    times = np.zeros(1 << n, dtype=np.int64)
    pats = cube_patterns(keys, n)
    for key, pts in zip(keys.tolist(), pats):
        mask, value = key >> 16, key & 0xFFFF
        assert mask <= full and value & ~mask == 0, f"cube {key:#x} is malformed for n = {n}"
        assert not off_b[pts].any(), f"cube {key:#x} holds an OFF pattern"
        for b in range(n):
            if mask >> b & 1:
                assert off_b[pts ^ (1 << b)].any(), f"cube {key:#x} is not prime: the literal of x_{n - 1 - b} can be dropped"
        times[pts] += 1
    assert times[on_b].all(), f"{int((times[on_b] == 0).sum())} ON patterns are not covered"
    assert not times[off_b].any(), "an OFF pattern is covered"
    for key, pts in zip(keys.tolist(), pats):
        mine = pts[on_b[pts]]
        assert len(mine) and (times[mine] == 1).any(), f"cube {key:#x} can be removed"


def _literals(key: int, n: int, complemented: bool) -> List[str]:
    mask, value = key >> 16, key & 0xFFFF
    out = []
    for j in range(n):
        b = n - 1 - j
        if mask >> b & 1:
            positive = bool(value >> b & 1) != complemented
            out.append(f"x_{j}" if positive else f"~x_{j}")
    return out


def _text(cubes, n: int, complemented: bool) -> str:
    inner, outer = (" | ", " & ") if complemented else (" & ", " | ")
    empty, tautology = ("True", "False") if complemented else ("False", "True")
    terms = [_literals(int(k), n, complemented) for k in np.asarray(cubes, dtype=np.uint32).tolist()]
    if not terms:
        return empty
    if any(not t for t in terms):
        return tautology
    if len(terms) == 1:
        return inner.join(terms[0])
    return outer.join(t[0] if len(t) == 1 else "(" + inner.join(t) + ")" for t in terms)


def dnf_text(cubes, n: int) -> str:
    """A cover as a sum of products in sympy's print style: ``(x_0 & ~x_3) | x_5``; ``True`` / ``False`` for constants."""
    return _text(cubes, n, False)


def cnf_text(cubes, n: int) -> str:
    """The cover of the COMPLEMENT (``complement``) read by De Morgan as a product of sums: ``(~x_0 | x_3) & ~x_5``."""
    return _text(cubes, n, True)


def literal_total(cubes) -> int:
    """Literals of a cover: the set bits of its masks."""
    return int(_POPCOUNT16[np.asarray(cubes, dtype=np.uint32) >> 16].sum())


def minimal_covers(on: np.ndarray, dc: np.ndarray, n: int, minimiser: str, device=None,
                   rounds: int = 0) -> List[Tuple[np.ndarray, np.ndarray]]:
    """``(DNF cover, cover of the complement)`` of every function of ``on`` / ``dc`` ``[F, words]``; with ``"device"`` both
    covers of all functions come from one launch, with ``"cpu"`` from the twin.  ``rounds``: reduce / expand rounds, 0 .. 8."""
    on = np.asarray(on, dtype=np.uint32)
    dc = np.asarray(dc, dtype=np.uint32)
    off = complement(on, dc, n)
    if minimiser == "device":
        both = minimise_device(np.concatenate([on, off]), np.concatenate([dc, dc]), n, device, rounds=rounds)
    elif minimiser == "cpu":
        both = [minimise_cpu(a, b, n, rounds) for a, b in zip(np.concatenate([on, off]), np.concatenate([dc, dc]))]
    else:
        raise ValueError(f"minimiser {minimiser!r}: 'device' or 'cpu' (sympy is export's own path)")
    f = on.shape[0]
    return [(both[i], both[f + i]) for i in range(f)]


def gate_count_row(on: np.ndarray, dc: np.ndarray, n: int, minimiser: str = "device", device=None, rounds: int = 0) -> dict:
    """``{filters, constant, dnf_cubes, dnf_literals, cnf_cubes, cnf_literals}`` of one block's functions; a filter that is
    constant on its care patterns counts under ``constant`` and has no cubes or literals in either form.  ``rounds``: as in
    ``minimal_covers``."""
    covers = minimal_covers(on, dc, n, minimiser, device, rounds)
    row = dict(filters=len(covers), constant=0, dnf_cubes=0, dnf_literals=0, cnf_cubes=0, cnf_literals=0)
    for dnf, cnf in covers:
        if literal_total(dnf) == 0 or literal_total(cnf) == 0:       # no cube, or the cube without a literal
            row["constant"] += 1
            continue
        row["dnf_cubes"] += len(dnf)
        row["dnf_literals"] += literal_total(dnf)
        row["cnf_cubes"] += len(cnf)
        row["cnf_literals"] += literal_total(cnf)
    return row
