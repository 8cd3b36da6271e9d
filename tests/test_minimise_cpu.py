"""The CPU twin of the truth-table minimiser (scale_imagenet_amd.minimise.minimise_cpu), its checker and its text forms.

No GPU.  ``check_cover`` enumerates every cube: the cover equals the function on every care pattern, every cube is a
prime implicant of ON u DC, and no cube can be removed.  Literal counts against sympy's minimal forms are printed, not
asserted: the covers are prime and irredundant, not minimum.

Recorded (this file's random functions, printed by ``test_text_is_equivalent_to_sympy..``): DNF + CNF literals, ours /
sympy's, summed per n: 6/6 at n = 2, 23/23 at n = 3, 82/79 = 1.038 at n = 4, 167/160 = 1.044 at n = 5, 394/362 = 1.088 at
n = 6; profiles/minimise_bench.txt has the wider measurement."""
import os

import numpy as np
import pytest

from _util import spec_and_state
from scale_imagenet_amd import export as E
from scale_imagenet_amd import minimise as M

DENSITIES = [(0.5, 0.0), (0.3, 0.4), (0.05, 0.9), (0.9, 0.05), (0.1, 0.0)]


def random_function(rng, n, p_on, p_dc):
    r = rng.random(1 << n)
    return M.pack_bits(r < p_on), M.pack_bits((r >= p_on) & (r < p_on + p_dc))


def cover_ok(on, dc, n):
    cubes = M.minimise_cpu(on, dc, n)
    M.check_cover(on, dc, n, cubes)
    return cubes


@pytest.mark.parametrize("n", range(1, 9))
def test_random_functions(n):
    rng = np.random.default_rng(100 + n)
    for p_on, p_dc in DENSITIES:
        for _ in range(6):
            cover_ok(*random_function(rng, n, p_on, p_dc), n)


def test_parity_keeps_every_minterm():
    n = 6
    idx = np.arange(1 << n)
    on = M.pack_bits(np.array([bin(i).count("1") & 1 for i in idx], dtype=bool))
    cubes = cover_ok(on, None, n)
    assert len(cubes) == 32 and all(int(k) >> 16 == 63 for k in cubes)
    assert [int(k) & 0xFFFF for k in cubes] == [i for i in idx if bin(i).count("1") & 1]     # step-2 order: minterm ascending


def test_single_cube():
    n = 7
    idx = np.arange(1 << n)
    mask, value = 0b1010010, 0b1000010
    on = M.pack_bits((idx & mask) == value)
    assert cover_ok(on, None, n).tolist() == [mask << 16 | value]
    assert M.dnf_text([mask << 16 | value], n) == "x_0 & ~x_2 & x_5"


def test_constants():
    for n in (1, 3, 5, 8):
        zero, ones = M.pack_bits(np.zeros(1 << n, dtype=bool)), M.pack_bits(np.ones(1 << n, dtype=bool))
        assert cover_ok(zero, None, n).tolist() == []                    # ON empty
        assert cover_ok(zero, ones, n).tolist() == []                    # ON empty, everything else free
        assert cover_ok(ones, None, n).tolist() == [0]                   # OFF empty
        one = np.zeros(1 << n, dtype=bool)
        one[(1 << n) - 2] = True
        assert cover_ok(M.pack_bits(one), M.pack_bits(~one), n).tolist() == [0]      # one ON pattern, the rest don't-care
    assert M.dnf_text([], 4) == "False" and M.dnf_text([0], 4) == "True"
    assert M.cnf_text([], 4) == "True" and M.cnf_text([0], 4) == "False"


def test_sixteen_inputs_with_dontcares():
    n = 16
    on, dc = random_function(np.random.default_rng(16), n, 0.005, 0.99)
    cubes = cover_ok(on, dc, n)
    assert 0 < len(cubes) <= int(M.unpack_bits(on, n).sum())


def test_on_wins_over_dc_and_unused_bits_are_ignored():
    n = 3
    on, dc = np.array([0b00010110], dtype=np.uint32), np.array([0b01000110], dtype=np.uint32)
    assert M.minimise_cpu(on, dc, n).tolist() == M.minimise_cpu(on, dc & ~on, n).tolist()
    M.check_cover(on, dc, n, M.minimise_cpu(on, dc, n))


def test_pack_functions_follows_export_rule():
    rng = np.random.default_rng(3)
    table = rng.integers(0, 2, size=(3, 16, 2)).astype(np.uint8)
    usage = rng.integers(0, 3, size=(3, 16))
    on, dc = M.pack_functions(table, usage)
    assert on.shape == (6, 1) and on.dtype == np.uint32
    for f in range(6):
        g, o = divmod(f, 2)
        assert M.unpack_bits(on[f], 4).tolist() == ((table[g, :, o] == 1) & (usage[g] > 0)).tolist()
        assert M.unpack_bits(dc[f], 4).tolist() == (usage[g] == 0).tolist()
    on0, dc0 = M.pack_functions(table)
    assert not dc0.any() and M.unpack_bits(on0[3], 4).tolist() == (table[1, :, 1] == 1).tolist()
    with pytest.raises(ValueError):
        M.pack_functions(table, usage[:2])


def _sympy_forms(on_b, dc_b, n):
    minterms = np.flatnonzero(on_b).tolist()
    return E.minimal_forms(minterms, n, np.flatnonzero(dc_b).tolist())


def test_text_is_equivalent_to_sympy_and_feeds_cnf_with_output(capsys):
    from sympy import lambdify, symbols, sympify
    rng = np.random.default_rng(7)
    ratio = {}
    for n in (2, 3, 4, 5, 6):
        names = {f"x_{i}": symbols(f"x_{i}") for i in range(n)}
        idx = np.arange(1 << n)
        columns = [((idx >> (n - 1 - j)) & 1).astype(bool) for j in range(n)]

        def values(expr):
            return np.broadcast_to(np.asarray(lambdify(list(names.values()), expr, "numpy")(*columns), dtype=bool), idx.shape)

        ours = theirs = 0
        for p_on, p_dc in [(0.5, 0.0), (0.3, 0.4), (0.2, 0.0), (0.6, 0.2)]:
            on, dc = random_function(rng, n, p_on, p_dc)
            on_b, dc_b = M.unpack_bits(on, n), M.unpack_bits(dc, n)
            if not on_b.any() or (on_b | dc_b).all():
                continue
            dnf = M.dnf_text(M.minimise_cpu(on, dc, n), n)
            cnf = M.cnf_text(M.minimise_cpu(M.complement(on, dc, n), dc, n), n)
            s_dnf, s_cnf = _sympy_forms(on_b, dc_b, n)
            for text, ref in ((dnf, s_dnf), (cnf, s_cnf)):
                expr = sympify(text, locals=names)                    # parsed back by sympy
                assert np.array_equal(values(expr)[~dc_b], values(ref)[~dc_b]), (n, text, str(ref))
                assert np.array_equal(values(expr)[~dc_b], on_b[~dc_b])
            y = E.cnf_with_output(dnf, cnf)
            assert y.count("~y") == cnf.count("&") + 1 and y.count("(y |") == len(M.minimise_cpu(on, dc, n))
            ours += E.literal_count(dnf) + E.literal_count(cnf)
            theirs += E.literal_count(str(s_dnf)) + E.literal_count(str(s_cnf))
        ratio[n] = (ours, theirs)
    with capsys.disabled():
        print("\nDNF + CNF literals, ours / sympy:", {n: f"{a}/{b} = {a / max(b, 1):.3f}" for n, (a, b) in ratio.items()})


def test_export_block_with_the_cpu_minimiser(tmp_path):
    from oracle import ttnet_bits as OB
    spec, st = spec_and_state("xsmall")
    table, _ = OB.build_lut(st, spec.blocks[0].conv1)
    n = 4
    filters = [f for f in range(table.shape[0] * table.shape[2]) if len(np.unique(table[f // table.shape[2], :, f % table.shape[2]])) == 2][:6]
    assert len(filters) >= 3
    base = E.export_block(table, str(tmp_path / "a"), 0, 0, filters=filters)
    again = E.export_block(table, str(tmp_path / "b"), 0, 0, filters=filters, minimiser="sympy")
    assert base == {f: {k: (v.replace("/b/", "/a/") if k == "csv" else v) for k, v in r.items()} for f, r in again.items()}
    for name in sorted(os.listdir(tmp_path / "a")):
        assert open(tmp_path / "a" / name).read() == open(tmp_path / "b" / name).read(), name
    got = E.export_block(table, str(tmp_path / "c"), 0, 0, filters=filters, minimiser="cpu")
    assert sorted(os.listdir(tmp_path / "c")) == sorted(os.listdir(tmp_path / "a"))          # the same four files per filter
    assert len(os.listdir(tmp_path / "c")) == 4 * len(filters)
    for f in filters:
        col = table[f // table.shape[2], :, f % table.shape[2]] == 1
        on = M.pack_bits(col)
        assert got[f]["dnf"] == M.dnf_text(M.minimise_cpu(on, None, n), n)
        assert got[f]["cnf"] == M.cnf_text(M.minimise_cpu(M.complement(on, 0 * on, n), None, n), n)
        assert got[f]["dnf_literals"] == E.literal_count(got[f]["dnf"]) > 0 and got[f]["cnf_literals"] > 0
        assert got[f]["cnf_with_y"] == E.cnf_with_output(got[f]["dnf"], got[f]["cnf"])
        assert open(got[f]["csv"]).read() == open(base[f]["csv"]).read()
    with pytest.raises(ValueError):
        E.export_block(table, str(tmp_path / "d"), 0, 0, filters=filters[:1], minimiser="espresso")


def test_export_sixteen_inputs_with_usage(tmp_path):
    """n = 16 through export_filter's own path, almost everything don't-care: the expressions exist and match the table on
    every pattern seen."""
    rng = np.random.default_rng(5)
    table = rng.integers(0, 2, size=(1, 65536, 1)).astype(np.uint8)
    usage = (rng.random((1, 65536)) < 0.004).astype(np.int64)
    out = E.export_block(table, str(tmp_path), 4, 0, usage=usage, minimiser="cpu")[0]
    assert out["dnf"] and out["cnf"] and out["dnf_literals"] > 0
    seen = usage[0] > 0
    for text in (out["dnf"], out["cnf"]):
        assert np.array_equal(evaluate_text(text, 16)[seen], table[0, seen, 0] == 1)


def evaluate_text(text: str, n: int) -> np.ndarray:
    """An expression in the printed style on all 2^n patterns (x_j = index bit n-1-j)."""
    idx = np.arange(1 << n)
    env = {f"x_{j}": ((idx >> (n - 1 - j)) & 1).astype(bool) for j in range(n)}
    return np.broadcast_to(eval(text, {"__builtins__": {}}, {**env, "True": True, "False": False}), idx.shape)   # &, |, ~ on bool arrays


def test_gate_count_row_counts_constants_apart():
    n = 4
    idx = np.arange(16)
    on = np.stack([M.pack_bits(idx >= 8), M.pack_bits(np.zeros(16, dtype=bool)), M.pack_bits((idx & 3) == 3)])
    row = M.gate_count_row(on, np.zeros_like(on), n, minimiser="cpu")
    assert row == dict(filters=3, constant=1, dnf_cubes=2, dnf_literals=3, cnf_cubes=3, cnf_literals=3)
