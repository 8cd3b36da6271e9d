"""The reduce / expand rounds of the minimiser on the CPU twin (scale_imagenet_amd.minimise.minimise_cpu(..., rounds)).

The rounds never cost a literal, keep the cover prime and irredundant (``check_cover``), and on the four seeded sets below two
rounds must strictly lower the literal total.  The pinned totals are those of the rules stated in ``include/ttnet.h``."""
import numpy as np
import pytest

from _minimise_util import DENSITIES, SETS, literal_set, random_functions, size
from _util import spec_and_state
from scale_imagenet_amd import minimise as M

# total DNF literals of the 30 functions of each set at rounds 0, 1, 2, 4
PINS = {(6, 0.0, 60): (1884, 1811, 1810, 1799), (6, 0.4, 64): (1014, 933, 932, 925),
        (8, 0.0, 80): (9560, 8937, 8849, 8801), (8, 0.4, 84): (5320, 4657, 4599, 4548)}


@pytest.mark.parametrize("n", [1, 2, 4, 5, 6, 9])
def test_no_rounds_is_the_plain_cover(n):
    on, dc = random_functions(2000 + n, n, 10, DENSITIES)
    for f in range(10):
        assert M.minimise_cpu(on[f], dc[f], n, rounds=0).tolist() == M.minimise_cpu(on[f], dc[f], n).tolist(), (n, f)
        assert M.minimise_cpu(on[f], None, n, 0).tolist() == M.minimise_cpu(on[f], None, n).tolist(), (n, f)


@pytest.mark.parametrize("case", SETS, ids=lambda c: f"n{c[0]}-dc{int(100 * c[1])}")
def test_rounds_shrink_the_four_sets(case):
    n, dcf, seed = case
    on, dc = literal_set(n, dcf, seed)
    total = {r: 0 for r in (0, 1, 2, 4)}
    for f in range(len(on)):
        last = None
        for r in (0, 1, 2, 4):
            cubes = M.minimise_cpu(on[f], dc[f], n, r)
            M.check_cover(on[f], dc[f], n, cubes)
            if last is not None:
                assert size(cubes) <= last, (f, r)                 # (literals, cubes) never grows with the rounds ..
                assert size(cubes)[0] <= first, (f, r)             # .. so never more literals than without them
            else:
                first = size(cubes)[0]
            last = size(cubes)
            total[r] += last[0]
    print(f"n = {n}, don't-cares {dcf:.0%}, seed {seed}: literals at rounds 0 / 1 / 2 / 4 = {[total[r] for r in (0, 1, 2, 4)]}")
    assert total[2] < total[0]
    assert tuple(total[r] for r in (0, 1, 2, 4)) == PINS[case]


@pytest.mark.parametrize("rounds", [1, 2, 4, 8])
def test_edge_cases_return_their_plain_cover(rounds):
    for n in (1, 3, 5, 8):
        none, every = np.zeros(1 << n, dtype=bool), np.ones(1 << n, dtype=bool)
        one = none.copy()
        one[(1 << n) - 2] = True
        half = (np.arange(1 << n) & 1) == 1                                 # the one cube x_{n-1}
        for on_b, dc_b in ((every, none), (none, none), (none, every), (one, ~one), (half, none), (one, none), (half, ~half & ~one)):
            on, dc = M.pack_bits(on_b), M.pack_bits(dc_b)
            assert M.minimise_cpu(on, dc, n, rounds).tolist() == M.minimise_cpu(on, dc, n).tolist(), (n, rounds)
    for on_bits in range(4):                                                # every function of one input
        on = np.array([on_bits], dtype=np.uint32)
        assert M.minimise_cpu(on, None, 1, rounds).tolist() == M.minimise_cpu(on, None, 1).tolist()


def test_rounds_out_of_range():
    on, dc = random_functions(3, 4, 1)
    for rounds in (9, -1):
        with pytest.raises(ValueError):
            M.minimise_cpu(on[0], dc[0], 4, rounds)
        with pytest.raises(ValueError):
            M.minimal_covers(on, dc, 4, "cpu", rounds=rounds)


def synthetic_table(n, groups, cout, seed):
    """A ``get_table``-shaped 0/1 array ``[groups, 2^n, cout]``: signs of seeded quadratic forms of the +-1 inputs."""
    rng = np.random.default_rng(seed)
    x = 2.0 * ((np.arange(1 << n)[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1) - 1.0
    w1 = rng.standard_normal((groups, cout, n))
    w2 = rng.standard_normal((groups, cout, n, n)) * 0.5
    pre = np.einsum("pi,gci->gpc", x, w1) + np.einsum("pi,gcij,pj->gpc", x, w2, x)
    return (pre > 0).astype(np.uint8)


def test_gate_count_row_passes_the_rounds_on():
    from oracle import ttnet_bits as OB
    spec, st = spec_and_state("xsmall")
    small, _ = OB.build_lut(st, spec.blocks[0].conv1)
    rng = np.random.default_rng(8)
    for table, usage, n in ((small, None, 4), (synthetic_table(8, 2, 4, 88), (rng.random((2, 256)) < 0.6).astype(np.int64), 8)):
        on, dc = M.pack_functions(table, usage)
        plain, two = M.gate_count_row(on, dc, n, "cpu"), M.gate_count_row(on, dc, n, "cpu", rounds=2)
        assert plain == M.gate_count_row(on, dc, n, "cpu", rounds=0)
        assert two["filters"] == plain["filters"] and two["constant"] == plain["constant"]
        assert two["dnf_literals"] <= plain["dnf_literals"] and two["cnf_literals"] <= plain["cnf_literals"]
        covers = M.minimal_covers(on, dc, n, "cpu", rounds=2)
        assert two["dnf_literals"] == sum(M.literal_total(d) for d, c in covers if M.literal_total(d) and M.literal_total(c))
    assert two["dnf_literals"] + two["cnf_literals"] < plain["dnf_literals"] + plain["cnf_literals"]     # the 8-input table


def test_command_line_checks_the_rounds_before_anything_runs():
    from scale_imagenet_amd import main as cli
    parser = cli.build_parser()
    flag = [a for a in parser._actions if "--table_gates_rounds" in a.option_strings][0]
    assert flag.default == 0 and list(flag.choices) == list(range(9))
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            parser.parse_args(["--table_gates", "g.csv", "--table_gates_rounds", bad])
    assert parser.parse_args(["--table_gates", "g.csv", "--table_gates_rounds", "2"]).table_gates_rounds == 2
    with pytest.raises(SystemExit, match="needs --table_gates"):
        cli.main(["--table_gates_rounds", "2"])
