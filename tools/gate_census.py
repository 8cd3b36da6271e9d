#!/usr/bin/env python3
"""Static instruction census of gate_block_kernel from the compiler's assembly listing.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off --save-temps -c \
        scale_imagenet_amd/csrc/gate_fused.hip -o /tmp/gate_fused.o
    python tools/gate_census.py gate_fused-hip-amdgcn-amd-amdhsa-gfx950.s 56 29 0 [--blocks]

The round loop of the kernel is cut at its workgroup barriers: the stretch after the k-th barrier of the
loop is phase A, B1, B2 (+ the store of bytes 0, 1), C1, C2.  Inside a stretch every basic block is listed
with the mnemonics of its vector instructions; a block that branches back to itself or to an earlier block
of the same stretch is an inner loop (phase A's border loop, phase C's wave-task loop, the parity tap) and
its trip count has to be multiplied in by hand (DESIGN.md 4 has the counts per geometry).

Purpose classes (by mnemonic, which in this kernel is unambiguous enough to be useful):
    exchange   v_mov_b32_dpp, ds_swizzle / ds_bpermute            lane exchanges of the transposes and majorities
    rotate     v_alignbit_b32                                     butterfly rotates, row shifts, table-bit rotates
    select     v_bitop3_b32, v_bfi_b32                            butterfly merges, nibble merges of index forming
    perm       v_perm_b32                                         byte permutes (indices, raw bytes, stores)
    extract    v_bfe_u32, v_lshl_or_b32, v_and_or_b32, v_or3      bit extraction and accumulation, table addresses
    logic      v_and / v_or / v_xor / v_lshl / v_lshr / v_not     masks, shifts, majorities
    predicate  v_cmp*, v_cndmask*                                 border and tail tests
    arith      v_add*, v_sub*, v_mul*, v_mad*, v_lshl_add*        address arithmetic, task decomposition
    move       v_mov_b32, v_readfirstlane, v_accvgpr*             copies
"""
import collections
import re
import sys

CLASSES = [
    ("exchange", r"v_mov_b32_dpp|v_\w+_dpp|ds_swizzle|ds_bpermute|v_permlane"),
    ("rotate", r"v_alignbit"),
    ("select", r"v_bitop3|v_bfi"),
    ("perm", r"v_perm_b32"),
    ("extract", r"v_bfe_u32|v_lshl_or|v_and_or|v_or3"),
    ("predicate", r"v_cmp|v_cndmask"),
    ("arith", r"v_add|v_sub|v_mul|v_mad|v_lshl_add|v_pk_"),
    ("move", r"v_mov_b32|v_readfirstlane|v_readlane|v_writelane|v_accvgpr"),
    ("logic", r"v_"),
]


def classify(m):
    for name, pat in CLASSES:
        if re.match(pat, m):
            return name
    return None


def main():
    path, H, HO, last = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    show_blocks = "--blocks" in sys.argv
    sym = f"gate_block_kernelILi{H}ELi{HO}ELb{last}EEE"
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if sym in l and l.split(";")[0].rstrip().endswith(":") and not l.startswith("\t"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], {"label": "entry", "ins": []}
    for l in lines[start + 1:end]:
        t = l.strip()
        if not t or t.startswith(";") or t.startswith("."):
            m = re.match(r"^(\.LBB\w+):", t)
            if m:
                blocks.append(cur)
                cur = {"label": m.group(1), "ins": []}
            continue
        cur["ins"].append(t.split(";")[0].strip())
    blocks.append(cur)
    order = {b["label"]: i for i, b in enumerate(blocks)}

    # the round loop: from the target of the last backward branch that spans a barrier to that branch
    best = None
    for i, b in enumerate(blocks):
        for ins in b["ins"]:
            m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", ins)
            if m and order.get(m.group(1), 1 << 30) <= i:
                j = order[m.group(1)]
                nb = sum(ins2.startswith("s_barrier") for bb in blocks[j:i + 1] for ins2 in bb["ins"])
                if best is None or nb > best[2]:
                    best = (j, i, nb)
    j0, j1, nb = best
    print(f"{sym}: round loop = blocks {blocks[j0]['label']} .. {blocks[j1]['label']}, {nb} barriers")
    names = ["(loop head)", "A", "B1", "B2+store", "C1", "C2"] if not last else ["(loop head)", "A", "B1", "B2+store", "out"]
    seg = 0
    table = collections.OrderedDict()
    for i in range(j0, j1 + 1):
        b = blocks[i]
        hist = collections.Counter()
        back = False
        for ins in b["ins"]:
            mn = ins.split()[0]
            if mn.startswith("s_barrier"):
                if show_blocks and hist:
                    print(f"  [{names[min(seg, len(names) - 1)]}] {b['label']} (to barrier): {dict(hist)}")
                seg += 1
                hist = collections.Counter()
                continue
            m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", ins)
            if m and j0 < order.get(m.group(1), 1 << 30) <= i:
                back = True
            c = classify(mn)
            key = names[min(seg, len(names) - 1)]
            t = table.setdefault(key, collections.Counter())
            if c:
                t[c] += 1
                t["VALU"] += 1
                hist[mn] += 1
            elif mn.startswith("ds_"):
                t["lds"] += 1
            elif mn.startswith("s_") and not mn.startswith(("s_waitcnt", "s_nop", "s_barrier")):
                t["salu"] += 1
        if show_blocks and hist:
            print(f"  [{names[min(seg, len(names) - 1)]}] {b['label']}{' (inner loop)' if back else ''}: {dict(hist)}")
    cols = ["VALU", "exchange", "rotate", "select", "perm", "extract", "logic", "predicate", "arith", "move", "lds", "salu"]
    print("phase        " + " ".join(f"{c:>9}" for c in cols))
    tot = collections.Counter()
    for k, t in table.items():
        print(f"{k:<12} " + " ".join(f"{t[c]:>9}" for c in cols))
        tot.update(t)
    print(f"{'static sum':<12} " + " ".join(f"{tot[c]:>9}" for c in cols))


if __name__ == "__main__":
    main()
