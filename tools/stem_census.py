#!/usr/bin/env python3
"""Static instruction census of stem_pc_kernel<false, false, 2> from the compiler's assembly listing: what one item
(one image x 8 output rows) makes a SIMD issue, set against the 7,392 cycles its 231 MFMAs hold the matrix pipe.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fno-slp-vectorize --save-temps -c \
        scale_imagenet_amd/csrc/stem.hip -o /tmp/stem.o
    python tools/stem_census.py stem-hip-amdgcn-amd-amdhsa-gfx950.s [--blocks]

A SIMD of the 12-wave workgroup holds consumer waves w and w + 4 (4 + 3 units of 33 MFMAs per item) and one producer
wave.  The listing is cut into basic blocks; a block belongs to
    unit loop      the innermost loop that holds the MFMAs (one trip per unit; the conditional store of the row-word
                   piece is its side block),
    item frame     the rest of the consumers' item loop (first fragment reads, the open transpose of the last item, barrier),
    producer pass  the blocks of the producers' item loop that hold buffer loads (16 row slots; an item that continues
                   its image runs 12 of them: slots 12-15 are separate blocks and are listed apart),
    halo copy      ds_read_b128 / ds_write_b128 pairs of the producers' item loop,
    emit rows      the loop around global_store_dwordx2 (2 trips per producer wave and item),
    producer frame whatever else the producers' item loop holds.
Vector instructions of the unit loop are split by purpose (mnemonic and operands, unambiguous in this kernel):
    sign      v_alignbit_b32 .., 31 and the v_lshrrev_b32 31 in front: sign_bits
    epilogue  DPP moves, v_permlane16_swap, register-count v_alignbit_b32, v_bitop3 / v_xor: the five epi_pieces
    address   the rest: unit_addr, the fragment bases, the producers' count
Issue cost (micro-architecture guide, cycle constants): an MFMA holds the SIMD's vector issue for 8 of its 32 cycles,
any other vector instruction for 4; LDS and memory instructions are counted, not priced.
"""
import collections
import re
import sys

SYM = "stem_pc_kernelILb0ELb0ELi2ELi2E"


def parse(path):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and SYM in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], {"label": "entry", "ins": []}
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            blocks.append(cur)
            cur = {"label": m.group(1), "ins": []}
            continue
        if not t or t.startswith(";") or t.startswith("."):
            continue
        cur["ins"].append(t.split(";")[0].strip())
    blocks.append(cur)
    return blocks


def kind(ins):
    m = ins.split()[0]
    if m.startswith("v_mfma"):
        return "mfma"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("buffer_", "global_", "scratch_", "flat_")):
        return "mem"
    if m.startswith("v_"):
        return "valu"
    return "scalar"


def purpose(ins):
    m = ins.split()[0]
    if (m == "v_alignbit_b32" and ins.rstrip().endswith(", 31")) or (m == "v_lshrrev_b32_e32" and re.search(r" 31, v\d+$", ins)):
        return "sign"
    if "dpp" in m or "row_" in ins or "quad_perm" in ins or m.startswith(("v_permlane", "v_alignbit", "v_bitop3", "v_xor")):
        return "epilogue"
    return "address"


def loops(blocks):
    """[(first, last)] block index ranges closed by a backward branch."""
    idx = {b["label"]: i for i, b in enumerate(blocks)}
    out = []
    for i, b in enumerate(blocks):
        for ins in b["ins"]:
            m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", ins)
            if m and idx.get(m.group(1), i + 1) <= i:
                out.append((idx[m.group(1)], i))
    return out


def count(blocks, sel):
    c = collections.Counter()
    for i in sel:
        for ins in blocks[i]["ins"]:
            k = kind(ins)
            c[k] += 1
            if k == "valu":
                c["valu:" + purpose(ins)] += 1
    return c


def fmt(c, split=False):
    v = c["valu"]
    by = f" (sign {c['valu:sign']}, epilogue {c['valu:epilogue']}, address {c['valu:address']})" if split else ""
    return (f"mfma {c['mfma']:4d}  valu {v:4d}{by}  lds {c['lds']:3d}  mem {c['mem']:3d}  scalar {c['scalar']:4d}  "
            f"issue {8 * c['mfma'] + 4 * v:5d} cycles")


def main():
    blocks = parse(sys.argv[1])
    has = lambda i, pat: any(re.match(pat, x) for x in blocks[i]["ins"])
    lp = loops(blocks)
    unit = min((l for l in lp if any(has(i, "v_mfma") for i in range(l[0], l[1] + 1))), key=lambda l: l[1] - l[0])
    cons = min((l for l in lp if l[0] <= unit[0] and unit[1] <= l[1] and l != unit), key=lambda l: l[1] - l[0])
    both = lambda l, *pats: all(any(has(i, p) for i in range(l[0], l[1] + 1)) for p in pats)
    prod = max((l for l in lp if both(l, "s_barrier", "buffer_load") and not both(l, "v_mfma")), key=lambda l: l[1] - l[0])
    sets = collections.OrderedDict()
    sets["unit loop (per unit)"] = list(range(unit[0], unit[1] + 1))
    sets["item frame (per consumer wave and item)"] = [i for i in range(cons[0], cons[1] + 1) if not unit[0] <= i <= unit[1]]
    pr = list(range(prod[0], prod[1] + 1))
    inner = [l for l in lp if prod[0] <= l[0] and l[1] <= prod[1] and l != prod]
    emit = sorted({i for l in inner for i in range(l[0], l[1] + 1) if any(has(k, "global_store") for k in range(l[0], l[1] + 1))})
    # blocks the compiler laid out behind the loop: the slots a continuing item skips (12-15) and three of the four halo pieces
    late = [i for i in range(prod[1] + 1, len(blocks)) if has(i, "buffer_load")]
    sets["producer pass, slots 0-11 (per producer wave and item)"] = [i for i in pr if has(i, "buffer_load") and i not in emit]
    sets["producer pass, slots 12-15 (whole tiles only)"] = late
    sets["halo copy"] = [i for i in range(prod[0], len(blocks)) if has(i, "ds_read_b128") and not has(i, "buffer_load")]
    sets["emit rows (per trip; 2 trips per wave and item)"] = emit
    used = set(sum(sets.values(), []))
    sets["producer frame"] = [i for i in pr if i not in used]
    res = {}
    for name, sel in sets.items():
        res[name] = count(blocks, sel)
        print(f"{name:58s} {fmt(res[name], name.startswith(('unit', 'item')))}")
        if "--blocks" in sys.argv:
            for i in sel:
                print(f"    {blocks[i]['label']:12s} {len(blocks[i]['ins'])} instructions")
    u, f = res["unit loop (per unit)"], res["item frame (per consumer wave and item)"]
    p = sum((res[k] for k in sets if k.startswith(("producer pass, slots 0", "halo", "producer frame"))), collections.Counter())
    e = res["emit rows (per trip; 2 trips per wave and item)"]
    simd = collections.Counter()
    for k in set(u) | set(f) | set(p) | set(e):
        simd[k] = 7 * u[k] + 2 * f[k] + p[k] + 2 * e[k]
    print(f"{'one SIMD, one continuing item: 7 units + 2 frames + 1 producer':58s} {fmt(simd)}")
    print(f"matrix pipe: {simd['mfma']} MFMAs x 32 = {32 * simd['mfma']} cycles; vector issue {8 * simd['mfma'] + 4 * simd['valu']} cycles "
          f"({8 * simd['mfma']} the MFMAs' own), {100 * (8 * simd['mfma'] + 4 * simd['valu']) / (32 * simd['mfma']):.0f} % of the pipe time")


if __name__ == "__main__":
    main()
