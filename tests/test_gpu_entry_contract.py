"""GPU: what the extension entries of the C ABI answer to bad calls, which fault wins when two meet, and which launches a
good call makes -- compared exactly with ``tests/golden/entry_contract.json``.

The golden file is a recording of ``record()`` below on the library as it stood before the plan's host code was split
into plan.hip / plan_tables.hip / plan_certify.hip.  Nothing in it is computed by the code under test: a status, a
``ttnet_last_error`` text, the order of two checks or the sequence of timing names that differs from the recording is a
change a caller can observe.

Plans: TT-small p = 64 --layers 1 and vAlexnet, both max_batch 4 with two lanes, a never-finalized plan of each, and a
never-finalized plan of the full variant (the variant that tables, usage counts and care sets refuse).  Inputs: three
synthetic images."""
import ctypes as C
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from _util import GOLD, args_for, spec_and_state
from scale_imagenet_amd import _lib, minimise, synth, ttnet
from scale_imagenet_amd.spec import make_spec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(GOLD, "entry_contract.json")
N = 3                      # images per call: a batch, a second lane, a non-first image
MAX_BATCH = 4
NAN, INF = float("nan"), float("inf")
STEM_ROWS, FEAT_ROWS = 64 * 10, 256 * 11


class Entry:
    """A C entry with a good call's arguments by name; ``entry(name=value, ..)`` replaces some of them."""

    def __init__(self, lib, fn, **good):
        self.lib, self.fn, self.good = lib, getattr(lib, fn), good

    def __call__(self, **kw):
        unknown = set(kw) - set(self.good)
        assert not unknown, unknown
        st = int(self.fn(*{**self.good, **kw}.values()))
        return [st, self.lib.ttnet_last_error().decode() if st < 0 else ""]


def make_plan(variant, dev, finalize=True):
    spec = make_spec("full", 6, 10, 1) if variant == "full" else spec_and_state(variant)[0]
    plan = ttnet._Plan(spec, args_for(variant), dev.index, MAX_BATCH)
    if finalize:
        st = spec_and_state(variant)[1]
        plan.load(OrderedDict((k, torch.from_numpy(v.copy())) for k, v in st.items()), torch.cuda.current_stream(dev).cuda_stream)
        plan.set_lanes(2)
    return plan


def timing_names(plan):
    cap = 128
    names, ms = (C.c_char_p * cap)(), (C.c_float * cap)()
    k = _lib.check(plan.lib.ttnet_plan_last_timings(plan.handle, names, ms, cap))
    assert k < cap
    return [names[i].decode() for i in range(k)]


def profiled(plan, call):
    """The timing names of one good call (profiling on for that call alone)."""
    _lib.check(plan.lib.ttnet_plan_set_profiling(plan.handle, 1))
    ans = call()
    assert ans == [0, ""], ans
    names = timing_names(plan)
    _lib.check(plan.lib.ttnet_plan_set_profiling(plan.handle, 0))
    return names


def record_small(dev, out):
    lib = _lib.load()
    single, both, timings, memory = out["single"], out["precedence"], out["timings"], out["memory"]
    spec = spec_and_state("small")[0]
    S, raw, full, V = make_plan("small", dev), make_plan("small", dev, False), make_plan("full", dev, False), make_plan("valexnet", dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    x = torch.from_numpy(synth.synth_images(MAX_BATCH)).to(dev)
    logits = torch.zeros((MAX_BATCH, 1000), dtype=torch.float32, device=dev)
    blocks = spec.block_tts()
    rows = torch.zeros((MAX_BATCH, len(blocks)), dtype=torch.int32, device=dev)
    b0 = blocks[0]
    name = b0.name.encode()
    counts = np.zeros((b0.groups, 1 << b0.fan_in_bits), dtype=np.int64)
    bits = np.zeros((b0.groups, minimise.n_words(b0.fan_in_bits)), dtype=np.uint32)
    table = np.zeros((b0.groups, 1 << b0.fan_in_bits, b0.cout_g), dtype=np.uint8)
    stage = np.zeros((N, spec.p, 56), dtype=np.uint64)
    host = lambda a: a.ctypes.data                                              # noqa: E731
    q = C.c_int64()

    usage_add = Entry(lib, "ttnet_table_usage_add", pl=S.handle, lane=0, stream=s)
    usage_get = Entry(lib, "ttnet_plan_get_table_usage", pl=S.handle, name=name, dst=host(counts), bytes=counts.nbytes)
    usage_reset = Entry(lib, "ttnet_plan_table_usage_reset", pl=S.handle, stream=s)
    set_care = Entry(lib, "ttnet_plan_set_care", pl=S.handle, name=name, bits=host(bits), bytes=bits.nbytes)
    misses = Entry(lib, "ttnet_care_misses", pl=S.handle, lane=0, rows=rows.data_ptr(), stream=s)
    read_stage = Entry(lib, "ttnet_read_stage", pl=S.handle, stage=b"features.3", n=N, dst=host(stage), bytes=stage.nbytes, on_device=0, stream=s)
    get_table = Entry(lib, "ttnet_plan_get_table", pl=S.handle, name=name, dst=host(table), bytes=table.nbytes)
    set_table = Entry(lib, "ttnet_plan_set_table", pl=S.handle, name=name, src=host(table), bytes=table.nbytes)
    forward = Entry(lib, "ttnet_forward_lane", pl=S.handle, lane=0, x=x.data_ptr(), n=N, out=logits.data_ptr(), stream=s)
    query = Entry(lib, "ttnet_plan_query", pl=S.handle, what=b"last_n:0", out=C.byref(q))

    def mem(tag):
        for k in ("usage_bytes", "care_bytes", "table_bytes", "workspace_bytes"):
            memory[f"small:{tag}:{k}"] = S.query(k)

    def group(dst, entry, prefix, cases):
        for tag, kw in cases.items():
            assert f"{prefix}:{tag}" not in dst
            dst[f"{prefix}:{tag}"] = entry(**kw)

    mem("created")
    # -- nothing enabled, no forward yet
    group(single, usage_add, "usage_add", {"null plan": dict(pl=None), "before enable": {}})
    group(both, usage_add, "usage_add", {"before enable + lane 2": dict(lane=2)})
    group(single, usage_reset, "usage_reset", {"null plan": dict(pl=None), "before enable": {}})
    group(single, usage_get, "usage_get", {"null plan": dict(pl=None), "null name": dict(name=None), "null dst": dict(dst=None), "before enable": {}})
    group(both, usage_get, "usage_get", {"before enable + unknown name": dict(name=b"features.9.Block_conv1")})
    group(single, misses, "care_misses", {"null plan": dict(pl=None), "before set_care": {}})
    group(both, misses, "care_misses", {"before set_care + null rows": dict(rows=None)})
    group(single, read_stage, "read_stage", {"null plan": dict(pl=None), "null stage": dict(stage=None), "null dst": dict(dst=None),
                                             "no forward has run": {}})
    group(single, forward, "forward_lane", {
        "null plan": dict(pl=None), "null x": dict(x=None), "null out": dict(out=None), "unfinalized": dict(pl=raw.handle), "n 0": dict(n=0),
        "n 5": dict(n=5), "x misaligned": dict(x=x.data_ptr() + 4), "out misaligned": dict(out=logits.data_ptr() + 2), "lane -1": dict(lane=-1),
        "lane 2": dict(lane=2)})
    group(both, forward, "forward_lane", {
        "null x + unfinalized": dict(x=None, pl=raw.handle), "unfinalized + n 0": dict(pl=raw.handle, n=0),
        "n 5 + x misaligned": dict(n=5, x=x.data_ptr() + 4), "x misaligned + out misaligned": dict(x=x.data_ptr() + 4, out=logits.data_ptr() + 2),
        "out misaligned + lane 2": dict(out=logits.data_ptr() + 2, lane=2)})
    group(single, query, "query", {"null plan": dict(pl=None), "null what": dict(what=None), "null out": dict(out=None),
                                   "last_n:-1": dict(what=b"last_n:-1"), "last_n:2": dict(what=b"last_n:2"), "last_n:0 before": {}})
    memory["small:last_n:0 before"] = q.value
    # -- counters on, still no forward
    _lib.check(lib.ttnet_plan_table_usage_enable(S.handle, 1))
    mem("usage on")
    group(single, usage_add, "usage_add", {"lane -1": dict(lane=-1), "lane 2": dict(lane=2), "no forward has run": {},
                                           "no forward has run on lane 1": dict(lane=1)})
    group(single, usage_get, "usage_get", {"unknown name": dict(name=b"features.9.Block_conv1"), "wrong bytes": dict(bytes=counts.nbytes - 8)})
    group(both, usage_get, "usage_get", {"unknown name + wrong bytes": dict(name=b"features.9.Block_conv1", bytes=8)})
    single["usage_reset:good"] = usage_reset()
    # -- care sets
    group(single, set_care, "set_care", {
        "null plan": dict(pl=None), "null name": dict(name=None), "unknown name": dict(name=b"features.9.Block_conv1"),
        "wrong bytes": dict(bytes=bits.nbytes - 4), "full variant": dict(pl=full.handle), "vAlexnet": dict(pl=V.handle),
        "null bits (no care set there)": dict(bits=None)})
    group(both, set_care, "set_care", {"full variant + unknown name": dict(pl=full.handle, name=b"features.9.Block_conv1"),
                                       "unknown name + wrong bytes": dict(name=b"features.9.Block_conv1", bytes=4)})
    single["care_misses:before set_care, after refused installs"] = misses()
    ones = {b.name: np.full((b.groups, minimise.n_words(b.fan_in_bits)), 0xFFFFFFFF, dtype=np.uint32) for b in blocks}
    for b in blocks:
        _lib.check(lib.ttnet_plan_set_care(S.handle, b.name.encode(), host(ones[b.name]), ones[b.name].nbytes))
    mem("usage and care on")
    group(single, misses, "care_misses", {"null rows": dict(rows=None), "rows misaligned": dict(rows=rows.data_ptr() + 2), "lane -1": dict(lane=-1),
                                          "lane 2": dict(lane=2), "no forward has run": {}})
    group(both, misses, "care_misses", {"null rows + lane 2": dict(rows=None, lane=2), "rows misaligned + lane 2": dict(rows=rows.data_ptr() + 2, lane=2),
                                        "lane 2 (no forward anywhere)": dict(lane=2)})
    # -- tables
    for tag, entry in (("get_table", get_table), ("set_table", set_table)):
        buf = "dst" if tag == "get_table" else "src"
        group(single, entry, tag, {
            "null plan": dict(pl=None), "null name": dict(name=None), "null buffer": {buf: None}, "unknown name": dict(name=b"features.9.Block_conv1"),
            "wrong bytes": dict(bytes=table.nbytes - 1), "full variant": dict(pl=full.handle, name=b"features.4.Block_conv1"),
            "unfinalized": dict(pl=raw.handle)})
        group(both, entry, tag, {"null buffer + unknown name": {buf: None, "name": b"features.9.Block_conv1"},
                                 "unknown name + wrong bytes": dict(name=b"features.9.Block_conv1", bytes=1),
                                 "unfinalized + wrong bytes": dict(pl=raw.handle, bytes=1)})
    # -- one forward on lane 0
    assert forward() == [0, ""]
    torch.cuda.synchronize(dev)
    group(single, read_stage, "read_stage", {"n 0": dict(n=0), "n 5": dict(n=5), "unknown stage": dict(stage=b"features.9"),
                                             "wrong bytes": dict(bytes=stage.nbytes - 8), "good": {}})
    group(both, read_stage, "read_stage", {"n 5 + unknown stage": dict(n=5, stage=b"features.9"), "unknown stage + wrong bytes": dict(stage=b"features.9", bytes=8)})
    group(single, usage_add, "usage_add", {"no forward has run on lane 1, one on lane 0": dict(lane=1)})
    group(single, misses, "care_misses", {"no forward has run on lane 1, one on lane 0": dict(lane=1)})
    group(both, misses, "care_misses", {"rows misaligned + no forward on lane 1": dict(rows=rows.data_ptr() + 2, lane=1)})
    group(single, query, "query", {"last_n:0 after": {}})
    memory["small:last_n:0 after"] = q.value
    group(single, query, "query", {"last_n:1 after": dict(what=b"last_n:1")})
    memory["small:last_n:1 after"] = q.value
    # -- the launches of the usage add and of care_misses, with a care set on every table and on one block's convf alone
    timings["small:forward_lane"] = profiled(S, forward)
    timings["small:table_usage_add"] = profiled(S, usage_add)
    timings["small:care_misses, every table"] = profiled(S, misses)
    for b in blocks:
        if b.name != "features.5.Block_convf":
            _lib.check(lib.ttnet_plan_set_care(S.handle, b.name.encode(), None, 0))
    timings["small:care_misses, features.5.Block_convf alone"] = profiled(S, misses)
    _lib.check(lib.ttnet_plan_set_care(S.handle, b"features.5.Block_convf", None, 0))
    _lib.check(lib.ttnet_plan_set_care(S.handle, b"features.6.Block_conv2", host(ones["features.6.Block_conv2"]), ones["features.6.Block_conv2"].nbytes))
    timings["small:care_misses, features.6.Block_conv2 alone"] = profiled(S, misses)
    mem("usage on, one care set")
    _lib.check(lib.ttnet_plan_table_usage_enable(S.handle, 0))
    mem("one care set")
    _lib.check(lib.ttnet_plan_clear_care(S.handle))
    mem("both off")
    torch.cuda.synchronize(dev)
    for p in (S, raw, full, V):
        p.close()


def record_valexnet(dev, out):
    lib = _lib.load()
    single, both, timings, memory = out["single"], out["precedence"], out["timings"], out["memory"]
    V, raw, S = make_plan("valexnet", dev), make_plan("valexnet", dev, False), make_plan("small", dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    x = torch.from_numpy(np.ascontiguousarray(synth.synth_images_u8(MAX_BATCH, hw=(32, 32)).transpose(0, 2, 3, 1))).to(dev)
    xcur = x.clone()
    cls = torch.tensor([3, 5, 7, 1], dtype=torch.int32, device=dev)
    rows = torch.zeros((MAX_BATCH, 4), dtype=torch.float64, device=dev)
    planes = torch.zeros(MAX_BATCH * 2 * (STEM_ROWS + FEAT_ROWS), dtype=torch.int64, device=dev)
    pmap = torch.zeros((MAX_BATCH, 64, 2), dtype=torch.float64, device=dev)        # 4 x 4 patches at stride 4: 8 x 8 positions
    worst = torch.zeros(MAX_BATCH, dtype=torch.int32, device=dev)
    active = torch.zeros(MAX_BATCH, dtype=torch.int32, device=dev)
    stem = torch.zeros((2, N, 64, 10), dtype=torch.int64, device=dev)
    cand = torch.zeros((MAX_BATCH, 8, 32, 32, 3), dtype=torch.uint8, device=dev)
    gains = torch.zeros((MAX_BATCH, 64, 10, 10), dtype=torch.float64, device=dev)
    logits = torch.zeros((MAX_BATCH * 8, 10), dtype=torch.float32, device=dev)
    arows = torch.zeros((MAX_BATCH, 8), dtype=torch.int32, device=dev)
    P = lambda t, off=0: t.data_ptr() + off                                       # noqa: E731

    certify = Entry(lib, "ttnet_certify_u8", pl=V.handle, lane=0, x=P(x), n=N, classes=P(cls), eps=1.0, enum_bits=10, min_margin=1e-6,
                    rows=P(rows), planes=P(planes), stream=s)
    box = Entry(lib, "ttnet_certify_box_u8", pl=V.handle, lane=0, lo=P(x), hi=P(x), n=N, classes=P(cls), enum_bits=10, min_margin=1e-6,
                rows=P(rows), planes=None, stream=s)
    patch = Entry(lib, "ttnet_certify_patch_u8", pl=V.handle, lane=0, x=P(x), n=N, classes=P(cls), h=4, w=4, stride=4, amp=1, enum_bits=10,
                  min_margin=1e-6, rows=P(rows), map=P(pmap), stream=s)
    propose = Entry(lib, "ttnet_attack_propose_u8", pl=V.handle, lane=0, x0=P(x), xcur=P(xcur), n=N, classes=P(cls), worst=P(worst),
                    planes=P(stem), levels=2, active=P(active), cand=P(cand), gains=P(gains), stream=s)
    select = Entry(lib, "ttnet_attack_select_u8", pl=V.handle, cand=P(x), logits=P(logits), n=N, n_cand=1, classes=P(cls), min_margin=0.0,
                   x0=P(x), xcur=P(xcur), rows=P(arows), worst=P(worst), active=P(active), round=0, stream=s)
    forward_u8 = Entry(lib, "ttnet_forward_u8", pl=V.handle, lane=0, x=P(x), n=N, out=P(logits), stream=s)

    def group(dst, entry, prefix, cases):                                         # (every case here is a refused call)
        for tag, kw in cases.items():
            assert f"{prefix}:{tag}" not in dst
            dst[f"{prefix}:{tag}"] = entry(**kw)
            assert dst[f"{prefix}:{tag}"][0] < 0, (prefix, tag)

    shared ={"null plan": dict(pl=None), "null classes": dict(classes=None), "null rows": dict(rows=None), "classes misaligned": dict(classes=P(cls, 2)),
              "rows misaligned": dict(rows=P(rows, 4)), "lane -1": dict(lane=-1), "lane 2": dict(lane=2), "n 0": dict(n=0), "n 5": dict(n=5),
              "enum_bits -1": dict(enum_bits=-1), "enum_bits 13": dict(enum_bits=13), "nan margin": dict(min_margin=NAN),
              "wrong variant": dict(pl=S.handle), "unfinalized": dict(pl=raw.handle)}
    group(single, certify, "certify_u8", {
        **shared, "null x": dict(x=None), "x misaligned": dict(x=P(x, 1)), "planes misaligned": dict(planes=P(planes, 4)), "eps -0.5": dict(eps=-0.5),
        "eps inf": dict(eps=INF), "eps nan": dict(eps=NAN)})
    group(single, box, "certify_box_u8", {
        **shared, "null lo": dict(lo=None), "null hi": dict(hi=None), "lo misaligned": dict(lo=P(x, 1)), "hi misaligned": dict(hi=P(x, 2)),
        "planes misaligned": dict(planes=P(planes, 4))})
    group(single, patch, "certify_patch_u8", {
        **shared, "null x": dict(x=None), "null map": dict(map=None), "x misaligned": dict(x=P(x, 1)), "map misaligned": dict(map=P(pmap, 4)),
        "patch 0x1": dict(h=0, w=1), "patch 9x1": dict(h=9, w=1), "patch 1x0": dict(h=1, w=0), "patch 1x9": dict(h=1, w=9), "stride 0": dict(stride=0),
        "stride 33": dict(stride=33), "amp 0": dict(amp=0), "amp 256": dict(amp=256)})
    # each adjacent pair of the certificate's checks, in their order
    group(both, certify, "certify_u8", {
        "wrong variant + null x": dict(pl=S.handle, x=None), "null x + unfinalized": dict(pl=raw.handle, x=None), "unfinalized + n 0": dict(pl=raw.handle, n=0),
        "n 0 + null classes": dict(n=0, classes=None), "null classes + eps nan": dict(classes=None, eps=NAN), "eps -0.5 + enum_bits 13": dict(eps=-0.5, enum_bits=13),
        "enum_bits 13 + rows misaligned": dict(enum_bits=13, rows=P(rows, 4)), "nan margin + planes misaligned": dict(min_margin=NAN, planes=P(planes, 4)),
        "rows misaligned + lane 2": dict(rows=P(rows, 4), lane=2)})
    group(both, box, "certify_box_u8", {
        "wrong variant + null hi": dict(pl=S.handle, hi=None), "unfinalized + null hi": dict(pl=raw.handle, hi=None), "n 5 + null hi": dict(n=5, hi=None),
        "null hi + enum_bits 13": dict(hi=None, enum_bits=13), "nan margin + hi misaligned": dict(min_margin=NAN, hi=P(x, 2)),
        "hi misaligned + lane -1": dict(hi=P(x, 2), lane=-1)})
    group(both, patch, "certify_patch_u8", {
        "wrong variant + patch 9x1": dict(pl=S.handle, h=9, w=1), "unfinalized + patch 9x1": dict(pl=raw.handle, h=9, w=1),
        "unfinalized + null map": dict(pl=raw.handle, map=None), "n 0 + amp 0": dict(n=0, amp=0), "null classes + patch 9x1": dict(classes=None, h=9, w=1),
        "null map + stride 0": dict(map=None, stride=0), "patch 9x1 + enum_bits 13": dict(h=9, w=1, enum_bits=13),
        "amp 256 + nan margin": dict(amp=256, min_margin=NAN), "enum_bits 13 + map misaligned": dict(enum_bits=13, map=P(pmap, 4)),
        "map misaligned + lane 2": dict(map=P(pmap, 4), lane=2), "amp 0 + lane 2": dict(amp=0, lane=2)})
    # -- the attack entries; no forward has run yet
    group(single, propose, "attack_propose", {
        "null plan": dict(pl=None), "null x0": dict(x0=None), "null xcur": dict(xcur=None), "null classes": dict(classes=None), "null worst": dict(worst=None),
        "null planes": dict(planes=None), "null active": dict(active=None), "null cand": dict(cand=None), "x0 misaligned": dict(x0=P(x, 1)),
        "xcur misaligned": dict(xcur=P(xcur, 1)), "classes misaligned": dict(classes=P(cls, 2)), "worst misaligned": dict(worst=P(worst, 2)),
        "active misaligned": dict(active=P(active, 2)), "cand misaligned": dict(cand=P(cand, 1)), "planes misaligned": dict(planes=P(stem, 4)),
        "gains misaligned": dict(gains=P(gains, 4)), "levels -1": dict(levels=-1), "levels 65": dict(levels=65), "lane -1": dict(lane=-1), "lane 2": dict(lane=2),
        "n 0": dict(n=0), "n 5": dict(n=5), "no forward has run": {}, "wrong variant": dict(pl=S.handle), "unfinalized": dict(pl=raw.handle)})
    group(both, propose, "attack_propose", {
        "wrong variant + null x0": dict(pl=S.handle, x0=None), "null cand + unfinalized": dict(pl=raw.handle, cand=None), "unfinalized + n 5": dict(pl=raw.handle, n=5),
        "n 5 + null xcur": dict(n=5, xcur=None), "null xcur + levels 65": dict(xcur=None, levels=65), "levels 65 + planes misaligned": dict(levels=65, planes=P(stem, 4)),
        "planes misaligned + lane 2": dict(planes=P(stem, 4), lane=2), "lane 2 + no forward has run": dict(lane=2)})
    group(single, select, "attack_select", {
        "null plan": dict(pl=None), "null cand": dict(cand=None), "null logits": dict(logits=None), "null classes": dict(classes=None), "null x0": dict(x0=None),
        "null xcur": dict(xcur=None), "null rows": dict(rows=None), "null worst": dict(worst=None), "null active": dict(active=None), "n_cand 0": dict(n_cand=0),
        "n_cand 9": dict(n_cand=9), "round -1": dict(round=-1), "nan margin": dict(min_margin=NAN), "cand misaligned": dict(cand=P(x, 1)),
        "logits misaligned": dict(logits=P(logits, 2)), "classes misaligned": dict(classes=P(cls, 2)), "x0 misaligned": dict(x0=P(x, 1)),
        "xcur misaligned": dict(xcur=P(xcur, 1)), "worst misaligned": dict(worst=P(worst, 2)), "active misaligned": dict(active=P(active, 2)),
        "rows misaligned": dict(rows=P(arows, 4)), "xcur is cand": dict(xcur=P(x)), "xcur is x0": dict(cand=P(cand), xcur=P(x)), "n 0": dict(n=0), "n 5": dict(n=5),
        "wrong variant": dict(pl=S.handle), "unfinalized": dict(pl=raw.handle)})
    group(both, select, "attack_select", {
        "wrong variant + null cand": dict(pl=S.handle, cand=None), "unfinalized + null rows": dict(pl=raw.handle, rows=None), "n 0 + null rows": dict(n=0, rows=None),
        "null rows + n_cand 9": dict(rows=None, n_cand=9), "n_cand 9 + rows misaligned": dict(n_cand=9, rows=P(arows, 4)),
        "rows misaligned + xcur is cand": dict(rows=P(arows, 4), xcur=P(x))})
    torch.cuda.synchronize(dev)
    for tag, t in dict(rows=rows, planes=planes, map=pmap, cand=cand, gains=gains, attack_rows=arows).items():
        assert not t.any().item(), tag                                            # no refused call launched anything
    # -- the launches of the good calls; the attack as attack_u8 drives it: forward, select (round 0), certificate, propose
    memory["valexnet:workspace_bytes"] = V.query("workspace_bytes")
    timings["valexnet:certify_u8 enum_bits 0"] = profiled(V, lambda: certify(enum_bits=0))
    timings["valexnet:certify_u8 enum_bits 10"] = profiled(V, certify)
    timings["valexnet:certify_u8 enum_bits 10, lane 1, no planes"] = profiled(V, lambda: certify(lane=1, planes=None))
    timings["valexnet:certify_box_u8"] = profiled(V, box)
    # (as recorded: the planes stand in for a missing upper image in the null check, and the call runs as the box [lo, lo])
    single["certify_box_u8:null hi, planes given"] = box(hi=None, planes=P(planes))
    timings["valexnet:certify_patch_u8"] = profiled(V, patch)
    timings["valexnet:forward_u8"] = profiled(V, forward_u8)
    timings["valexnet:attack_select_u8"] = profiled(V, select)
    assert certify(eps=2.0, enum_bits=0, min_margin=0.0) == [0, ""]
    torch.cuda.synchronize(dev)
    stem.copy_(planes[:2 * N * STEM_ROWS].view(2, N, 64, 10))
    timings["valexnet:attack_propose_u8"] = profiled(V, propose)
    group(single, propose, "attack_propose", {"n 2 after a forward of 3": dict(n=2), "lane 1 without a forward": dict(lane=1)})
    memory["valexnet:workspace_bytes after the certificates"] = V.query("workspace_bytes")
    torch.cuda.synchronize(dev)
    for p in (V, raw, S):
        p.close()


def record(dev):
    out = {"single": {}, "precedence": {}, "timings": {}, "memory": {}}
    record_small(dev, out)
    record_valexnet(dev, out)
    return out


@pytest.fixture(scope="module")
def answers():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    got = record(torch.device("cuda", 0))
    with open(GOLDEN) as f:
        return got, json.load(f)


@pytest.mark.parametrize("section", ["single", "precedence", "timings", "memory"])
def test_entries_answer_as_recorded(answers, section):
    got, want = (a[section] for a in answers)
    got = json.loads(json.dumps(got))
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, "\n".join(f"{k}: got {g!r}, recorded {w!r}" for k, (g, w) in diff.items())
    assert len(want) >= {"single": 150, "precedence": 50, "timings": 13, "memory": 20}[section]
