"""JPEG decoding on the device: the ``PIL.Image.open(path).convert("RGB")`` of ``ImageFolder``'s default loader
(main.py:208) in front of the eval transform (utils/preprocess.py:104-108), from compressed file bytes.

    file bytes --pack_jpeg (loader worker: header walk, tables)--> RaggedJpeg --H2D--> decode_ragged (libttnet,
    csrc/jpeg.hip) --> RaggedU8 --> resize_center_crop_u8_ragged --> forward_u8

``parse_header`` walks the markers in front of the first SOS in pure Python (no Pillow, no GPU).  Baseline and
extended Huffman-coded sequential 8-bit files with one scan are decoded on the device: YCbCr with luma sampling 1x1,
2x1 or 2x2 and chroma 1x1, and greyscale.  Everything else is decoded by Pillow in ``pack_jpeg`` (in the worker) and
carried through the same batch as raw pixels that the device copies; nothing is dropped.  The device output is byte
for byte Pillow's (libjpeg's islow IDCT, fancy upsampling, jdcolor.c's tables).

Opt-in: ``pack_jpeg(..., progressive=True)`` / ``collate_jpeg_progressive`` also send complete progressive (SOF2) files
to the device (``parse_progressive`` walks and validates every scan; kind 2 of the batch), byte-identical as well; with
the flag off they take the Pillow fallback as before.
"""
from __future__ import annotations

import ctypes as C
import io
import os
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .preprocess import MAX_SIDE, RaggedU8, _StickyCount, imgnet_views_forward, resize_center_crop_u8_ragged

KIND_JPEG, KIND_RAW, KIND_PROGRESSIVE = 0, 1, 2
TABLE_BYTES = 2048        # per-image table block: uint16 quant[3][64] (zig-zag) + [3][dc, ac] x (counts[16], symbols[256])
_HUFF_OFF = 384
_HUFF_BYTES = 272
# ttnet_jpeg_desc (include/ttnet.h), 80 bytes
JDESC_DTYPE = np.dtype([("data_offset", "<i8"), ("data_bytes", "<i8"), ("table_offset", "<i8"), ("out_offset", "<i8"),
                        ("block_offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("kind", "<i4"), ("ncomp", "<i4"),
                        ("restart_interval", "<i4"), ("comp", "u1", (3, 4)), ("reserved", "<i4", (2,))])
assert JDESC_DTYPE.itemsize == 80 == C.sizeof(_lib.JpegDesc)
# kind 2 (progressive): ttnet_jpeg_scan records (32 bytes) at SCAN_OFF of the table block, a pool of Huffman tables behind it
MAX_SCANS = 32            # TTNET_JPEG_MAX_SCANS
SCAN_OFF = _HUFF_OFF
JSCAN_DTYPE = np.dtype([("data_offset", "<u4"), ("data_bytes", "<u4"), ("restart_interval", "<u2"), ("ncomp", "u1"),
                        ("slot", "u1"), ("comp", "u1", (4,)), ("ss", "u1"), ("se", "u1"), ("ah", "u1"), ("al", "u1"),
                        ("table", "u1", (4,)), ("reserved", "<i4", (2,))])
assert JSCAN_DTYPE.itemsize == 32 == C.sizeof(_lib.JpegScan) and SCAN_OFF + MAX_SCANS * 32 <= TABLE_BYTES
_JDESC_WORDS = JDESC_DTYPE.itemsize // 8

_SOF_NAMES = {0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic-coded sequential (SOF9)", 0xCA: "arithmetic-coded progressive (SOF10)",
              0xCB: "arithmetic-coded lossless (SOF11)", 0xCD: "arithmetic-coded differential (SOF13)",
              0xCE: "arithmetic-coded differential progressive (SOF14)", 0xCF: "arithmetic-coded differential lossless (SOF15)"}


@dataclass
class Unsupported:
    """A file the device does not decode, and why."""
    reason: str


@dataclass(kw_only=True)
class JpegFrame:
    """The frame of a file, as both decoders need it: the SOF's size and components, the quantisation tables and the
    colour-space markers."""
    h: int
    w: int
    comps: List[Tuple[int, int, int, int]]       # per frame component: (id, h_samp, v_samp, quant table)
    qt: Dict[int, List[int]]                     # quant tables, zig-zag order, as in DQT
    jfif: bool = False
    adobe_transform: Optional[int] = None

    @property
    def ncomp(self) -> int:
        return len(self.comps)

    @property
    def sampling(self) -> List[Tuple[int, int]]:
        return [(c[1], c[2]) for c in self.comps]

    def mcus(self) -> Tuple[int, int, int]:
        """(MCU columns, MCU rows, blocks per MCU)."""
        if self.ncomp == 1:
            return (self.w + 7) // 8, (self.h + 7) // 8, 1
        hs, vs = self.comps[0][1], self.comps[0][2]
        return (self.w + 8 * hs - 1) // (8 * hs), (self.h + 8 * vs - 1) // (8 * vs), hs * vs + 2

    def blocks(self) -> int:
        mx, my, b = self.mcus()
        return mx * my * b


@dataclass(kw_only=True)
class JpegHeader(JpegFrame):
    """What the device decoder needs, from the markers before the first SOS."""
    sof: int                                     # 0 or 1
    scan_tables: List[Tuple[int, int]]           # per component, in frame order: (dc table, ac table)
    dht: Dict[Tuple[int, int], Tuple[List[int], List[int]]] = field(default_factory=dict)  # (class, id) -> counts, symbols
    restart_interval: int = 0
    scan_offset: int = 0                         # first byte of the entropy-coded data

    def segments(self) -> int:
        mx, my, _ = self.mcus()
        ri = self.restart_interval
        return 1 if ri == 0 else (mx * my + ri - 1) // ri


@dataclass
class ProgressiveScan:
    """One scan of a progressive file: ``comps`` are frame component indices (increasing), ``tables`` the Huffman
    table in force for each of them when the SOS was read (DC tables in a DC scan, the AC table in an AC scan, as
    (counts, symbols); None in a DC refinement, which reads raw bits), [data_start, data_end) the entropy-coded
    bytes in the file."""
    comps: List[int]
    ss: int
    se: int
    ah: int
    al: int
    restart_interval: int
    tables: List[Optional[Tuple[List[int], List[int]]]]
    data_start: int
    data_end: int
    slot: int = 0                                # 4 * round + wave of the device schedule (_schedule)


@dataclass(kw_only=True)
class ProgressiveHeader(JpegFrame):
    """What the device decoder needs of a progressive (SOF2) file: the frame and every scan."""
    scans: List[ProgressiveScan]
    rounds: int = 0

    @property
    def restart_interval(self) -> int:
        """The first scan's (DRI may change between scans; each scan carries its own)."""
        return self.scans[0].restart_interval


def _check_huffman(counts: List[int], symbols: List[int], dc: bool) -> Optional[str]:
    """libjpeg's jpeg_make_d_derived_tbl checks: at most 256 symbols, no code overflows its length (the all-ones code
    of a length is never assigned), DC symbols at most 15."""
    if sum(counts) > 256 or sum(counts) != len(symbols):
        return "Huffman table with more than 256 symbols"
    code = 0
    for l in range(1, 17):
        code += counts[l - 1]
        if code >= (1 << l):
            return "Huffman table with an overfull code length"
        code <<= 1
    if dc and any(s > 15 for s in symbols):
        return "DC Huffman table with a symbol above 15"
    return None


def _read_dqt(seg, qt) -> Optional[str]:
    """A DQT segment's tables into ``qt`` (zig-zag order, as stored); an error string if malformed."""
    j = 0
    while j < len(seg):
        pq, tq = seg[j] >> 4, seg[j] & 15
        size = 64 * (pq + 1)
        if pq > 1 or tq > 3 or j + 1 + size > len(seg):
            return "malformed DQT"
        vals = seg[j + 1:j + 1 + size]
        qt[tq] = list(vals) if pq == 0 else [(vals[2 * k] << 8) | vals[2 * k + 1] for k in range(64)]
        j += 1 + size
    return None


def _read_dht(seg, dht) -> Optional[str]:
    """A DHT segment's tables into ``dht`` ((class, id) -> counts, symbols); an error string if malformed."""
    j = 0
    while j < len(seg):
        if j + 17 > len(seg):
            return "malformed DHT"
        tc, th = seg[j] >> 4, seg[j] & 15
        counts = list(seg[j + 1:j + 17])
        total = sum(counts)
        if tc > 1 or th > 3 or j + 17 + total > len(seg):
            return "malformed DHT"
        syms = list(seg[j + 17:j + 17 + total])
        err = _check_huffman(counts, syms, tc == 0)
        if err:
            return err
        dht[(tc, th)] = (counts, syms)
        j += 17 + total
    return None


def _read_sos(seg):
    """An SOS payload as ([(component id, dc table, ac table)], Ss, Se, Ah, Al); None if malformed."""
    if len(seg) < 1 or len(seg) < 1 + 2 * seg[0] + 3:
        return None
    ns = seg[0]
    sel = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
    return sel, seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15


class _Walk:
    """The marker walk behind ``parse_header`` and ``parse_progressive``: SOI, fill FFs, stand-alone markers, segment
    lengths, and the segments that mean the same to both -- JFIF, Adobe, DQT, DHT, DAC, DRI and the SOF payload, kept
    in ``jfif``, ``adobe``, ``qt``, ``dht``, ``ri`` and ``sof``.  Iterating yields ``(marker, payload)`` for what a client
    decides about -- the frame just read (SOF0 / SOF1 / SOF2), SOS (a frame has been read by then), DNL -- with ``i``
    behind the segment, and may be resumed after a ``break``.  It ends with ``error`` set at a malformed or refused
    file, with ``eoi`` set at EOI, with neither at the end of the buffer, and never reads outside the buffer.

    ``progressive`` names the client and may be switched off during the walk: ``parse_progressive`` takes SOF2 for a
    frame where ``parse_header`` refuses it by name, and each words a cut-off length and a misplaced SOI its own way."""

    def __init__(self, buf, progressive: bool):
        self.b = bytes(buf)
        self.progressive = progressive
        self.i = 2                               # behind the segment last yielded
        self.qt: Dict[int, List[int]] = {}
        self.dht: Dict[Tuple[int, int], Tuple[List[int], List[int]]] = {}
        self.sof = None                          # (marker, h, w, components)
        self.ri, self.jfif, self.adobe = 0, False, None
        self.scans = 0                           # scans passed by skip_scan_data
        self.eoi, self.error = False, None
        self._events = self._run()

    def __iter__(self):
        return self._events

    def _run(self):
        b, n, i = self.b, len(self.b), 2
        if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
            self.error = "not a JPEG file (no SOI marker)"
            return
        while i < n:
            if b[i] != 0xFF:
                self.error = f"garbage between markers at byte {i}"
                return
            while i < n and b[i] == 0xFF:
                i += 1
            if i >= n:
                return
            m = b[i]
            i += 1
            if m == 0x01 or 0xD0 <= m <= 0xD7:
                continue
            if m == 0xD9:
                self.eoi = True
                return
            if m == 0xD8 or m == 0x00:
                self.error = f"unexpected marker 0xFF{m:02X}" + ("" if self.progressive else " in the header")
                return
            if i + 2 > n:
                self.error = f"{'file' if self.progressive else 'header'} ends inside a marker length"
                return
            length = (b[i] << 8) | b[i + 1]
            if length < 2 or i + length > n:
                self.error = f"marker 0xFF{m:02X} runs past the end of the file"
                return
            seg = b[i + 2:i + length]
            i += length
            self.error = self._segment(m, seg)
            if self.error is not None:
                return
            if m in (0xC0, 0xC1, 0xC2, 0xDA, 0xDC):
                self.i = i
                yield m, seg
                i = self.i                       # (skip_scan_data may have moved it)

    def _segment(self, m: int, seg: bytes) -> Optional[str]:
        """Digests one marker segment; the reason if the file ends here."""
        if m == 0xE0 and seg[:5] == b"JFIF\0":
            self.jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            self.adobe = seg[11]
        elif m == 0xDB:
            return "quantisation tables redefined between scans" if self.scans else _read_dqt(seg, self.qt)
        elif m == 0xC4:
            return _read_dht(seg, self.dht)
        elif m == 0xCC:
            return "arithmetic coding (DAC)"
        elif m == 0xDD:
            if len(seg) < 2:
                return "malformed DRI"
            self.ri = (seg[0] << 8) | seg[1]
        elif m in _SOF_NAMES and not (m == 0xC2 and self.progressive):
            return _SOF_NAMES[m]
        elif m in (0xC0, 0xC1, 0xC2):
            if self.sof is not None:
                return "more than one SOF"
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                return "malformed SOF"
            p, h, w, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if p != 8:
                return f"{p}-bit samples"
            self.sof = (m, h, w, [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k])
                                  for k in range(nf)])
        elif m == 0xDA and self.sof is None:
            return "SOS before SOF"
        return None

    def skip_scan_data(self) -> Tuple[int, int]:
        """After an SOS: moves behind the entropy-coded data that starts at ``i`` and returns its [start, end).  It
        ends at the FF of the next marker other than FF00 / RSTn (fill FFs in front of it belong to the data), or at
        the end of the file."""
        b, n, start = self.b, len(self.b), self.i
        i = start
        while True:
            j = b.find(b"\xff", i)
            if j < 0 or j + 1 >= n:
                j = n
                break
            m = b[j + 1]
            if m == 0x00 or 0xD0 <= m <= 0xD7:
                i = j + 2
            elif m == 0xFF:
                i = j + 1
            else:
                break
        self.i = j
        self.scans += 1
        return start, j


def parse_header(buf) -> "JpegHeader | Unsupported":
    """Marker walk up to the first SOS.  Returns a JpegHeader if the device decodes the file, otherwise
    Unsupported(reason).  Never reads outside ``buf``; a truncated or malformed header is Unsupported."""
    return _sequential(_Walk(buf, progressive=False))


def _sequential(walk: _Walk) -> "JpegHeader | Unsupported":
    """Reads on to the first SOS and classifies a sequential frame (a DNL in front of it is passed over)."""
    walk.progressive = False
    for m, seg in walk:
        if m == 0xDA:
            return _classify(walk, seg)
    if walk.error is not None:
        return Unsupported(walk.error)
    return Unsupported("EOI before any scan" if walk.eoi else "header ends before the first SOS")


def _classify_frame(h, w, comps) -> Optional[str]:
    """The frame rules shared by sequential and progressive files: size and component count."""
    nf = len(comps)
    if h < 1 or w < 1:
        return "height given by a DNL marker" if h == 0 else "zero width"
    if h > MAX_SIDE or w > MAX_SIDE:
        return f"{w}x{h} is beyond {MAX_SIDE} px"
    if nf == 4:
        return "4 components (CMYK / YCCK)"
    if nf not in (1, 3):
        return f"{nf} components"
    return None


def _classify_colour(comps, jfif, adobe) -> Optional[str]:
    """Colour space and sampling, known once every marker in front of the first SOS has been read."""
    if len(comps) == 3:
        ids = tuple(c[0] for c in comps)
        if adobe is not None and adobe != 1:
            return f"Adobe colour transform {adobe} (not YCbCr)"
        if adobe is None and not jfif and ids != (1, 2, 3):
            return f"3 components with ids {ids} and no JFIF / Adobe marker (colour space unknown)"
        ys = (comps[0][1], comps[0][2])
        if ys not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return f"sampling {[(c[1], c[2]) for c in comps]}"
    elif not (1 <= comps[0][1] <= 4 and 1 <= comps[0][2] <= 4):
        return "bad sampling factors"
    return None


def _classify(walk: _Walk, seg) -> "JpegHeader | Unsupported":
    """The first SOS of a sequential file: a JpegHeader if this one scan is all the device has to decode."""
    sos = _read_sos(seg)
    if sos is None:
        return Unsupported("malformed SOS")
    scomps, ss, se, ah, al = sos
    m, h, w, comps = walk.sof
    err = _classify_frame(h, w, comps)
    if err:
        return Unsupported(err)
    if len(scomps) != len(comps):
        return Unsupported("multi-scan sequential file (a scan without every component)")
    if [c[0] for c in scomps] != [c[0] for c in comps]:
        return Unsupported("scan components in another order than the frame's")
    if (ss, se, ah, al) != (0, 63, 0, 0):
        return Unsupported("sequential scan with a spectral selection other than 0..63")
    err = _classify_colour(comps, walk.jfif, walk.adobe)
    if err:
        return Unsupported(err)
    for c in comps:
        if c[3] not in walk.qt:
            return Unsupported(f"quantisation table {c[3]} is not defined")
    tables = []
    for (_, td, ta) in scomps:
        if (0, td) not in walk.dht or (1, ta) not in walk.dht:
            return Unsupported(f"Huffman table DC {td} / AC {ta} is not defined")
        tables.append((td, ta))
    return JpegHeader(h=h, w=w, sof=m - 0xC0, comps=comps, scan_tables=tables, qt=walk.qt, dht=walk.dht,
                      restart_interval=walk.ri, scan_offset=walk.i, jfif=walk.jfif, adobe_transform=walk.adobe)


def _schedule(scans: List[ProgressiveScan]) -> int:
    """Assigns each scan its slot (4 * round + wave) on the device: a scan runs in a later round than every earlier
    scan that touches one of its (component, coefficient) pairs (a refinement after the pass it refines; DC and AC
    bands, and different components, are independent), four scans at most per round, long scans placed first.
    Returns the round count."""
    deps = [[i for i in range(j) if set(s.comps) & set(scans[i].comps) and s.ss <= scans[i].se and scans[i].ss <= s.se]
            for j, s in enumerate(scans)]
    level = []
    for j in range(len(scans)):
        level.append(1 + max((level[i] for i in deps[j]), default=-1))
    order = sorted(range(len(scans)), key=lambda j: (level[j], scans[j].data_start - scans[j].data_end, j))
    load: List[int] = []
    rnd: Dict[int, int] = {}
    for j in order:
        r = 1 + max((rnd[i] for i in deps[j]), default=-1)
        while r < len(load) and load[r] == 4:
            r += 1
        if r == len(load):
            load.append(0)
        scans[j].slot = 4 * r + load[r]
        load[r] += 1
        rnd[j] = r
    return len(load)


def parse_progressive(buf) -> "ProgressiveHeader | Unsupported":
    """Marker walk over the whole of a progressive (SOF2) file: the frame, then every scan with its spectral band,
    bit positions, restart interval, the Huffman tables defined at that point and the byte range of its data.
    Returns a ProgressiveHeader if the device decodes the file under ``pack_jpeg(..., progressive=True)``, otherwise
    Unsupported(reason); a file that is not SOF2 gets the reason ``parse_header`` gives or "not progressive".  The
    progression is validated as libjpeg's jdphuff.c does and must be complete (every coefficient of every component
    refined down to bit 0), because libjpeg smooths blocks of an incomplete one.  Never reads outside ``buf``."""
    walk = _Walk(buf, progressive=True)
    scans: List[ProgressiveScan] = []
    bits: List[List[int]] = []                   # per component, per coefficient: the bit position reached, -1: none
    for m, seg in walk:
        if m == 0xDC:
            return Unsupported("height given by a DNL marker")
        if m in (0xC0, 0xC1):                    # a sequential frame: the reason is the sequential walk's
            r = _sequential(walk)
            return r if isinstance(r, Unsupported) else Unsupported("not progressive (sequential: parse_header)")
        _, h, w, comps = walk.sof
        if m == 0xC2:
            err = _classify_frame(h, w, comps)
            if err:
                return Unsupported(err)
            bits = [[-1] * 64 for _ in comps]
            continue
        if len(scans) >= MAX_SCANS:
            return Unsupported(f"more than {MAX_SCANS} scans")
        if not scans:
            err = _classify_colour(comps, walk.jfif, walk.adobe)
            if err:
                return Unsupported(err)
        sc = _read_progressive_sos(seg, comps, walk.qt, walk.dht, bits, walk.ri)
        if isinstance(sc, Unsupported):
            return sc
        sc.data_start, sc.data_end = walk.skip_scan_data()
        if sc.data_end == sc.data_start:
            return Unsupported(f"scan {len(scans)} has no entropy-coded data")
        scans.append(sc)
    if walk.error is not None:
        return Unsupported(walk.error)
    if walk.sof is None:
        return Unsupported("no SOF before the end of the file")
    if not scans:
        return Unsupported("no scan before the end of the file")
    for c, cb in enumerate(bits):
        for k, v in enumerate(cb):
            if v != 0:
                return Unsupported(f"incomplete progression (component {c}, coefficient {k} "
                                   f"{'never coded' if v < 0 else f'stops at bit {v}'}): libjpeg would smooth it")
    _, h, w, comps = walk.sof
    hd = ProgressiveHeader(h=h, w=w, comps=comps, qt=walk.qt, scans=scans, jfif=walk.jfif, adobe_transform=walk.adobe)
    hd.rounds = _schedule(scans)
    return hd


def _read_progressive_sos(seg, comps, qt, dht, bits, ri) -> "ProgressiveScan | Unsupported":
    """One SOS header of a progressive file, checked against T.81 G.1.1.1 the way jdphuff.c does (and stricter: what
    libjpeg only warns about is refused); updates ``bits``."""
    sos = _read_sos(seg)
    if sos is None:
        return Unsupported("malformed SOS")
    sel, ss, se, ah, al = sos
    ns = len(sel)
    if ns < 1 or ns > len(comps):
        return Unsupported(f"scan with {ns} components")
    ids = [c[0] for c in comps]
    idx = []
    for cid, _, _ in sel:
        if cid not in ids:
            return Unsupported(f"scan names component {cid}, which the frame does not have")
        idx.append(ids.index(cid))
    if any(a >= c for a, c in zip(idx, idx[1:])):
        return Unsupported("scan components in another order than the frame's")
    if ss > se or se > 63 or al > 13 or ah > 13:
        return Unsupported(f"bad progression parameters Ss {ss} Se {se} Ah {ah} Al {al}")
    if ss == 0 and se != 0:
        return Unsupported(f"scan mixes DC and AC coefficients (Ss 0, Se {se})")
    if ss > 0 and ns != 1:
        return Unsupported("AC scan with more than one component")
    if ah != 0 and al != ah - 1:
        return Unsupported(f"refinement scan with Al {al} other than Ah - 1 ({ah - 1})")
    for c in idx:
        if comps[c][3] not in qt:
            return Unsupported(f"quantisation table {comps[c][3]} is not defined")
        if ss > 0 and bits[c][0] < 0:
            return Unsupported(f"AC scan of component {c} before its DC scan")
        for k in range(ss, se + 1):
            have = bits[c][k]
            if have == 0:
                return Unsupported(f"component {c}, coefficient {k} is coded again after its last bit")
            if ah != (0 if have < 0 else have):
                return Unsupported(f"out-of-order refinement (component {c}, coefficient {k}: Ah {ah} after "
                                   f"{'no scan' if have < 0 else f'Al {have}'})")
            bits[c][k] = al
    tables: List[Optional[Tuple[List[int], List[int]]]] = []
    for (_, td, ta) in sel:
        if ss == 0 and ah != 0:
            tables.append(None)
            continue
        key = (0, td) if ss == 0 else (1, ta)
        if key not in dht:
            return Unsupported(f"Huffman table {'DC' if ss == 0 else 'AC'} {key[1]} is not defined")
        tables.append(dht[key])
    return ProgressiveScan(comps=idx, ss=ss, se=se, ah=ah, al=al, restart_interval=ri, tables=tables, data_start=0,
                           data_end=0)


def _pillow_decode(item, name: str, reason: str) -> np.ndarray:
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"pack_jpeg: {name} is not decoded on the device ({reason}) and Pillow, which decodes "
                           f"such files on the host, is not importable: {e}") from None
    try:
        return np.asarray(Image.open(io.BytesIO(bytes(item))).convert("RGB"))
    except Exception as e:        # noqa: BLE001 -- name the file
        raise RuntimeError(f"pack_jpeg: {name} is not decoded on the device ({reason}) and Pillow fails on it: {e}") from e


class RaggedJpeg:
    """A batch of compressed images: ``data`` (uint8 [bytes]: per JPEG item a table block and its entropy-coded
    data, per raw item its uint8 HWC pixels, every item 16-byte aligned), ``desc`` (int64 [n, 10]: the 80-byte
    ttnet_jpeg_desc records) and the header totals the device call needs: coefficient blocks, output bytes, the
    largest height and width.  Move it with ``.to(device, non_blocking=True)``; ``DataLoader(pin_memory=True)``
    calls ``.pin_memory()``."""

    def __init__(self, data: torch.Tensor, desc: torch.Tensor, n_blocks: int, out_bytes: int, max_h: int, max_w: int,
                 reasons: Optional[List[Optional[str]]] = None):
        if data.dtype != torch.uint8 or data.dim() != 1 or desc.dtype != torch.int64 or desc.dim() != 2 or \
                desc.shape[1] != _JDESC_WORDS:
            raise RuntimeError(f"RaggedJpeg: expected uint8 [bytes] and int64 [n,{_JDESC_WORDS}], got {data.dtype} "
                               f"{tuple(data.shape)}, {desc.dtype} {tuple(desc.shape)}")
        self.data, self.desc = data, desc
        self.n_blocks, self.out_bytes, self.max_h, self.max_w = int(n_blocks), int(out_bytes), int(max_h), int(max_w)
        self.reasons = reasons if reasons is not None else [None] * desc.shape[0]

    def __len__(self) -> int:
        return self.desc.shape[0]

    @property
    def device(self) -> torch.device:
        return self.data.device

    def _like(self, data, desc) -> "RaggedJpeg":
        return RaggedJpeg(data, desc, self.n_blocks, self.out_bytes, self.max_h, self.max_w, self.reasons)

    def to(self, device, non_blocking: bool = False) -> "RaggedJpeg":
        return self._like(self.data.to(device, non_blocking=non_blocking), self.desc.to(device, non_blocking=non_blocking))

    def pin_memory(self) -> "RaggedJpeg":
        return self._like(self.data.pin_memory(), self.desc.pin_memory())

    def descriptors(self) -> np.ndarray:
        return self.desc.cpu().numpy().view(JDESC_DTYPE).reshape(-1)


def _align16(x: int) -> int:
    return (x + 15) & ~15


def _write_quant(blk: np.ndarray, hd: JpegFrame):
    """The head of a table block: uint16 quant[3][64], zig-zag order, one row per frame component."""
    q = blk[:_HUFF_OFF].view("<u2").reshape(3, 64)
    for k, c in enumerate(hd.comps):
        q[k] = hd.qt[c[3]]


def _write_huffman(buf: np.ndarray, offset: int, table):
    """One Huffman record of _HUFF_BYTES at ``offset``: counts[16], symbols[256]."""
    counts, syms = table
    buf[offset:offset + 16 + len(syms)] = np.frombuffer(bytes(counts) + bytes(syms), dtype=np.uint8)


def table_block(hd: JpegHeader) -> np.ndarray:
    """The TABLE_BYTES table block the device reads for one image (layout: include/ttnet.h, ttnet_jpeg_desc)."""
    blk = np.zeros(TABLE_BYTES, dtype=np.uint8)
    _write_quant(blk, hd)
    for k, (td, ta) in enumerate(hd.scan_tables):
        _write_huffman(blk, _HUFF_OFF + 2 * k * _HUFF_BYTES, hd.dht[(0, td)])
        _write_huffman(blk, _HUFF_OFF + (2 * k + 1) * _HUFF_BYTES, hd.dht[(1, ta)])
    return blk


def progressive_block(hd: ProgressiveHeader) -> Tuple[np.ndarray, np.ndarray]:
    """(table block, Huffman pool) the device reads for one progressive image (layout: include/ttnet.h,
    ttnet_jpeg_scan): quant tables, the scan list with data offsets relative to the first scan's data, and each distinct
    Huffman table once."""
    blk = np.zeros(TABLE_BYTES, dtype=np.uint8)
    _write_quant(blk, hd)
    pool: Dict[Tuple[Tuple[int, ...], Tuple[int, ...]], int] = {}
    base = hd.scans[0].data_start
    rows = []                                    # the JSCAN_DTYPE records, field by field
    for sc in hd.scans:
        table = [0, 0, 0, 0]
        for k, t in enumerate(sc.tables):
            if t is not None:
                table[k] = pool.setdefault((tuple(t[0]), tuple(t[1])), len(pool))
        rows.append((sc.data_start - base, sc.data_end - sc.data_start, sc.restart_interval, len(sc.comps), sc.slot,
                     tuple(sc.comps) + (0,) * (4 - len(sc.comps)), sc.ss, sc.se, sc.ah, sc.al, tuple(table), (0, 0)))
    blk[SCAN_OFF:SCAN_OFF + 32 * len(rows)] = np.array(rows, dtype=JSCAN_DTYPE).view(np.uint8)
    tabs = np.zeros(len(pool) * _HUFF_BYTES, dtype=np.uint8)
    for table, k in pool.items():
        _write_huffman(tabs, k * _HUFF_BYTES, table)
    return blk, tabs


class _Item(NamedTuple):
    """One item of a batch, ready to be laid out: ``pieces`` are the uint8 arrays that go into ``data`` back to back
    (a coded image: its table block, a progressive one's Huffman pool, the entropy-coded bytes; a raw image: its
    pixels), the rest is what its descriptor says."""
    kind: int
    h: int
    w: int
    pieces: Tuple[np.ndarray, ...]
    reason: Optional[str]
    blocks: int = 0
    ncomp: int = 3
    restart_interval: int = 0
    comp: Tuple = ((0, 0, 0, 0),) * 3            # per frame component: id, sampling, quant table, dc << 4 | ac table
    reserved: Tuple[int, int] = (0, 0)


def _coded_item(hd: JpegFrame, file: np.ndarray) -> _Item:
    if isinstance(hd, ProgressiveHeader):
        kind, tables = KIND_PROGRESSIVE, progressive_block(hd)
        payload = file[hd.scans[0].data_start:hd.scans[-1].data_end]
        sel = [0] * hd.ncomp
        reserved = (len(hd.scans) | (hd.rounds << 8) | ((len(tables[1]) // _HUFF_BYTES) << 16), SCAN_OFF)
    else:
        kind, tables = KIND_JPEG, (table_block(hd),)
        payload = file[hd.scan_offset:]
        sel = [(td << 4) | ta for td, ta in hd.scan_tables]
        reserved = (0, 0)
    comp = [(c[0], (c[1] << 4) | c[2], c[3], s) for c, s in zip(hd.comps, sel)] + [(0, 0, 0, 0)] * (3 - hd.ncomp)
    return _Item(kind, hd.h, hd.w, (*tables, payload), None, hd.blocks(), hd.ncomp, hd.restart_interval, tuple(comp),
                 reserved)


def pack_jpeg(items: Sequence, names: Optional[Sequence[str]] = None, progressive: bool = False) -> RaggedJpeg:
    """Compressed files (bytes-like) and already-decoded images (uint8 HWC [h, w, 3] arrays) -> one host RaggedJpeg,
    in order.  A file the device does not decode is decoded here with Pillow and packed raw; ``reasons[i]`` says why.
    With ``progressive=True`` a complete progressive (SOF2) file that ``parse_progressive`` accepts is packed for the
    device's progressive decoder (kind 2) instead of taking that fallback.
    Raises RuntimeError naming the item if it can be neither decoded on the device nor by Pillow."""
    n = len(items)
    if n < 1 or n > 65535:
        raise RuntimeError(f"pack_jpeg: expected 1 to 65535 items, got {n}")
    names = list(names) if names is not None else [f"item {i}" for i in range(n)]
    plan: List[_Item] = []
    for i, it in enumerate(items):
        if isinstance(it, torch.Tensor):
            it = it.numpy()
        reason = "already decoded"
        if isinstance(it, np.ndarray):
            if it.dtype != np.uint8 or it.ndim != 3 or it.shape[2] != 3 or not (
                    1 <= it.shape[0] <= MAX_SIDE and 1 <= it.shape[1] <= MAX_SIDE):
                raise RuntimeError(f"pack_jpeg: {names[i]} must be file bytes or uint8 HWC [h, w, 3] with sides in "
                                   f"[1, {MAX_SIDE}], got {it.dtype} {tuple(it.shape)}")
        elif not isinstance(it, (bytes, bytearray, memoryview)):
            raise RuntimeError(f"pack_jpeg: {names[i]} is a {type(it).__name__}, not file bytes or a uint8 array")
        else:
            hd = parse_header(it)
            if progressive and isinstance(hd, Unsupported) and hd.reason == _SOF_NAMES[0xC2]:
                hd = parse_progressive(it)
            if not isinstance(hd, Unsupported):
                plan.append(_coded_item(hd, np.frombuffer(bytes(it), dtype=np.uint8)))
                continue
            reason = hd.reason
            it = _pillow_decode(it, names[i], reason)
            if not (1 <= it.shape[0] <= MAX_SIDE and 1 <= it.shape[1] <= MAX_SIDE):
                raise RuntimeError(f"pack_jpeg: {names[i]} is {it.shape[1]}x{it.shape[0]}; sides must lie in [1, {MAX_SIDE}]")
        plan.append(_Item(KIND_RAW, it.shape[0], it.shape[1], (np.ascontiguousarray(it).reshape(-1),), reason))
    # layout: every item 16-byte aligned; a coded item's tables in front of its data
    size = out = blocks = 0
    rows = []                      # per item: where its pieces start, then the five offsets of its descriptor
    for it in plan:
        coded = it.kind != KIND_RAW
        head = sum(len(p) for p in it.pieces[:-1])
        rows.append((size, size + head, len(it.pieces[-1]), size if coded else 0, out, blocks if coded else 0))
        size = _align16(size + head + len(it.pieces[-1]))
        out += it.h * it.w * 3
        blocks += it.blocks
    starts, *offsets = zip(*rows)
    desc = np.zeros(n, dtype=JDESC_DTYPE)
    for name, column in zip(("data_offset", "data_bytes", "table_offset", "out_offset", "block_offset"), offsets):
        desc[name] = column
    for name in ("h", "w", "kind", "ncomp", "restart_interval", "comp", "reserved"):
        desc[name] = [getattr(it, name) for it in plan]
    data = torch.zeros(max(size, 16), dtype=torch.uint8)
    flat = data.numpy()
    for it, o in zip(plan, starts):
        for p in it.pieces:
            flat[o:o + len(p)] = p
            o += len(p)
    return RaggedJpeg(data, torch.from_numpy(desc.view(np.int64).reshape(n, _JDESC_WORDS)), blocks, out,
                      int(desc["h"].max()), int(desc["w"].max()), [it.reason for it in plan])


def collate_jpeg(batch, progressive: bool = False):
    """``DataLoader`` ``collate_fn`` for ``(file_bytes, target)`` samples (``FileBytesFolder``): returns
    ``(RaggedJpeg, targets)``, the targets collated as the default collate does."""
    files, targets = zip(*batch)
    return pack_jpeg(files, progressive=progressive), torch.utils.data.default_collate(list(targets))


def collate_jpeg_progressive(batch):
    """``collate_jpeg`` with the device's progressive decoder switched on: complete progressive files are shipped
    compressed (kind 2) instead of being decoded by Pillow in the worker."""
    return collate_jpeg(batch, progressive=True)


IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


class FileBytesFolder(torch.utils.data.Dataset):
    """``torchvision.datasets.ImageFolder``'s indexing (sorted class directories, their image files sorted, walked
    recursively) returning ``(file bytes, class index)``: the decode happens in ``collate_jpeg`` and on the device."""

    def __init__(self, root: str):
        self.root = root
        self.classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
        if not self.classes:
            raise FileNotFoundError(f"FileBytesFolder: no class directories in {root}")
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for base, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for f in sorted(files):
                    if f.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(base, f), self.class_to_idx[c]))
        self.targets = [t for _, t in self.samples]

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, i):
        path, target = self.samples[i]
        with open(path, "rb") as f:
            return f.read(), target


class FileBytesList(torch.utils.data.Dataset):
    """The unlabelled sibling of ``FileBytesFolder``: every image file under a directory (sorted, walked recursively --
    no class directories needed) or an explicit list of paths, kept in the order given.  Returns
    ``(file bytes, index)``, so ``collate_jpeg`` works on it unchanged and a batch knows which files it holds."""

    def __init__(self, root_or_paths):
        if isinstance(root_or_paths, (str, os.PathLike)):
            root = os.fspath(root_or_paths)
            if not os.path.isdir(root):
                raise FileNotFoundError(f"FileBytesList: {root} is not a directory")
            self.paths = []
            for base, dirs, files in os.walk(root, followlinks=True):
                dirs.sort()                               # (os.walk descends in this order)
                self.paths += [os.path.join(base, f) for f in files if f.lower().endswith(IMG_EXTENSIONS)]
            self.paths.sort()
            if not self.paths:
                raise FileNotFoundError(f"FileBytesList: no image files under {root}")
        else:
            self.paths = [os.fspath(p) for p in root_or_paths]
        self.samples = [(p, i) for i, p in enumerate(self.paths)]

    def __len__(self) -> int:
        return len(self.paths)

    def __getitem__(self, i):
        with open(self.paths[i], "rb") as f:
            return f.read(), i


# ----------------------------------------------------------------------------------------------------------------------
# device side

def _raise_corrupt(count: int):
    raise RuntimeError(f"decode_ragged: {count} image(s) of an earlier batch had corrupt entropy-coded data (truncated, "
                       "a bad Huffman code, a coefficient index past 63 or a missing restart marker): they were "
                       "decoded as all-zero images")


class _Ctx:
    def __init__(self, device: torch.device):
        self.device = device
        h = C.c_void_p()
        _lib.check(_lib.load().ttnet_jpeg_ctx_create(device.index, C.byref(h)))
        self.h = h
        self.res = (0, 0, 0)
        # int32 [2]: corrupt images, segments decoded sequentially (added to by the device)
        self.count = _StickyCount(device, 2, _raise_corrupt)
        self.stats = self.count.dev
        self.captured = False      # a graph captured a decode on this workspace: it must never be replaced

    def reserve(self, images: int, blocks: int, nbytes: int):
        if images <= self.res[0] and blocks <= self.res[1] and nbytes <= self.res[2]:
            return
        if images > MAX_IMAGES:
            raise RuntimeError(f"decode_ragged: {images} images in one batch; at most {MAX_IMAGES}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"decode_ragged: the batch ({images} images, {blocks} blocks, {nbytes} bytes) exceeds the "
                               f"decoder's reservation {self.res} while a graph is being captured; call "
                               "reserve_jpeg first")
        if self.captured:
            raise RuntimeError(f"decode_ragged: the batch ({images} images, {blocks} blocks, {nbytes} bytes) exceeds the "
                               f"reservation {self.res} of a lane whose workspace a captured graph decodes into; growing "
                               "it would free that workspace under the graph.  Use another lane, or reserve_jpeg enough "
                               "before capturing")
        grow = lambda need, have: max(need, have, int(need * 1.25) if have else need)   # noqa: E731
        res = (min(grow(images, self.res[0]), MAX_IMAGES), grow(blocks, self.res[1]), grow(nbytes, self.res[2]))
        _lib.check(_lib.load().ttnet_jpeg_ctx_reserve(self.h, res[0], res[1], res[2]))
        self.res = res


# one decoder context (workspace) per (device, lane): decodes on different lanes may be in flight together
_ctx: Dict[Tuple[torch.device, int], _Ctx] = {}
MAX_IMAGES = 65535          # ttnet_jpeg_ctx_reserve's bound


def _context(device: torch.device, lane: int = 0) -> _Ctx:
    key = (device, int(lane))
    if key not in _ctx:
        with torch.cuda.device(device):
            _ctx[key] = _Ctx(device)
    return _ctx[key]


def reserve_jpeg(device, max_images: int, max_blocks: int, max_bytes: int, lane: int = 0):
    """Size a lane's device decoder workspace ahead of time (e.g. before capturing a graph)."""
    device = torch.device(device)
    _context(device, lane).reserve(int(max_images), int(max_blocks), int(max_bytes))


def jpeg_counters(device=None, clear: bool = True) -> Tuple[int, int]:
    """Synchronise ``device`` and return (corrupt images, segments decoded by the sequential fallback) counted
    since the last clear."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    torch.cuda.synchronize(device)
    bad = seq = 0
    for (dev, _), c in _ctx.items():
        if dev == device:
            v = c.count.read(clear)
            bad, seq = bad + v[0], seq + v[1]
    return int(bad), int(seq)


def check_jpeg(device=None):
    """Synchronise ``device`` and raise if any decode on it met a corrupt image (then clear the count)."""
    bad, _ = jpeg_counters(device, clear=True)
    if bad:
        _raise_corrupt(bad)


def decode_ragged(rj: RaggedJpeg, lane: int = 0) -> RaggedU8:
    """A RaggedJpeg on a HIP device -> the decoded RGB images (a RaggedU8 on the device, in input order), with no host
    synchronisation (capturable in a graph once the workspace is reserved).  Each ``lane`` has its own workspace:
    batches in flight together on different streams use different lanes; a lane must not be reused before the
    decode issued on it has finished or been ordered before the new one by its stream.  The workspace grows with the
    batches, except on a lane that a captured graph decodes on: a larger batch there raises (use ``reserve_jpeg``
    before capturing, or another lane), since growing would free memory the graph still uses.  A corrupt image decodes as zeros and
    makes a later call raise (the device count is copied to the host after each call); ``check_jpeg`` checks at
    once."""
    if not isinstance(rj, RaggedJpeg):
        raise RuntimeError(f"expected a RaggedJpeg (pack_jpeg / collate_jpeg), got {type(rj).__name__}")
    if not rj.data.is_cuda:
        raise RuntimeError(f"the JPEG batch is on {rj.device}: move it with .to(device, non_blocking=True)")
    dev = rj.data.device
    ctx = _context(dev, lane)
    capturing = torch.cuda.is_current_stream_capturing()
    ctx.captured = ctx.captured or capturing
    ctx.count.raise_pending(capturing)
    n = len(rj)
    ctx.reserve(n, rj.n_blocks, rj.data.numel())
    data = rj.data if rj.data.data_ptr() % 16 == 0 else rj.data.clone()
    desc = rj.desc.contiguous()
    out = torch.empty(_align16(max(rj.out_bytes, 16)), dtype=torch.uint8, device=dev)
    odesc = torch.empty((n, 2), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().ttnet_jpeg_decode_ragged(
            ctx.h, C.c_void_p(data.data_ptr()), data.numel(), C.c_void_p(desc.data_ptr()), n, rj.n_blocks,
            C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(odesc.data_ptr()), C.c_void_p(ctx.stats.data_ptr()),
            C.c_void_p(stream)))
        ctx.count.mirror(capturing)
    return RaggedU8(out, odesc, rj.max_h, rj.max_w)


def jpeg_eval_forward(model, rj: RaggedJpeg, lane: int = 0) -> torch.Tensor:
    """``model(imgnet_transform(False)(Image.open(f).convert("RGB")))`` for a batch of files: decode ->
    resize_center_crop_u8_ragged -> forward_u8, all on the current stream, no host synchronisation."""
    return model.forward_u8(resize_center_crop_u8_ragged(decode_ragged(rj, lane=lane)), lane=lane)


def jpeg_views_forward(model, rj: RaggedJpeg, family: str, lane: int = 0) -> torch.Tensor:
    """``jpeg_eval_forward`` with several views per file (``preprocess.imgnet_views_forward``): every file is decoded
    ONCE, then the ``family`` of crops is cut from the decoded image on the device, all ``n * V`` crops are forwarded and
    each image's logits are averaged.  No host synchronisation."""
    return imgnet_views_forward(model, decode_ragged(rj, lane=lane), family, lane=lane)
