// Baseline / extended sequential and (kind 2) progressive Huffman JPEG decoding of a ragged batch on the GPU (ttnet_jpeg_decode_ragged):
// PIL.Image.open(f).convert("RGB") of ImageFolder's default loader (main.py:208), byte for byte as Pillow with
// libjpeg-turbo decodes it (islow IDCT, fancy upsampling, jdcolor.c's SCALEBITS 16 tables).
//
// Four kernels, all reading their image's descriptor and tables from the batch buffer (nothing per geometry is
// cached or uploaded; a captured graph replays with new images):
//   1. jpeg_destuff_kernel   one workgroup per image: drops FF 00 stuffing, splits at RSTn (sequence checked) and
//                            stops at any other marker, byte-parallel with workgroup prefix sums.  The clean stream is
//                            written at the image's own byte offset of a workspace as large as the reservation.
//   2. jpeg_entropy_kernel   one workgroup per image: Huffman decoding inside a segment in parallel with the
//                            self-synchronising subsequence method (Weissenberger & Schmidt, ICPP 2018).  Every
//                            segment is cut into subsequences of S bits; each is decoded from a guessed state (bit
//                            position, block of the MCU, zig-zag index) and the state where it crosses into its
//                            successor replaces the successor's guess, round after round, until no start state changes
//                            (a fixpoint: every start state is then the true one).  Segments still changing after
//                            kMaxRounds are walked sequentially (counted per segment).  A prefix sum of the blocks started per
//                            subsequence places the output; a last pass writes int16 coefficients in zig-zag order
//                            (every position of a block is written once, zero runs included); DC differences are
//                            resolved by a segmented prefix sum per component, reset at each restart.
//   2b. jpeg_progressive_kernel  one workgroup per progressive (SOF2, kind 2) image: zeroes the image's coefficients,
//                            then decodes its scans, up to four side by side (one per wave) in the rounds the host
//                            scheduled; each scan is walked sequentially with wave-uniform control flow, lane k holding
//                            coefficient k of the current block.  Sequential images leave at once, and the other way round.
//   3. jpeg_idct_kernel      workgroups over (image, tile of one MCU row x kTileMcus MCU columns): dequantise + islow
//                            IDCT into LDS planes (chroma with one context row / column around the tile), fancy
//                            upsampling, YCbCr -> RGB, dword stores.  Raw-passthrough images are copied here.
// A corrupt image (truncated, bad Huffman code, coefficient index past 63, missing or misnumbered RST) is written as
// zeros and counted; bounds come from the descriptor and the reservation, never from the bitstream.

#include <stdlib.h>

#include <algorithm>

#include "ttnet_common.h"

namespace ttnet {
namespace {

constexpr int kThreads = 256;
constexpr int kTableBytes = 2048, kHuffOff = 384, kHuffBytes = 272;
constexpr int kMaxRounds = 64;
constexpr int kTileMcus = 32;                   // MCU columns per IDCT tile
constexpr int kIdctGrid = 32;                   // workgroups per image of the IDCT kernel (they stride over its tiles)
constexpr int kMinSub = 2048, kSubs = 256;     // subsequence bits (at least) and count per large segment
constexpr int kLut = 9;                         // first-level Huffman lookup bits
constexpr int kMaxScans = TTNET_JPEG_MAX_SCANS; // scans of a progressive image
constexpr int kWaves = kThreads / 64;           // scans of a progressive image decoded side by side

enum : int { ST_OK = 0, ST_BAD_DESC = 1, ST_CORRUPT = 2 };

struct Workspace {
  int16_t *coef;          // [max_blocks][64]
  uint32_t *stream;       // destuffed bytes at each image's data_offset, (max_bytes + 16) bytes
  int64_t stream_words;
  int32_t *seg;           // per image at seg_base(): segment start bytes in the clean stream
  int32_t *seg_round;     // per segment: the last synchronisation round that changed one of its start states
  int2 *item;             // (start bit, segment)
  int2 *st;               // start state: (bit, k | c << 8)
  int2 *from;             // the start state an item's recorded result was decoded from
  int32_t *nb;            // blocks started per item, then their exclusive prefix
  int4 *info;             // per image: status, segments found, clean bytes, items
  int64_t max_images, max_blocks, max_bytes, entries;
};

struct DecodeArgs {
  const uint8_t *src;
  int64_t src_bytes;
  const ttnet_jpeg_desc *desc;
  uint8_t *dst;
  int64_t dst_bytes;
  ttnet_image_desc *dst_desc;
  int32_t *stats;
  Workspace ws;
  int sequential;
};

// per-image geometry from the descriptor
struct Geo {
  int h, w, ncomp, hs, vs, bpm, mcux, mcuy, ri, nseg;
  int64_t nblocks;
};

__host__ __device__ inline Geo geometry(const ttnet_jpeg_desc &d) {
  Geo g;
  g.h = d.h; g.w = d.w; g.ncomp = d.ncomp; g.ri = d.restart_interval;
  if (d.ncomp == 1) {
    g.hs = g.vs = 1; g.bpm = 1;
  } else {
    g.hs = d.comp[0][1] >> 4; g.vs = d.comp[0][1] & 15; g.bpm = g.hs * g.vs + 2;
  }
  g.mcux = (g.w + 8 * g.hs - 1) / (8 * g.hs);
  g.mcuy = (g.h + 8 * g.vs - 1) / (8 * g.vs);
  g.nblocks = (int64_t)g.mcux * g.mcuy * g.bpm;
  g.nseg = g.ri > 0 ? (int)(((int64_t)g.mcux * g.mcuy + g.ri - 1) / g.ri) : 1;
  return g;
}

// descriptor checks shared by the kernels: everything the kernels index is inside the buffers and the reservation
__device__ inline bool desc_ok(const DecodeArgs &a, const ttnet_jpeg_desc &d, int i) {
  if (d.h < 1 || d.w < 1 || d.h > 8192 || d.w > 8192) return false;
  const int64_t out = (int64_t)d.h * d.w * 3;
  if (d.out_offset < 0 || d.out_offset > a.dst_bytes - out) return false;
  if (d.data_offset < 0 || d.data_bytes < 0 || d.data_offset > a.src_bytes - d.data_bytes) return false;
  if (d.kind == 1) return d.data_bytes >= out;
  if (d.kind != 0 && d.kind != 2) return false;
  if (d.table_offset < 0 || d.table_offset > a.src_bytes - kTableBytes || (d.table_offset & 1)) return false;
  if (d.kind == 2) {       // scan list inside the table block, Huffman pool behind it, both inside the source buffer
    const int ns = d.reserved[0] & 255, nr = (d.reserved[0] >> 8) & 255, nt = (d.reserved[0] >> 16) & 255;
    if (ns < 1 || ns > kMaxScans || nr < 1 || nr > ns || (d.reserved[0] >> 24)) return false;
    if (d.reserved[1] < kHuffOff || d.reserved[1] > kTableBytes - ns * (int)sizeof(ttnet_jpeg_scan) || (d.reserved[1] & 3))
      return false;
    if ((d.table_offset & 3) || d.table_offset > a.src_bytes - kTableBytes - (int64_t)nt * kHuffBytes) return false;
  }
  if (d.ncomp == 3) {
    const int hs = d.comp[0][1] >> 4, vs = d.comp[0][1] & 15;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    if (d.comp[1][1] != 0x11 || d.comp[2][1] != 0x11) return false;
  } else if (d.ncomp != 1) {
    return false;
  }
  if (d.restart_interval < 0 || d.data_bytes >= (int64_t)1 << 28) return false;  // bit positions (8 * bytes) fit int32
  const Geo g = geometry(d);
  if (d.block_offset < 0 || d.block_offset > a.ws.max_blocks - g.nblocks) return false;
  if (d.kind == 0 && g.nseg > d.data_bytes / 2 + 1) return false;                 // cannot hold that many RSTs
  (void)i;
  return true;
}

// per-image table area of the workspace: [base, base + cap)
__device__ inline int64_t seg_base(const ttnet_jpeg_desc &d, int i) { return d.data_offset / 2 + 2 * (int64_t)i; }
__device__ inline int64_t seg_cap(const ttnet_jpeg_desc &d) { return d.data_bytes / 2 + 2; }

// inclusive prefix sum over the workgroup (kThreads), s: kThreads ints of LDS
__device__ inline int block_scan(int v, int *s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    const int x = t >= o ? s[t - o] : 0;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  const int r = s[t];
  __syncthreads();
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. de-stuff + segment

__global__ __launch_bounds__(kThreads) void jpeg_destuff_kernel(DecodeArgs a) {
  __shared__ int s_scan[kThreads];
  __shared__ int s_end, s_err;
  const int i = blockIdx.x, t = threadIdx.x;
  const ttnet_jpeg_desc d = a.desc[i];
  int4 *info = a.ws.info + i;
  if (d.kind != 0) return;
  if (!desc_ok(a, d, i)) {
    if (t == 0) *info = make_int4(ST_BAD_DESC, 0, 0, 0);
    return;
  }
  const Geo g = geometry(d);
  const uint8_t *s = a.src + d.data_offset;
  const int64_t len = d.data_bytes;
  uint8_t *out = (uint8_t *)a.ws.stream + d.data_offset;
  int32_t *seg = a.ws.seg + seg_base(d, i);
  if (t == 0) { s_end = (int)len; s_err = 0; seg[0] = 0; }
  __syncthreads();
  int outpos = 0, rsts = 0;
  // `lim`: the scan's end as known after the previous chunk's barrier (s_end itself may already be lowered by a faster
  // wave working on the next chunk, so the loop condition must not read it)
  int64_t lim = len;
  for (int64_t base = 0; base < lim; base += 4 * kThreads) {
    uint8_t b[4];
    int prv[4], nxt[4];
    int cand = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t p = base + 4 * t + u;
      b[u] = p < len ? s[p] : 0;
      prv[u] = (p > 0 && p <= len) ? s[p - 1] : 0;
      nxt[u] = p + 1 < len ? s[p + 1] : -1;
      if (p < len && prv[u] == 0xFF && b[u] != 0x00 && b[u] != 0xFF && !(b[u] >= 0xD0 && b[u] <= 0xD7))
        cand = min(cand, (int)(p - 1));           // any other marker ends the scan
    }
    if (cand != 0x7fffffff) atomicMin(&s_end, cand);
    __syncthreads();
    const int end = s_end;
    int keep = 0, rst = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t p = base + 4 * t + u;
      if (p >= end) continue;
      if (b[u] == 0xFF) keep += nxt[u] == 0x00;
      else if (prv[u] == 0xFF) rst += (b[u] >= 0xD0 && b[u] <= 0xD7);
      else ++keep;
    }
    const int inc = block_scan(keep | (rst << 16), s_scan);
    const int total = s_scan[kThreads - 1];
    __syncthreads();
    int o = outpos + ((inc - (keep | (rst << 16))) & 0xffff), r = rsts + ((inc - (keep | (rst << 16))) >> 16);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t p = base + 4 * t + u;
      if (p >= end) continue;
      if (b[u] == 0xFF) {
        if (nxt[u] == 0x00) out[o++] = 0xFF;
      } else if (prv[u] == 0xFF) {
        if (b[u] >= 0xD0 && b[u] <= 0xD7) {
          if (r + 1 < g.nseg && b[u] == 0xD0 + (r & 7)) seg[r + 1] = o;
          else s_err = 1;                       // one RST too many, or out of sequence
          ++r;
        }
      } else {
        out[o++] = b[u];
      }
    }
    outpos += total & 0xffff;
    rsts += total >> 16;
    lim = end;
    __syncthreads();
  }
  // zero padding behind the clean stream, inside the image's own span (the reader's words may reach past the end)
  for (int k = t; k < 4; k += kThreads)
    if (outpos + k < len) out[outpos + k] = 0;
  __syncthreads();
  if (t == 0) {
    const bool bad = s_err || rsts + 1 != g.nseg;
    *info = make_int4(bad ? ST_CORRUPT : ST_OK, rsts + 1, outpos, 0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2. entropy decoding

struct Huff {
  uint16_t lut[1 << kLut];      // (length << 8) | symbol, 0: longer than kLut bits
  int maxcode[18];              // largest code of each length, -1 if none
  int valoff[18];
  uint8_t vals[256];
};

struct Reader {
  const uint32_t *w;
  int64_t nwords;
  int64_t base_bit;             // bit of the image's first clean byte, from a word boundary
  int64_t word0;
  __device__ inline uint32_t peek(int pos) const {
    const int64_t ab = base_bit + pos;
    int64_t wi = word0 + (ab >> 5);
    const int sh = (int)(ab & 31);
    const int64_t w0i = min(max(wi, (int64_t)0), nwords - 1), w1i = min(max(wi + 1, (int64_t)0), nwords - 1);
    const uint64_t v = ((uint64_t)__builtin_bswap32(w[w0i]) << 32) | __builtin_bswap32(w[w1i]);
    return (uint32_t)((v << sh) >> 32);
  }
};

// decode one symbol at the top of `v`: returns (length << 8) | symbol, or 0 for a bad code
__device__ inline int huff_decode(const Huff &h, uint32_t v) {
  const int e = h.lut[v >> (32 - kLut)];
  if (e) return e;
  for (int l = kLut + 1; l <= 16; ++l) {
    const int code = (int)(v >> (32 - l));
    if (code <= h.maxcode[l]) return (l << 8) | h.vals[(code + h.valoff[l]) & 255];
  }
  return 0;
}

// fills `h` from a DHT-style table (counts[16], symbols[256]); h.lut must be zero.  Bounded whatever the counts hold.
__device__ inline void build_huff(Huff &h, const uint8_t *src) {
  int code = 0, kk = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = src[l - 1];
    h.valoff[l] = kk - code;
    h.maxcode[l] = cnt ? code + cnt - 1 : -1;
    for (int q = 0; q < cnt; ++q, ++code, ++kk) {
      if (l <= kLut) {
        const int lo = code << (kLut - l), hi = (code + 1) << (kLut - l);
        for (int x = lo; x < hi && x < (1 << kLut); ++x) h.lut[x] = (uint16_t)((l << 8) | src[16 + (kk & 255)]);
      }
    }
    code <<= 1;
  }
  for (int q = 0; q < 256; ++q) h.vals[q] = src[16 + q];
}

__device__ inline int extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }

struct DecodeResult {
  int pos, kc, nb;
  bool err;      // corrupt data (bad code, index past 63, a block index outside the image)
  bool out;      // stopped at the end of the segment's bits
};

// Decodes the symbols that start in [pos, end) from state kc (k | c << 8), never accepting bits at or past seg_end.
// WRITE: stores coefficients of blocks blk0 - 1 + (DCs seen), in zig-zag order, DC as the difference.
template <bool WRITE>
__device__ DecodeResult decode_run(const Reader &rd, const Huff *dc, const Huff *ac, const int *comp_of, int bpm, int pos,
                                   int kc, int end, int seg_end, int16_t *coef, int64_t blk0, int64_t nblk) {
  DecodeResult r{pos, kc, 0, false, false};
  int k = kc & 255, c = kc >> 8;
  int64_t cur = blk0 - 1;
  while (pos < end) {
    const uint32_t v = rd.peek(pos);
    const int cp = comp_of[c];
    const int e = huff_decode(k == 0 ? dc[cp] : ac[cp], v);
    if (!e) {
      if (seg_end - pos < 32) { r.out = true; break; }
      if (WRITE) { r.err = true; break; }
      ++pos;            // a guessed state decodes garbage until it synchronises: keep going, deterministically
      continue;
    }
    const int L = e >> 8, sym = e & 255;
    const int s = k == 0 ? sym : (sym & 15);
    if (pos + L + s > seg_end) { r.out = true; break; }
    const int bits = s ? (int)((v << L) >> (32 - s)) : 0;
    pos += L + s;
    if (k == 0) {
      ++cur;
      ++r.nb;
      if (WRITE) {
        if (cur < 0 || cur >= nblk) { r.err = true; break; }
        coef[cur * 64] = (int16_t)(s ? extend(bits, s) : 0);
      }
      k = 1;
    } else {
      const int run = sym >> 4;
      int kn;
      if (s) {
        kn = k + run;
        if (kn > 63) {
          if (WRITE) { r.err = true; break; }
          kn = 63;      // (guessed state only, as above)
        }
      } else {
        kn = run == 15 ? min(k + 16, 64) : 64;     // ZRL, or EOB
      }
      if (WRITE) {
        if (cur < 0 || cur >= nblk) { r.err = true; break; }
        int16_t *b = coef + cur * 64;
        for (int z = k; z < kn; ++z) b[z] = 0;
        if (s) b[kn] = (int16_t)extend(bits, s);
      }
      k = s ? kn + 1 : kn;
    }
    if (k >= 64) {
      k = 0;
      c = c + 1 == bpm ? 0 : c + 1;
    }
  }
  r.pos = pos;
  r.kc = k | (c << 8);
  return r;
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(DecodeArgs a) {
  __shared__ Huff s_h[6];
  __shared__ int s_scan[kThreads];
  __shared__ int s_comp_of[6];
  __shared__ int s_changed, s_err, s_nitems, s_carry, s_nseq;
  const int i = blockIdx.x, t = threadIdx.x;
  const ttnet_jpeg_desc d = a.desc[i];
  if (d.kind != 0) return;
  int4 *info = a.ws.info + i;
  const int4 inf = *info;
  if (inf.x != ST_OK) return;
  const Geo g = geometry(d);
  const int nseg = inf.y, clean = inf.z;
  const int64_t base = seg_base(d, i), cap = seg_cap(d);
  const int32_t *seg = a.ws.seg + base;
  int2 *item = a.ws.item + base;
  int2 *st = a.ws.st + base;
  int2 *from = a.ws.from + base;
  int32_t *nb = a.ws.nb + base;
  int32_t *seg_round = a.ws.seg_round + base;
  int16_t *coef = a.ws.coef + d.block_offset * 64;
  // Huffman tables: 0..2 DC of components 0..2, 3..5 AC
  const uint8_t *tb = a.src + d.table_offset;
  for (int e = t; e < 6 * (1 << kLut); e += kThreads) s_h[e >> kLut].lut[e & ((1 << kLut) - 1)] = 0;
  if (t < 6) s_comp_of[t] = t < g.bpm ? (g.ncomp == 1 ? 0 : (t < g.bpm - 2 ? 0 : t - (g.bpm - 3))) : 0;
  if (t == 0) { s_err = 0; s_carry = 0; }
  __syncthreads();
  if (t < 2 * g.ncomp) {
    const int comp = t >> 1, isac = t & 1;
    build_huff(s_h[isac * 3 + comp], tb + kHuffOff + (2 * comp + isac) * kHuffBytes);
  }
  // subsequence length: at least kMinSub bits, about kSubs subsequences for a large single-segment image.  Bit
  // synchronisation is quick, but the position in the MCU (c) only re-synchronises after some hundreds of symbols.
  const int S = max(kMinSub, (int)(((int64_t)clean * 8 / kSubs + 31) & ~31));
  // items: segment j covers clean bytes [seg[j], seg[j+1]), cut into ceil(bits / S) subsequences (at least one)
  auto seg_lo = [&](int j) { return seg[j] * 8; };
  auto seg_hi = [&](int j) { return (j + 1 < nseg ? seg[j + 1] : clean) * 8; };
  if (t == 0) s_nitems = 0;
  __syncthreads();
  for (int j0 = 0; j0 < nseg; j0 += kThreads) {
    const int j = j0 + t;
    int cnt = 0;
    if (j < nseg) cnt = max(1, (seg_hi(j) - seg_lo(j) + S - 1) / S);
    const int inc = block_scan(cnt, s_scan);
    const int tot = s_scan[kThreads - 1];
    const int first = s_nitems + inc - cnt;
    if (j < nseg) {
      seg_round[j] = -1;
      for (int q = 0; q < cnt; ++q) {
        const int it = first + q;
        if (it < cap) {
          const int sb = seg_lo(j) + q * S;
          item[it] = make_int2(sb, j);
          st[it] = make_int2(sb, 0);
          from[it] = make_int2(-1, -1);
        } else {
          s_err = 1;
        }
      }
    }
    __syncthreads();
    if (t == 0) s_nitems += tot;
    __syncthreads();
  }
  const int nitems = min((int64_t)s_nitems, cap);
  if (s_err) {
    if (t == 0) { *info = make_int4(ST_CORRUPT, nseg, clean, 0); }
    return;
  }
  const Reader rd{a.ws.stream, a.ws.stream_words, (d.data_offset & 3) * 8, d.data_offset >> 2};
  auto item_end = [&](int it, int j) {
    return (it + 1 < nitems && item[it + 1].y == j) ? item[it + 1].x : seg_hi(j);
  };
  const Huff *dc = s_h, *ac = s_h + 3;
  // synchronisation rounds
  bool settled = false;
  if (!a.sequential) {
    for (int round = 0; round < kMaxRounds; ++round) {
      if (t == 0) s_changed = 0;
      __syncthreads();                            // (the previous round's flag has been read by every wave)
      for (int it = t; it < nitems; it += kThreads) {
        const int2 s0 = st[it], f = from[it];
        if (s0.x == f.x && s0.y == f.y) continue;
        const int j = item[it].y;
        const DecodeResult r = decode_run<false>(rd, dc, ac, s_comp_of, g.bpm, s0.x, s0.y, item_end(it, j), seg_hi(j),
                                                 nullptr, 0, 0);
        from[it] = s0;
        nb[it] = r.nb;
        if (it + 1 < nitems && item[it + 1].y == j) {
          const int2 nx = st[it + 1];
          if (nx.x != r.pos || nx.y != r.kc) {
            st[it + 1] = make_int2(r.pos, r.kc);
            seg_round[j] = round;
            s_changed = 1;
          }
        }
      }
      __syncthreads();
      const int changed = s_changed;
      __syncthreads();                            // every wave has its copy before thread 0 clears the flag
      if (!changed) { settled = true; break; }
    }
  }
  if (!settled) {
    // Sequential walk (one thread per segment) of the segments still changing in the last round: a segment with no
    // change in a round is at its fixpoint (only an item writes its successor's start), every other one is walked.
    if (t == 0) s_nseq = 0;
    __syncthreads();
    for (int j = t; j < nseg; j += kThreads) {
      if (!a.sequential && seg_round[j] != kMaxRounds - 1) continue;
      atomicAdd(&s_nseq, 1);
      int it = 0;
      // first item of segment j: items are in segment order; find by scanning from an estimate
      int lo = 0, hi = nitems;
      while (lo < hi) { const int m = (lo + hi) >> 1; if (item[m].y < j) lo = m + 1; else hi = m; }
      it = lo;
      for (; it < nitems && item[it].y == j; ++it) {
        const int2 s0 = st[it];
        const DecodeResult r = decode_run<false>(rd, dc, ac, s_comp_of, g.bpm, s0.x, s0.y, item_end(it, j), seg_hi(j),
                                                 nullptr, 0, 0);
        from[it] = s0;
        nb[it] = r.nb;
        if (it + 1 < nitems && item[it + 1].y == j) st[it + 1] = make_int2(r.pos, r.kc);
      }
    }
    __syncthreads();
    if (t == 0 && a.stats && s_nseq) atomicAdd(a.stats + 1, s_nseq);
  }
  __syncthreads();
  // exclusive prefix of the blocks started per item, checked against each segment's expected start
  for (int i0 = 0; i0 < nitems; i0 += kThreads) {
    const int it = i0 + t;
    const int v = it < nitems ? nb[it] : 0;
    const int inc = block_scan(v, s_scan);
    const int tot = s_scan[kThreads - 1];
    if (it < nitems) {
      const int ex = s_carry + inc - v;
      nb[it] = ex;
      const int j = item[it].y;
      if ((it == 0 || item[it - 1].y != j) && (int64_t)ex != (int64_t)j * g.ri * g.bpm) s_err = 1;
    }
    __syncthreads();
    if (t == 0) s_carry += tot;
    __syncthreads();
  }
  if ((int64_t)s_carry != g.nblocks) s_err = 1;
  __syncthreads();
  // the final pass: coefficients
  if (!s_err) {
    for (int it = t; it < nitems; it += kThreads) {
      const int2 s0 = st[it];
      const int j = item[it].y;
      const bool last = !(it + 1 < nitems && item[it + 1].y == j);
      const DecodeResult r = decode_run<true>(rd, dc, ac, s_comp_of, g.bpm, s0.x, s0.y, item_end(it, j), seg_hi(j), coef,
                                              nb[it], g.nblocks);
      if (r.err || (r.out && !last) || (last && r.kc != 0)) s_err = 1;
    }
  }
  __syncthreads();
  // DC: segmented prefix sum per component over the MCUs in order (reset at each restart)
  if (!s_err) {
    __shared__ int s_v[3][kThreads];
    __shared__ int s_f[kThreads];
    __shared__ int s_dcc[3];
    if (t < 3) s_dcc[t] = 0;
    __syncthreads();
    const int64_t nmcu = (int64_t)g.mcux * g.mcuy;
    const int ny = g.bpm == 1 ? 1 : g.bpm - 2;
    for (int64_t m0 = 0; m0 < nmcu; m0 += kThreads) {
      const int64_t m = m0 + t;
      int v[3] = {0, 0, 0};
      int f = 0;
      if (m < nmcu) {
        const int16_t *b = coef + m * g.bpm * 64;
        for (int q = 0; q < ny; ++q) v[0] += b[q * 64];
        if (g.ncomp == 3) { v[1] = b[ny * 64]; v[2] = b[(ny + 1) * 64]; }
        f = (m == 0 || (g.ri > 0 && m % g.ri == 0)) ? 1 : 0;
      }
      // inclusive segmented scan of (f, v)
      s_f[t] = f;
      for (int c = 0; c < 3; ++c) s_v[c][t] = v[c];
      __syncthreads();
      for (int o = 1; o < kThreads; o <<= 1) {
        int pv[3] = {0, 0, 0}, pf = 0;
        if (t >= o) { pf = s_f[t - o]; for (int c = 0; c < 3; ++c) pv[c] = s_v[c][t - o]; }
        __syncthreads();
        if (t >= o && !s_f[t]) for (int c = 0; c < 3; ++c) s_v[c][t] += pv[c];
        if (t >= o) s_f[t] |= pf;
        __syncthreads();
      }
      // exclusive value + carry from the previous chunk unless a reset lies at or before this MCU in the chunk
      int pred[3];
      const int incf = s_f[t];
      for (int c = 0; c < 3; ++c) {
        const int ex = s_v[c][t] - v[c];                        // (for f == 1 the exclusive part is not used)
        pred[c] = f ? 0 : (incf ? ex : s_dcc[c] + ex);
      }
      if (m < nmcu) {
        int16_t *b = coef + m * g.bpm * 64;
        int p = pred[0];
        for (int q = 0; q < ny; ++q) { p += b[q * 64]; b[q * 64] = (int16_t)p; }
        if (g.ncomp == 3) {
          b[ny * 64] = (int16_t)(pred[1] + b[ny * 64]);
          b[(ny + 1) * 64] = (int16_t)(pred[2] + b[(ny + 1) * 64]);
        }
      }
      __syncthreads();
      if (t == kThreads - 1) for (int c = 0; c < 3; ++c) s_dcc[c] = s_f[t] ? s_v[c][t] : s_dcc[c] + s_v[c][t];
      __syncthreads();
    }
  }
  if (t == 0) {
    *info = make_int4(s_err ? ST_CORRUPT : ST_OK, nseg, clean, nitems);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2b. progressive (SOF2) entropy decoding
//
// One workgroup per kind-2 image, its scans spread over the workgroup's waves in rounds that the host scheduled so
// that a scan runs after every scan it refines (ttnet_jpeg_scan::slot = 4 * round + wave).  A wave walks its scan
// sequentially with wave-uniform control flow: the bit reader and the Huffman state are the same in every lane, and
// lane k holds coefficient k (zig-zag) of the current block, so that a block is loaded and stored with one coalesced
// access and the refinement walk tests "is coefficient k non-zero" in a ballot mask instead of a dependent load.

// Bits of one scan, un-stuffed on the fly.  Stops in front of any marker; bytes come from aligned 8-byte words.
struct ProgReader {
  const uint8_t *src;
  int64_t src_bytes;
  int64_t base;                 // scan's first byte in src; [base, base + n) is inside [0, src_bytes)
  int n, pos;
  uint64_t acc;                 // the next `cnt` bits at the top, zeros below
  int cnt;
  bool stop;                    // a marker or the end of the data lies at `pos`
  bool bad;                     // bits were asked for that the scan does not have, or a code without a symbol
  int64_t cw_idx;
  uint64_t cw;

  __device__ inline int byte_at(int p) {
    const int64_t a = base + p, wi = a >> 3;
    if (wi != cw_idx) {
      cw_idx = wi;
      if ((wi + 1) * 8 <= src_bytes) {
        cw = *(const uint64_t *)(src + wi * 8);
      } else {
        cw = 0;
        for (int q = 0; q < 8; ++q)
          if (wi * 8 + q < src_bytes) cw |= (uint64_t)src[wi * 8 + q] << (8 * q);
      }
    }
    return (int)((cw >> ((a & 7) * 8)) & 0xff);
  }
  __device__ inline void fill() {
    while (cnt <= 56 && !stop) {          // every turn advances pos or stops: at most n turns over the scan
      if (pos >= n) { stop = true; break; }
      const int b = byte_at(pos);
      if (b == 0xFF) {
        if (pos + 1 >= n) { stop = true; break; }
        const int b2 = byte_at(pos + 1);
        if (b2 == 0xFF) { ++pos; continue; }            // fill byte
        if (b2 != 0) { stop = true; break; }            // RSTn or another marker
        pos += 2;
      } else {
        ++pos;
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  __device__ inline int get(int nb) {                   // 0 <= nb <= 16
    if (nb == 0) return 0;
    if (cnt < nb) {
      fill();
      if (cnt < nb) { bad = true; return 0; }
    }
    const int v = (int)(acc >> (64 - nb));
    acc <<= nb;
    cnt -= nb;
    return v;
  }
  __device__ inline int decode(const Huff &h) {
    if (cnt < 16) fill();
    const int e = huff_decode(h, (uint32_t)(acc >> 32));
    const int L = e >> 8;
    if (!e || L > cnt) { bad = true; return 0; }
    acc <<= L;
    cnt -= L;
    return e & 255;
  }
  // the restart marker number `num` must be the next thing in the data (behind less than a byte of padding bits)
  __device__ inline bool restart(int num) {
    if (cnt >= 8) return false;
    acc = 0; cnt = 0; stop = false;
    if (pos >= n || byte_at(pos) != 0xFF) return false;
    while (pos < n && byte_at(pos) == 0xFF) ++pos;
    if (pos >= n || byte_at(pos) != 0xD0 + (num & 7)) return false;
    ++pos;
    return true;
  }
};

// Block geometry of one scan.  A scan of one component covers that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks
// in raster order (T.81 A.2.2) and its restart interval counts blocks; a scan of several covers the frame's MCUs.
struct ScanMap {
  int single;                   // one component
  int bw, hi, vi, base;         // single: blocks per row, the component's blocks per MCU (h, v), first block in the MCU
  int mcux, bpm, ny;
  int64_t units;                // blocks (single) or MCUs
  __device__ inline int64_t slot(int64_t u) const {     // single: the block's place in the MCU-ordered buffer
    const int by = (int)(u / bw), bx = (int)(u - (int64_t)by * bw);
    return ((int64_t)(by / vi) * mcux + bx / hi) * bpm + base + (by % vi) * hi + (bx % hi);
  }
};

__device__ inline ScanMap scan_map(const Geo &g, const ttnet_jpeg_scan &sc) {
  ScanMap m;
  m.mcux = g.mcux; m.bpm = g.bpm;
  m.ny = g.ncomp == 3 ? g.hs * g.vs : 1;
  m.single = sc.ncomp == 1;
  const int ci = sc.comp[0];
  const bool luma = ci == 0;
  m.hi = luma ? g.hs : 1;
  m.vi = luma ? g.vs : 1;
  m.base = luma ? 0 : m.ny + ci - 1;
  const int cw = luma ? g.w : (g.w + g.hs - 1) / g.hs, ch = luma ? g.h : (g.h + g.vs - 1) / g.vs;
  m.bw = (cw + 7) / 8;
  m.units = m.single ? (int64_t)m.bw * ((ch + 7) / 8) : (int64_t)g.mcux * g.mcuy;
  return m;
}

// everything a scan record lets the kernel index is inside the image's own buffers
__device__ inline bool scan_ok(const ttnet_jpeg_desc &d, const ttnet_jpeg_scan &sc, int ntables) {
  if (sc.ncomp < 1 || sc.ncomp > 3 || sc.ncomp > d.ncomp) return false;
  for (int q = 0; q < sc.ncomp; ++q) {
    if (sc.comp[q] >= d.ncomp || (q > 0 && sc.comp[q] <= sc.comp[q - 1])) return false;
    const bool uses_table = sc.ss > 0 ? q == 0 : sc.ah == 0;
    if (uses_table && sc.table[q] >= ntables) return false;
  }
  if ((int64_t)sc.data_offset + sc.data_bytes > d.data_bytes) return false;
  if (sc.al > 13 || sc.ah > 13 || sc.ss > sc.se || sc.se > 63) return false;
  if (sc.ss == 0 ? sc.se != 0 : sc.ncomp != 1) return false;
  return true;
}

// DC scans (first pass and refinement): 1 .. 3 components, interleaved over the MCUs when more than one.
__device__ bool prog_dc_scan(ProgReader &rd, const ttnet_jpeg_scan &sc, const ScanMap &m, const Huff *tab, int16_t *coef,
                             int64_t nblocks, int lane) {
  const int ri = sc.restart_interval, al = sc.al;
  const bool refine = sc.ah != 0;
  unsigned pred[3] = {0, 0, 0};
  int rst = 0, pend = 0;
  int64_t my_slot = 0;          // refinement: lane j keeps the j-th pending block's slot and bit until 64 are flushed
  int my_bit = 0;
  auto flush = [&]() {
    if (lane < pend && my_bit) coef[my_slot * 64] = (int16_t)(coef[my_slot * 64] | (1 << al));
    pend = 0;
  };
  for (int64_t u = 0; u < m.units; ++u) {
    if (ri > 0 && u > 0 && u % ri == 0) {
      if (!rd.restart(rst++)) return false;
      pred[0] = pred[1] = pred[2] = 0;
    }
    for (int q = 0; q < sc.ncomp; ++q) {
      const int ci = sc.comp[q];
      const int nb = m.single ? 1 : (ci == 0 ? m.ny : 1);
      const int64_t first = m.single ? m.slot(u) : u * m.bpm + (ci == 0 ? 0 : m.ny + ci - 1);
      for (int j = 0; j < nb; ++j) {
        const int64_t s = first + j;
        if (s < 0 || s >= nblocks) return false;
        if (refine) {
          const int bit = rd.get(1);
          if (lane == pend) { my_slot = s; my_bit = bit; }
          if (++pend == 64) flush();
        } else {
          const int sz = rd.decode(tab[q]);
          if (sz > 15) return false;
          const int bits = rd.get(sz);
          if (rd.bad) return false;
          pred[q] += (unsigned)(sz ? extend(bits, sz) : 0);
          if (lane == 0) coef[s * 64] = (int16_t)(pred[q] << al);
        }
      }
    }
    if (rd.bad) return false;
  }
  flush();
  return true;
}

// AC scans of one component: first pass of a band (every coefficient of the band still zero) and refinement
// (T.81 G.1.2.3, jdphuff.c decode_mcu_AC_refine).  c: this lane's coefficient of the current block.
__device__ bool prog_ac_scan(ProgReader &rd, const ttnet_jpeg_scan &sc, const ScanMap &m, const Huff &tab, int16_t *coef,
                             int64_t nblocks, int lane) {
  const int ri = sc.restart_interval, al = sc.al, ss = sc.ss, se = sc.se;
  const bool refine = sc.ah != 0, inband = lane >= ss && lane <= se;
  const int p1 = 1 << al, m1 = -(1 << al);
  int rst = 0;
  int64_t eobrun = 0;
  for (int64_t u = 0; u < m.units; ++u) {
    if (ri > 0 && u > 0 && u % ri == 0) {
      if (!rd.restart(rst++)) return false;
      eobrun = 0;
    }
    if (!refine && eobrun > 0) {          // a first pass leaves the blocks of an end-of-band run as they are: zero
      --eobrun;
      continue;
    }
    const int64_t s = m.slot(u);
    if (s < 0 || s >= nblocks) return false;
    int16_t *blk = coef + s * 64;
    int c = (refine && inband) ? blk[lane] : 0;
    const uint64_t nz = __ballot(c != 0);
    bool dirty = false;
    int k = ss;
    if (eobrun == 0) {
      for (; k <= se; ++k) {
        const int sym = rd.decode(tab);
        int r = sym >> 4;
        const int sz = sym & 15;
        if (rd.bad) return false;
        int val = 0;
        if (sz) {
          if (refine) {
            if (sz != 1) return false;
            val = rd.get(1) ? p1 : m1;
          } else {
            val = extend(rd.get(sz), sz) * (1 << al);
          }
        } else if (r != 15) {             // EOBr: this block and (1 << r) + extra - 1 more end here
          eobrun = ((int64_t)1 << r) + rd.get(r);
          if (eobrun > m.units - u) return false;
          break;
        }
        if (refine) {
          // skip r coefficients with a zero history; every non-zero one in the way takes a correction bit
          do {
            if ((nz >> k) & 1) {
              if (rd.get(1)) {
                if (lane == k && (c & p1) == 0) c += c >= 0 ? p1 : m1;
                dirty = true;
              }
            } else if (--r < 0) {
              break;
            }
            ++k;
          } while (k <= se);
        } else {
          k += r;
        }
        if (rd.bad) return false;
        if (sz) {
          if (k > se) return false;       // a coefficient index past the band
          if (lane == k) c = val;
          dirty = true;
        }
      }
    }
    if (eobrun > 0) {
      if (refine) {
        for (; k <= se; ++k) {
          if ((nz >> k) & 1) {
            if (rd.get(1)) {
              if (lane == k && (c & p1) == 0) c += c >= 0 ? p1 : m1;
              dirty = true;
            }
          }
        }
        if (rd.bad) return false;
      }
      --eobrun;
    }
    if (dirty && inband) blk[lane] = (int16_t)c;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void jpeg_progressive_kernel(DecodeArgs a) {
  __shared__ Huff s_h[kWaves][3];
  __shared__ ttnet_jpeg_scan s_scan[kMaxScans];
  __shared__ int s_err;
  const int i = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const ttnet_jpeg_desc d = a.desc[i];
  if (d.kind != 2) return;
  int4 *info = a.ws.info + i;
  if (!desc_ok(a, d, i)) {
    if (t == 0) *info = make_int4(ST_BAD_DESC, 0, 0, 0);
    return;
  }
  const Geo g = geometry(d);
  const int nscans = d.reserved[0] & 255, nrounds = (d.reserved[0] >> 8) & 255, ntables = (d.reserved[0] >> 16) & 255;
  const uint32_t *sl = (const uint32_t *)(a.src + d.table_offset + d.reserved[1]);
  for (int e = t; e < nscans * (int)(sizeof(ttnet_jpeg_scan) / 4); e += kThreads) ((uint32_t *)s_scan)[e] = sl[e];
  if (t == 0) s_err = 0;
  // every coefficient starts at zero: scans only write what they code
  int16_t *coef = a.ws.coef + d.block_offset * 64;
  uint4 *z = (uint4 *)coef;
  for (int64_t e = t; e < g.nblocks * 8; e += kThreads) z[e] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  const uint8_t *pool = a.src + d.table_offset + kTableBytes;
  for (int round = 0; round < nrounds; ++round) {
    int mine = -1;
    for (int j = 0; j < nscans; ++j)
      if (s_scan[j].slot == round * kWaves + wave) mine = j;
    const ttnet_jpeg_scan sc = s_scan[mine < 0 ? 0 : mine];
    const bool run = mine >= 0 && scan_ok(d, sc, ntables);
    const int ntab = !run ? 0 : (sc.ss > 0 ? 1 : (sc.ah == 0 ? sc.ncomp : 0));
    for (int e = lane; e < ntab * (1 << kLut); e += 64) s_h[wave][e >> kLut].lut[e & ((1 << kLut) - 1)] = 0;
    __syncthreads();                                // (every wave has read the last round's s_err)
    if (mine >= 0 && !run) s_err = 1;
    if (lane < ntab) build_huff(s_h[wave][lane], pool + (int)sc.table[lane] * kHuffBytes);
    __syncthreads();
    if (run && !s_err) {
      ProgReader rd{};
      rd.src = a.src; rd.src_bytes = a.src_bytes; rd.base = d.data_offset + sc.data_offset; rd.n = (int)sc.data_bytes;
      rd.cw_idx = -1;
      const ScanMap m = scan_map(g, sc);
      const bool ok = sc.ss == 0 ? prog_dc_scan(rd, sc, m, s_h[wave], coef, g.nblocks, lane)
                                 : prog_ac_scan(rd, sc, m, s_h[wave][0], coef, g.nblocks, lane);
      if (!ok) s_err = 1;
    }
    __syncthreads();                                // the round's coefficients are visible to the next round's waves
    if (s_err) break;
  }
  if (t == 0) *info = make_int4(s_err ? ST_CORRUPT : ST_OK, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// 3. dequantise + islow IDCT + fancy upsampling + YCbCr -> RGB

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jidctint.c's range_limit[(x) & RANGE_MASK] with the IDCT's CENTERJSAMPLE offset
__device__ inline int idct_range(int x) {
  const int m = x & 1023;
  return m < 128 ? m + 128 : (m < 512 ? 255 : (m < 896 ? 0 : m - 896));
}

// jpeg_idct_islow: in (natural order, dequantised) -> out rows of 8 bytes, row stride `pitch`
__device__ inline void idct_islow(const int *in, uint8_t *out, int pitch, int row_lo, int row_hi) {
  constexpr int CB = 13, P1 = 2;
  constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299,
                F1847 = 15137, F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
  int ws[64];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int *p = in + c;
    int z2 = p[16], z3 = p[48];
    int z1 = (z2 + z3) * F0541;
    int tmp2 = z1 + z3 * (-F1847);
    int tmp3 = z1 + z2 * F0765;
    z2 = p[0]; z3 = p[32];
    int tmp0 = (z2 + z3) * (1 << CB);
    int tmp1 = (z2 - z3) * (1 << CB);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = p[56]; tmp1 = p[40]; tmp2 = p[24]; tmp3 = p[8];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2; int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F1175;
    tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int sh = CB - P1, rnd = 1 << (sh - 1);
    ws[c + 0] = (tmp10 + tmp3 + rnd) >> sh;
    ws[c + 56] = (tmp10 - tmp3 + rnd) >> sh;
    ws[c + 8] = (tmp11 + tmp2 + rnd) >> sh;
    ws[c + 48] = (tmp11 - tmp2 + rnd) >> sh;
    ws[c + 16] = (tmp12 + tmp1 + rnd) >> sh;
    ws[c + 40] = (tmp12 - tmp1 + rnd) >> sh;
    ws[c + 24] = (tmp13 + tmp0 + rnd) >> sh;
    ws[c + 32] = (tmp13 - tmp0 + rnd) >> sh;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int *p = ws + 8 * r;
    int z2 = p[2], z3 = p[6];
    int z1 = (z2 + z3) * F0541;
    int tmp2 = z1 + z3 * (-F1847);
    int tmp3 = z1 + z2 * F0765;
    int tmp0 = (p[0] + p[4]) * (1 << CB);
    int tmp1 = (p[0] - p[4]) * (1 << CB);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = p[7]; tmp1 = p[5]; tmp2 = p[3]; tmp3 = p[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2; int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F1175;
    tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
    z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int sh = CB + P1 + 3, rnd = 1 << (sh - 1);
    if (r < row_lo || r >= row_hi) continue;
    uint8_t *o = out + (r - row_lo) * pitch;
    const uint32_t lo = (uint32_t)idct_range((tmp10 + tmp3 + rnd) >> sh) | ((uint32_t)idct_range((tmp11 + tmp2 + rnd) >> sh) << 8) |
                        ((uint32_t)idct_range((tmp12 + tmp1 + rnd) >> sh) << 16) |
                        ((uint32_t)idct_range((tmp13 + tmp0 + rnd) >> sh) << 24);
    const uint32_t hi = (uint32_t)idct_range((tmp13 - tmp0 + rnd) >> sh) | ((uint32_t)idct_range((tmp12 - tmp1 + rnd) >> sh) << 8) |
                        ((uint32_t)idct_range((tmp11 - tmp2 + rnd) >> sh) << 16) |
                        ((uint32_t)idct_range((tmp10 - tmp3 + rnd) >> sh) << 24);
    ((uint32_t *)o)[0] = lo;                     // (LDS rows are 4-byte aligned)
    ((uint32_t *)o)[1] = hi;
  }
}

// jdcolor.c build_ycc_rgb_table (SCALEBITS 16)
__device__ inline void ycc_rgb(int y, int cb, int cr, uint8_t *o) {
  constexpr int ONE_HALF = 1 << 15;
  const int xcb = cb - 128, xcr = cr - 128;
  const int crr = (91881 * xcr + ONE_HALF) >> 16;
  const int cbb = (116130 * xcb + ONE_HALF) >> 16;
  const int g = (-46802 * xcr + (-22554 * xcb + ONE_HALF)) >> 16;
  o[0] = (uint8_t)min(max(y + crr, 0), 255);
  o[1] = (uint8_t)min(max(y + g, 0), 255);
  o[2] = (uint8_t)min(max(y + cbb, 0), 255);
}

// LDS of the IDCT kernel
constexpr int kYRows = 16, kYCols = kTileMcus * 16;            // luma plane of a tile (2x2 sampling at most)
constexpr int kCRows = 10, kCCols = (kTileMcus + 2) * 8;       // chroma plane: one context row above / below, one block left / right
constexpr int kOutPitch = kTileMcus * 16 * 3;

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(DecodeArgs a) {
  __shared__ __align__(16) uint8_t s_y[kYRows * kYCols];
  __shared__ __align__(16) uint8_t s_c[2][kCRows * kCCols];
  __shared__ __align__(16) uint8_t s_o[kYRows * kOutPitch];
  __shared__ int s_q[3][64];
  const int i = blockIdx.x, t = threadIdx.x;
  const ttnet_jpeg_desc d = a.desc[i];
  const bool ok = desc_ok(a, d, i);
  if (blockIdx.y == 0 && t == 0) {
    ttnet_image_desc od;
    od.offset = ok ? d.out_offset : 0;
    od.h = ok ? d.h : 0;
    od.w = ok ? d.w : 0;
    a.dst_desc[i] = od;
  }
  if (!ok) {
    if (blockIdx.y == 0 && t == 0 && a.stats) atomicAdd(a.stats, 1);
    return;
  }
  const int64_t out_bytes = (int64_t)d.h * d.w * 3;
  uint8_t *dst = a.dst + d.out_offset;
  const int64_t gsz = (int64_t)gridDim.y * kThreads, gid = (int64_t)blockIdx.y * kThreads + t;
  if (d.kind == 1) {
    const uint8_t *s = a.src + d.data_offset;
    for (int64_t b = gid; b < out_bytes; b += gsz) dst[b] = s[b];
    return;
  }
  const int status = a.ws.info[i].x;
  if (status != ST_OK) {
    for (int64_t b = gid; b < out_bytes; b += gsz) dst[b] = 0;
    if (blockIdx.y == 0 && t == 0 && a.stats) atomicAdd(a.stats, 1);
    return;
  }
  const Geo g = geometry(d);
  const uint16_t *qsrc = (const uint16_t *)(a.src + d.table_offset);
  for (int e = t; e < 3 * 64; e += kThreads) s_q[e >> 6][e & 63] = qsrc[e];
  const int16_t *coef = a.ws.coef + d.block_offset * 64;
  const int tcols = (g.mcux + kTileMcus - 1) / kTileMcus, ntiles = tcols * g.mcuy;
  const int dw = (g.w + g.hs - 1) / g.hs, dh = (g.h + g.vs - 1) / g.vs;    // chroma size
  const int ny = g.ncomp == 3 ? g.hs * g.vs : 1;
  for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
    const int my = tile / tcols, mx0 = (tile % tcols) * kTileMcus, mx1 = min(mx0 + kTileMcus, g.mcux);
    const int nm = mx1 - mx0;
    // blocks: luma of the tile, then per chroma component the MCUs [mx0 - 1, mx1] x [my - 1, my + 1] that exist
    const int cxl = (g.ncomp == 3 && g.hs == 2 && mx0 > 0) ? mx0 - 1 : mx0;
    const int cxh = (g.ncomp == 3 && g.hs == 2 && mx1 < g.mcux) ? mx1 + 1 : mx1;
    const int cyl = (g.ncomp == 3 && g.vs == 2 && my > 0) ? my - 1 : my;
    const int cyh = (g.ncomp == 3 && g.vs == 2 && my + 1 < g.mcuy) ? my + 2 : my + 1;
    const int ncx = cxh - cxl, ncy = cyh - cyl;
    const int nyb = nm * ny, ncb = g.ncomp == 3 ? 2 * ncx * ncy : 0;
    __syncthreads();                              // the previous tile's LDS has been consumed
    for (int b = t; b < nyb + ncb; b += kThreads) {
      int64_t blk;
      int comp;
      uint8_t *o;
      int pitch, row_lo = 0, row_hi = 8;
      if (b < nyb) {
        const int m = b / ny, q = b - m * ny;
        blk = ((int64_t)my * g.mcux + mx0 + m) * g.bpm + q;
        comp = 0;
        const int bx = q % g.hs, by = q / g.hs;
        o = s_y + (by * 8) * kYCols + (m * g.hs + bx) * 8;
        pitch = kYCols;
      } else {
        const int e = b - nyb, cc = e / (ncx * ncy), r = e - cc * (ncx * ncy);
        const int cy = cyl + r / ncx, cx = cxl + r % ncx;
        blk = ((int64_t)cy * g.mcux + cx) * g.bpm + ny + cc;
        comp = 1 + cc;
        // plane row 1 + 8 * (cy - my) + row; keep rows 0 .. 9
        const int prow = 1 + 8 * (cy - my);
        row_lo = max(0, -prow);
        row_hi = min(8, kCRows - prow);
        o = s_c[cc] + (prow + row_lo) * kCCols + (cx - mx0 + 1) * 8;
        pitch = kCCols;
      }
      const uint4 *cp = (const uint4 *)(coef + blk * 64);
      int nat[64];
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const uint4 w = cp[v];
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int h2 = 0; h2 < 4; ++h2) {
          const int z0 = 8 * v + 2 * h2;
          nat[kZigzag[z0]] = (int)(int16_t)(ww[h2] & 0xffffu) * s_q[comp][z0];
          nat[kZigzag[z0 + 1]] = (int)(int16_t)(ww[h2] >> 16) * s_q[comp][z0 + 1];
        }
      }
      idct_islow(nat, o, pitch, row_lo, row_hi);
    }
    __syncthreads();
    // pixels of the tile -> RGB in s_o
    const int y0 = my * 8 * g.vs, x0 = mx0 * 8 * g.hs;
    const int rows = min(8 * g.vs, g.h - y0), cols = min(nm * 8 * g.hs, g.w - x0);
    for (int e = t; e < rows * cols; e += kThreads) {
      const int ry = e / cols, rx = e - ry * cols;
      const int Y = s_y[ry * kYCols + rx];
      uint8_t *o = s_o + ry * kOutPitch + rx * 3;
      if (g.ncomp == 1) { o[0] = o[1] = o[2] = (uint8_t)Y; continue; }
      int cv[2];
      const int x = x0 + rx, y = y0 + ry;
      const int ccol = (g.hs == 2 ? x >> 1 : x), crow = (g.vs == 2 ? y >> 1 : y);
      const int pc = ccol - (mx0 * 8 - 8);                   // plane column
      for (int cc = 0; cc < 2; ++cc) {
        const uint8_t *P = s_c[cc];
        auto at = [&](int row, int col) { return (int)P[(row - (my * 8 - 1)) * kCCols + col]; };
        if (g.hs == 1 || dw <= 2) {      // 4:4:4, or jdsample.c's plain replication below a chroma width of 3
          cv[cc] = at(crow, pc);
        } else if (g.vs == 1) {                                // h2v1_fancy_upsample
          const int v0 = at(crow, pc);
          if (!(x & 1)) cv[cc] = ccol == 0 ? v0 : (v0 * 3 + at(crow, pc - 1) + 1) >> 2;
          else cv[cc] = (ccol == dw - 1 && dw > 1) ? v0 : (v0 * 3 + at(crow, pc + 1) + 2) >> 2;
        } else {                                               // h2v2_fancy_upsample
          const int far = (y & 1) ? min(crow + 1, dh - 1) : max(crow - 1, 0);
          auto colsum = [&](int col) { return at(crow, col) * 3 + at(far, col); };
          const int c0 = colsum(pc);
          if (!(x & 1)) cv[cc] = ccol == 0 ? (c0 * 4 + 8) >> 4 : (c0 * 3 + colsum(pc - 1) + 8) >> 4;
          else cv[cc] = (ccol == dw - 1 && dw > 1) ? (c0 * 4 + 7) >> 4 : (c0 * 3 + colsum(pc + 1) + 7) >> 4;
        }
      }
      ycc_rgb(Y, cv[0], cv[1], o);
    }
    __syncthreads();
    // store: per row, bytes [x0 * 3, (x0 + cols) * 3) of the image row; dwords where aligned, bytes at the ends
    const int rb = cols * 3;
    for (int ry = 0; ry < rows; ++ry) {
      const int64_t g0 = ((int64_t)(y0 + ry) * g.w + x0) * 3;
      uint8_t *gp = dst + g0;
      const uint8_t *lp = s_o + ry * kOutPitch;
      const int head = min(rb, (int)((4 - (((uintptr_t)gp) & 3)) & 3));
      const int nq = (rb - head) >> 2;
      for (int e = t; e < nq; e += kThreads) {
        const uint8_t *l = lp + head + 4 * e;
        ((uint32_t *)(gp + head))[e] = (uint32_t)l[0] | ((uint32_t)l[1] << 8) | ((uint32_t)l[2] << 16) | ((uint32_t)l[3] << 24);
      }
      const int tail0 = head + 4 * nq;
      if (t < head) gp[t] = lp[t];
      else if (t >= 4 && t - 4 < rb - tail0) gp[tail0 + t - 4] = lp[tail0 + t - 4];
    }
  }
}

}  // namespace
}  // namespace ttnet

using namespace ttnet;

struct ttnet_jpeg_ctx {
  int device = 0;
  Workspace ws{};
  void *mem = nullptr;
};

extern "C" int ttnet_jpeg_ctx_create(int device, ttnet_jpeg_ctx **out) {
  if (!out) { set_error("jpeg_ctx_create: out is NULL"); return TTNET_E_INVALID; }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
    set_error("jpeg_ctx_create: no HIP device %d", device);
    return TTNET_E_INVALID;
  }
  ttnet_jpeg_ctx *c = new ttnet_jpeg_ctx();
  c->device = device;
  *out = c;
  return TTNET_OK;
}

extern "C" int ttnet_jpeg_ctx_reserve(ttnet_jpeg_ctx *c, int64_t max_images, int64_t max_blocks, int64_t max_bytes) {
  if (!c || max_images < 1 || max_images > 65535 || max_blocks < 0 || max_bytes < 16 || max_blocks > ((int64_t)1 << 34) ||
      max_bytes > ((int64_t)1 << 36)) {
    set_error("jpeg_ctx_reserve: bad argument (images %lld, blocks %lld, bytes %lld)", (long long)max_images,
              (long long)max_blocks, (long long)max_bytes);
    return TTNET_E_INVALID;
  }
  TT_HIP(hipSetDevice(c->device));
  Workspace w{};
  w.max_images = max_images; w.max_blocks = max_blocks; w.max_bytes = max_bytes;
  w.entries = max_bytes / 2 + 2 * max_images + 2;
  w.stream_words = (max_bytes + 16 + 3) / 4;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t sz_coef = al((size_t)max_blocks * 128 + 16), sz_stream = al((size_t)w.stream_words * 4),
               sz_seg = al((size_t)w.entries * 4), sz_i2 = al((size_t)w.entries * 8), sz_info = al((size_t)max_images * 16);
  const size_t total = sz_coef + sz_stream + 3 * sz_seg + 3 * sz_i2 + sz_info;
  void *mem = nullptr;
  TT_HIP(hipMalloc(&mem, total));
  if (c->mem) TT_HIP(hipFree(c->mem));
  c->mem = mem;
  uint8_t *p = (uint8_t *)mem;
  w.coef = (int16_t *)p; p += sz_coef;
  w.stream = (uint32_t *)p; p += sz_stream;
  w.seg = (int32_t *)p; p += sz_seg;
  w.seg_round = (int32_t *)p; p += sz_seg;
  w.item = (int2 *)p; p += sz_i2;
  w.st = (int2 *)p; p += sz_i2;
  w.from = (int2 *)p; p += sz_i2;
  w.nb = (int32_t *)p; p += sz_seg;
  w.info = (int4 *)p;
  TT_HIP(hipMemset(w.stream, 0, sz_stream));
  c->ws = w;
  return TTNET_OK;
}

extern "C" int ttnet_jpeg_decode_ragged(ttnet_jpeg_ctx *c, const uint8_t *src_dev, int64_t src_bytes,
                                        const ttnet_jpeg_desc *jdesc_dev, int64_t n, int64_t n_blocks, uint8_t *dst_dev,
                                        int64_t dst_bytes, ttnet_image_desc *dst_desc_dev, int32_t *stats_dev,
                                        void *stream) {
  if (!c || !src_dev || !jdesc_dev || !dst_dev || !dst_desc_dev || n < 1 || src_bytes < 1 || dst_bytes < 1 ||
      n_blocks < 0) {
    set_error("jpeg_decode_ragged: bad argument (n %lld, src_bytes %lld, dst_bytes %lld, blocks %lld)", (long long)n,
              (long long)src_bytes, (long long)dst_bytes, (long long)n_blocks);
    return TTNET_E_INVALID;
  }
  if (((uintptr_t)src_dev & 15) || ((uintptr_t)jdesc_dev & 15) || ((uintptr_t)dst_desc_dev & 7)) {
    set_error("jpeg_decode_ragged: src and descriptors must be 16-byte aligned, the output descriptors 8-byte aligned");
    return TTNET_E_INVALID;
  }
  if (!c->mem || n > c->ws.max_images || n_blocks > c->ws.max_blocks || src_bytes > c->ws.max_bytes) {
    set_error("jpeg_decode_ragged: the batch (%lld images, %lld blocks, %lld bytes) exceeds the reservation (%lld, %lld, "
              "%lld): call ttnet_jpeg_ctx_reserve first", (long long)n, (long long)n_blocks, (long long)src_bytes,
              (long long)c->ws.max_images, (long long)c->ws.max_blocks, (long long)c->ws.max_bytes);
    return TTNET_E_INVALID;
  }
  DecodeArgs a{};
  a.src = src_dev; a.src_bytes = src_bytes; a.desc = jdesc_dev; a.dst = dst_dev; a.dst_bytes = dst_bytes;
  a.dst_desc = dst_desc_dev; a.stats = stats_dev; a.ws = c->ws;
  const char *seq = getenv("TTNET_JPEG_SEQUENTIAL");
  a.sequential = seq && seq[0] == '1';
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_destuff_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_progressive_kernel, dim3((unsigned)n), dim3(kThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)n, kIdctGrid), dim3(kThreads), 0, s, a);
  TT_HIP(hipGetLastError());
  return TTNET_OK;
}

extern "C" void ttnet_jpeg_ctx_destroy(ttnet_jpeg_ctx *c) {
  if (!c) return;
  if (c->mem) {
    (void)hipSetDevice(c->device);
    (void)hipFree(c->mem);
  }
  delete c;
}
