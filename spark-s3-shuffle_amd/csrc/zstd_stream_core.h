// zstd_stream_core.h — resumable Zstandard: the unit walk and the block-by-block frame decoder of the streaming reduce side
// (s3s_dstream_open_zstd), written once for the device (zstd_decode_stream.hip) and for the host
// (tests/model/zstd_stream_model.cpp).
//
// decode_frame (zstd_decode_core.h) runs a frame from its header to its last block with everything a later block may reuse
// in its locals.  Here that state is a record (ZStreamState) that outlives the call: run_piece starts from a fresh frame or
// from the record, runs the blocks the unit table names, and writes the record back when the frame is still open at the end.
// It is a sibling of decode_frame, built from the same primitives (read_ncount / build_fse / default_norm, read_huf_table /
// block_literals, the bit readers, put_*) and the same per-sequence arithmetic; decode_frame itself and every kernel built
// from it stay what they were.
#pragma once
#include "zstd_decode_core.h"

namespace s3s_zstd {

// ---- units ----------------------------------------------------------------------------------------------------------------------
// A frame header (6..18 bytes, no output), a block (3-byte header + payload; an RLE block's payload is 1 byte), a skippable
// frame (8 + n bytes, no output).  kind = one of the values below, | ZU_LAST on a frame's last block.
enum { ZU_FRAME = 0, ZU_SKIP = 1, ZU_RAW = 2, ZU_RLE = 3, ZU_COMP = 4, ZU_LAST = 0x10 };
struct ZUnit {
  int64_t off;         // where the unit starts in the window
  int32_t kind;
  int32_t payload;     // ZU_FRAME: header bytes; ZU_SKIP: 8 + n; blocks: Block_Size
  int32_t frame_unit;  // blocks: the index of their frame's ZU_FRAME unit, -1 = the frame that was open when the window started
  int32_t pad;
};
constexpr int64_t kSkipMax = (int64_t)32 << 20;  // a skippable frame above this is refused, not walked

// One piece [beg, end) of a partition that ends at pend >= end (pend > end: the window ends first).  open: a frame is open at
// beg.  A unit is read only when it lies in front of `end`; one that does not fit in front of pend is corrupt (-1), one that
// fits there but not in front of `end` ends the walk: *stop = where it starts, *need = its length as far as the piece shows
// it (a frame header: 6, then the header's length; a skippable frame: 6, 8, then 8 + n; a block: 3, then 3 + payload).
// Returns the units in front of *stop, -1 (S3S_E_BAD_FRAME) or -2 (S3S_E_UNSUPPORTED: a content checksum, a Dictionary_ID
// field, a Window_Size above wmax, a skippable frame above kSkipMax).  emit: units[0, n) and dsize[0, n) are written
// (dsize: the decoded size where the header states it, 0 for a compressed block - the size pass fills it in).
ZS_HD int walk_piece(const uint8_t* comp, int64_t beg, int64_t end, int64_t pend, bool open, int64_t wmax, bool emit, ZUnit* units,
                     uint32_t* dsize, int32_t unit_base, int64_t* stop, int64_t* need) {
  int64_t ip = beg;
  int n = 0;
  int32_t fu = -1;
  *need = 0;
  // 0: x more bytes are there; 1: the window ends first (*need set); -1: the partition ends first
  auto want = [&](int64_t x) -> int {
    if (x > pend - ip) return -1;
    if (x > end - ip) {
      *need = x;
      return 1;
    }
    return 0;
  };
  while (ip < end) {
    int r;
    ZUnit u;
    u.off = ip;
    u.pad = 0;
    uint32_t out = 0;
    if (!open) {
      if ((r = want(6)) != 0) { if (r < 0) return -1; break; }
      const uint32_t magic = rd_le(comp + ip, 4);
      if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
        if ((r = want(8)) != 0) { if (r < 0) return -1; break; }
        const int64_t sk = 8 + (int64_t)rd_le(comp + ip + 4, 4);
        if (sk > kSkipMax) return -2;
        if ((r = want(sk)) != 0) { if (r < 0) return -1; break; }
        u.kind = ZU_SKIP;
        u.payload = (int32_t)sk;
        u.frame_unit = -2;
      } else {
        if (magic != 0xFD2FB528u) return -1;
        const uint32_t fhd = comp[ip + 4];
        if (fhd & 0x08) return -1;  // reserved bit
        const int fcs_flag = (int)(fhd >> 6), single = (int)((fhd >> 5) & 1), did_flag = (int)(fhd & 3);
        const int hlen = 5 + (single ? 0 : 1) + (did_flag == 3 ? 4 : did_flag) +
                         (fcs_flag == 0 ? (single ? 1 : 0) : (fcs_flag == 1 ? 2 : (fcs_flag == 2 ? 4 : 8)));
        if ((r = want(hlen)) != 0) { if (r < 0) return -1; break; }
        if ((fhd & 0x04) || did_flag) return -2;  // Content_Checksum / Dictionary_ID: outside the streaming contract
        FrameHdr fh;
        if (frame_header(comp + ip, hlen, &fh) != ZS_OK) return -1;
        if (fh.window > wmax || fh.window < 0) return -2;
        u.kind = ZU_FRAME;
        u.payload = hlen;
        u.frame_unit = unit_base + n;
        fu = unit_base + n;
        open = true;
      }
    } else {
      if ((r = want(3)) != 0) { if (r < 0) return -1; break; }
      const uint32_t bh = rd_le(comp + ip, 3);
      const int last = (int)(bh & 1), type = (int)((bh >> 1) & 3);
      const int64_t bsize = bh >> 3;
      if (type == 3 || bsize > kMaxBlock || (type == 2 && bsize < 2)) return -1;
      if ((r = want(3 + (type == 1 ? 1 : bsize))) != 0) { if (r < 0) return -1; break; }
      u.kind = (ZU_RAW + type) | (last ? ZU_LAST : 0);
      u.payload = (int32_t)bsize;
      u.frame_unit = fu;
      out = type < 2 ? (uint32_t)bsize : 0u;
      if (last) open = false;
    }
    if (emit) {
      units[n] = u;
      dsize[n] = out;
    }
    n++;
    ip += (u.kind & 15) == ZU_FRAME || (u.kind & 15) == ZU_SKIP ? u.payload : 3 + ((u.kind & 15) == ZU_RLE ? 1 : u.payload);
  }
  if (ip == pend && open) return -1;  // the partition ends with a frame open
  *stop = ip;
  return n;
}

// ---- the state a stream keeps for its open frame (device memory between feeds; the history bytes lie behind it) ------------
struct ZStreamState {
  HufWork h;                           // the Huffman tree a treeless literals section reuses (have_huf says whether there is one)
  uint32_t ll[1 << kLLLogMax];         // the LL / ML / OF tables a Repeat_Mode block reuses
  uint32_t ml[1 << kMLLogMax];
  uint32_t of[1 << kOFLogMax];
  int32_t ll_log, ml_log, of_log;
  int32_t have_ll, have_ml, have_of;
  uint32_t rep0, rep1, rep2;           // the three repeat offsets
  int32_t pad;
  int64_t produced;                    // bytes of the frame decoded so far (Frame_Content_Size check, window reach)
  int64_t window, fcs;                 // from the frame's header: Window_Size, Frame_Content_Size (-1: none)
};

// One compressed block b[0, bsize): decode_frame's block body with the repeat offsets handed in and out.  obase + bop is where
// the block's output starts, obase[0, bop) the bytes of the frame that are there to be matched (the saved history and what this
// feed decoded); total0 = bytes of the frame in front of the block, so that an offset may reach back min(window, total0 + what
// the block has produced) bytes and no further.  execute: bcap = the size the size pass measured (the block must not pass it).
ZS_HD int stream_block(Work& w, HufWork& h, const uint8_t* b, int64_t bsize, uint8_t* obase, int64_t bop, int64_t total0, int64_t window,
                       bool execute, uint32_t bcap, uint8_t* lit_buf, uint32_t& rep0, uint32_t& rep1, uint32_t& rep2, Lanes L,
                       uint32_t* produced) {
  const uint8_t* const bend = b + bsize;
  LitHdr lh;
  {
    const int rc = literals_header(b, bsize, &lh);
    if (rc != ZS_OK) return rc;
  }
  const int64_t regen = lh.regen;
  const uint8_t* lit = nullptr;
  int lit_rle = -1;
  if (lh.ltype == 0) {
    lit = b + lh.lh;
    b += lh.lh + regen;
  } else if (lh.ltype == 1) {
    lit_rle = b[lh.lh];
    b += lh.lh + 1;
  } else {
    if (execute) {
      const int rc = block_literals(h, lh, b + lh.lh, lh.lcomp, lit_buf, L);
      if (rc != ZS_OK) return rc;
      ZS_FENCE();  // (lanes 0..3 wrote the literals, every lane reads them)
    }
    lit = lit_buf;
    b += lh.lh + lh.lcomp;
  }
  if (b >= bend) return ZS_FAIL();
  int64_t nseq = b[0];
  if (nseq < 128) {
    b += 1;
  } else if (nseq < 255) {
    if (b + 2 > bend) return ZS_FAIL();
    nseq = ((nseq - 128) << 8) + b[1];
    b += 2;
  } else {
    if (b + 3 > bend) return ZS_FAIL();
    nseq = (int64_t)b[1] + ((int64_t)b[2] << 8) + 0x7F00;
    b += 3;
  }
  uint8_t* const bdst = obase + bop;
  const uint32_t rq0 = (uint32_t)bop;
  const uint32_t regen32 = (uint32_t)regen;
  uint32_t bout = 0, lit_pos = 0, visible = 0;
  int32_t litw_base = -1;
  if (nseq > 0) {
    if (b >= bend) return ZS_FAIL();
    const int modes = b[0];
    b += 1;
    if (modes & 3) return ZS_FAIL();
    for (int t = 0; t < 3; t++) {  // LL, OF, ML
      const int mode = (modes >> (6 - 2 * t)) & 3;
      uint32_t* tab = t == 0 ? w.ll : t == 1 ? w.of : w.ml;
      int32_t& tlog = t == 0 ? w.ll_log : t == 1 ? w.of_log : w.ml_log;
      int32_t& have = t == 0 ? w.have_ll : t == 1 ? w.have_of : w.have_ml;
      const int max_sym = t == 0 ? 35 : t == 1 ? 31 : 52, max_log = t == 0 ? kLLLogMax : t == 1 ? kOFLogMax : kMLLogMax;
      if (mode == 0) {
        int log;
        const int ms = default_norm(t, w.norm, &log);
        if (build_fse(tab, w.norm, ms, log, w.next) != ZS_OK) return ZS_FAIL();
        tlog = log;
        have = 1;
      } else if (mode == 1) {
        if (b >= bend) return ZS_FAIL();
        if (b[0] > max_sym) return ZS_FAIL();
        build_rle(tab, b[0]);
        tlog = 0;
        have = 1;
        b += 1;
      } else if (mode == 2) {
        int ms, log;
        const int used = read_ncount(w.norm, max_sym, max_log, b, bend - b, &ms, &log);
        if (used < 0) return used;
        if (build_fse(tab, w.norm, ms, log, w.next) != ZS_OK) return ZS_FAIL();
        tlog = log;
        have = 1;
        b += used;
      } else if (!have) {
        return ZS_FAIL();
      }
    }
    if (modes >> 6 != 3 || !w.vals_ll)  // (a repeated table keeps its values)
      for (int u = L.lane; u < (1 << w.ll_log); u += L.n) {
        const int c = (int)(w.ll[u] >> 24);
        w.llv[u] = ll_base(c) | ((uint32_t)ll_bits(c) << 24);
      }
    if (((modes >> 2) & 3) != 3 || !w.vals_ml)
      for (int u = L.lane; u < (1 << w.ml_log); u += L.n) {
        const int c = (int)(w.ml[u] >> 24);
        w.mlv[u] = ml_base(c) | ((uint32_t)ml_bits(c) << 24);
      }
    w.vals_ll = w.vals_ml = 1;
    ZS_FENCE();  // (lane-strided LDS fills above, read by every lane below: one wavefront, no barrier needed)
    BitR r;
    if (!bitr_init(r, b, bend - b)) return ZS_FAIL();
    uint32_t sl = bitr_read(r, w.ll_log), so = bitr_read(r, w.of_log), sm = bitr_read(r, w.ml_log);
    if (r.pos < 0) return ZS_FAIL();
    // how far back an offset may reach: the frame's window, and never further than the frame has produced
    const uint64_t wnd = (uint64_t)window;
    for (int64_t i = 0; i < nseq; i++) {
      const uint32_t el = ZS_UNI32(w.ll[sl]), eo = ZS_UNI32(w.of[so]), em = ZS_UNI32(w.ml[sm]);
      const uint32_t vl = ZS_UNI32(w.llv[sl]), vm = ZS_UNI32(w.mlv[sm]);
      const int co = (int)(eo >> 24);
      if (co > 31) return ZS_FAIL();
      uint32_t ov, mlen, llen;
      const int bm = (int)(vm >> 24), bl = (int)(vl >> 24);
      const bool more = i + 1 < nseq;
      const int nl = more ? (int)((el >> 16) & 0xff) : 0, nm = more ? (int)((em >> 16) & 0xff) : 0, no = more ? (int)((eo >> 16) & 0xff) : 0;
      const int nb = co + bm + bl + nl + nm + no;
      if (nb <= 57) {  // all fields of the sequence from one window of the stream
        if (!(r.pos - nb >= r.cbase && r.pos <= r.cbase + 64)) {
          const int32_t top = (r.pos - 1) >> 3;
          r.cbase = (top - 7) * 8;
          r.cache = load_bits64(r.p, r.size, top - 7);
#ifdef S3S_ZSTD_DEVICE
          r.cache = (uint64_t)ZS_UNI32((uint32_t)r.cache) | ((uint64_t)ZS_UNI32((uint32_t)(r.cache >> 32)) << 32);
#endif
        }
        const int sh = r.pos - nb - r.cbase;
        const uint64_t bits = sh < 64 ? r.cache >> sh : 0;
        int rem = nb;
        auto take = [&](int n) -> uint32_t {
          rem -= n;
          return (uint32_t)(bits >> rem) & ((1u << n) - 1u);
        };
        ov = take(co);
        mlen = (vm & 0xFFFFFFu) + take(bm);
        llen = (vl & 0xFFFFFFu) + take(bl);
        sl = (el & 0xFFFFu) + take(nl);
        sm = (em & 0xFFFFu) + take(nm);
        so = (eo & 0xFFFFu) + take(no);
        r.pos -= nb;
      } else {
        if (co > 24) {
          const uint32_t hi = bitr_read(r, co - 16);
          ov = (hi << 16) | bitr_read(r, 16);
        } else {
          ov = bitr_read(r, co);
        }
        mlen = (vm & 0xFFFFFFu) + bitr_read(r, bm);
        llen = (vl & 0xFFFFFFu) + bitr_read(r, bl);
        if (more) {
          sl = (el & 0xFFFFu) + bitr_read(r, nl);
          sm = (em & 0xFFFFu) + bitr_read(r, nm);
          so = (eo & 0xFFFFu) + bitr_read(r, no);
        }
      }
      const uint32_t oval = (1u << co) + ov;
      uint32_t bad = r.pos < 0 ? 1u : 0u;
      // the repeat offsets: three scalars and selects (an array indexed by the repeat code would live in scratch memory)
      const bool is_rep = oval <= 3;
      const uint32_t idx = oval - 1 + (llen == 0 ? 1u : 0u);
      uint32_t rv = rep0;
      rv = idx == 1 ? rep1 : rv;
      rv = idx == 2 ? rep2 : rv;
      rv = idx == 3 ? rep0 - 1 : rv;
      const uint32_t offset = is_rep ? rv : oval - 3;
      const bool change = !is_rep || idx != 0, deep = !is_rep || idx >= 2;
      rep2 = deep ? rep1 : rep2;
      rep1 = change ? rep0 : rep1;
      rep0 = change ? offset : rep0;
      const uint32_t reach = bout + llen;
      const uint32_t nbout = reach + mlen;
      // RFC 8878 3.1.1.1.2 / 3.1.1.5: no offset beyond min(Window_Size, bytes of the frame so far).  That is also all the
      // stream keeps, so this check is the bound of every match read below.
      const uint64_t have = (uint64_t)total0 + reach;
      const uint64_t lim = have < wnd ? have : wnd;
      bad |= (offset == 0 ? 1u : 0u) | (lit_pos + llen > regen32 ? 1u : 0u) | (nbout > (uint32_t)kMaxBlock ? 1u : 0u) |
             ((uint64_t)offset > lim ? 1u : 0u);
      const bool over = execute && nbout > bcap;
      if (bad | (over ? 1u : 0u)) return ZS_FAIL();  // (over: the size pass measured another size - the input changed under us)
      if (execute) {
        if (llen) {
          if (lit_rle >= 0) put_fill(w, bdst + bout, rq0 + bout, (uint8_t)lit_rle, llen, L);
          else put_literals(w, bdst + bout, rq0 + bout, lit, regen32, lit_pos, llen, L, litw_base);
        }
        const bool near = offset <= (uint32_t)kRing && offset + mlen <= (uint32_t)kRing;
        if (!near) {  // a far source comes from memory: what was stored since the last fence must have landed
          const bool fence = offset >= mlen ? offset < nbout - visible : reach > visible;
          if (fence) {
            ZS_FENCE();
            visible = reach;
          }
        }
        put_match(w, bdst + reach, rq0 + reach, offset, mlen, near, L);
      }
      lit_pos += llen;
      bout = nbout;
    }
    if (r.pos != 0) return ZS_FAIL();
  } else if (b != bend) {
    return ZS_FAIL();
  }
  const uint32_t rest = regen32 - lit_pos;
  if (execute) {
    if (bout + rest > bcap) return ZS_FAIL();
    if (rest) {
      if (lit_rle >= 0) put_fill(w, bdst + bout, rq0 + bout, (uint8_t)lit_rle, rest, L);
      else put_literals(w, bdst + bout, rq0 + bout, lit, regen32, lit_pos, rest, L, litw_base);
    }
  }
  bout += rest;
  if (bout > (uint32_t)kMaxBlock) return ZS_FAIL();
  *produced = bout;
  return ZS_OK;
}

// What one run reports: bytes the frame that was open at the start produced in it (they went to the staging area), and whether
// a frame is open behind the last unit.
struct ZPieceRes {
  int64_t resumed_out;
  int32_t open, rc;
};

// The units [u0, u1) of one piece, in order.  resumed: the first units belong to the frame whose state is *st_in, its history
// staging[0, hist_len) and its output in this run staging[hist_len, ...); frames that start in the run decode to
// dst + unit_out[their header's unit].  execute = false: the size pass - dsize[u] of every compressed block is written, nothing
// else.  execute = true: dsize[u] is what the block must decode to, and the frame left open behind u1 - 1 writes *st_out.
ZS_HD int run_piece(Work& w, HufWork& h, const uint8_t* comp, const ZUnit* units, uint32_t* dsize, const int64_t* unit_out, int32_t u0,
                    int32_t u1, bool execute, bool resumed, const ZStreamState* st_in, ZStreamState* st_out, uint8_t* dst,
                    uint8_t* staging, int64_t hist_len, uint8_t* lit_buf, Lanes L, ZPieceRes* res) {
  uint32_t rep0 = 1, rep1 = 4, rep2 = 8;
  int64_t window = 0, fcs = -1;
  int64_t total = 0;         // bytes of the open frame so far
  int64_t op = 0;            // ... of which obase[0, op) are addressable
  uint8_t* obase = dst;
  bool open = false;
  res->resumed_out = 0;
  w.have_ll = w.have_ml = w.have_of = 0;
  w.vals_ll = w.vals_ml = 0;
  h.have_huf = 0;
  if (resumed) {
    for (int i = L.lane; i < (int)(sizeof(ZStreamState::ll) / 4); i += L.n) w.ll[i] = st_in->ll[i];
    for (int i = L.lane; i < (int)(sizeof(ZStreamState::ml) / 4); i += L.n) w.ml[i] = st_in->ml[i];
    for (int i = L.lane; i < (int)(sizeof(ZStreamState::of) / 4); i += L.n) w.of[i] = st_in->of[i];
    for (int i = L.lane; i < (1 << kHufLogMax); i += L.n) h.huf[i] = st_in->h.huf[i];
    w.ll_log = st_in->ll_log;
    w.ml_log = st_in->ml_log;
    w.of_log = st_in->of_log;
    w.have_ll = st_in->have_ll;
    w.have_ml = st_in->have_ml;
    w.have_of = st_in->have_of;
    h.huf_log = st_in->h.huf_log;
    h.have_huf = st_in->h.have_huf;
    rep0 = ZS_UNI32(st_in->rep0);
    rep1 = ZS_UNI32(st_in->rep1);
    rep2 = ZS_UNI32(st_in->rep2);
    total = st_in->produced;
    window = st_in->window;
    fcs = st_in->fcs;
    open = true;
    obase = staging;
    op = hist_len;
    if (execute) {  // the ring holds the frame's most recent bytes: near matches read it, not memory
      const int64_t from = op > kRing ? op - kRing : 0;
      for (int64_t q = from + L.lane; q < op; q += L.n) w.ring[(uint32_t)q & (kRing - 1)] = staging[q];
    }
    ZS_FENCE();
  }
  for (int32_t u = u0; u < u1; u++) {
    const ZUnit z = units[u];
    const int kind = z.kind & 15;
    if (kind == ZU_SKIP) continue;
    if (kind == ZU_FRAME) {
      FrameHdr fh;
      if (frame_header(comp + z.off, z.payload, &fh) != ZS_OK) return ZS_FAIL();
      window = fh.window;
      fcs = fh.fcs;
      rep0 = 1;
      rep1 = 4;
      rep2 = 8;
      w.have_ll = w.have_ml = w.have_of = 0;
      w.vals_ll = w.vals_ml = 0;
      h.have_huf = 0;
      total = 0;
      op = 0;
      obase = execute ? dst + unit_out[u] : dst;
      open = true;
      continue;
    }
    if (!open) return ZS_FAIL();
    const uint8_t* b = comp + z.off + 3;
    uint32_t n = (uint32_t)z.payload;
    if (kind == ZU_COMP) {
      const int rc = stream_block(w, h, b, z.payload, obase, op, total, window, execute, execute ? dsize[u] : 0u, lit_buf, rep0, rep1,
                                  rep2, L, &n);
      if (rc != ZS_OK) return rc;
      if (execute && n != dsize[u]) return ZS_FAIL();
      if (!execute && L.lane == 0) dsize[u] = n;
    } else if (execute) {
      if (kind == ZU_RAW) put_plain(w, obase + op, (uint32_t)op, b, n, L);
      else put_fill(w, obase + op, (uint32_t)op, b[0], n, L);
    }
    if (execute) ZS_FENCE();  // (every block ends with one: a later block's far match may read this output from memory)
    op += n;
    total += n;
    if (z.frame_unit == -1) res->resumed_out += n;
    if (z.kind & ZU_LAST) {
      if (fcs >= 0 && fcs != total) return ZS_FAIL();
      open = false;
    } else if (fcs >= 0 && total > fcs) {
      return ZS_FAIL();
    }
  }
  res->open = open ? 1 : 0;
  if (open && execute && st_out) {
    ZS_FENCE();
    for (int i = L.lane; i < (int)(sizeof(ZStreamState::ll) / 4); i += L.n) st_out->ll[i] = w.ll[i];
    for (int i = L.lane; i < (int)(sizeof(ZStreamState::ml) / 4); i += L.n) st_out->ml[i] = w.ml[i];
    for (int i = L.lane; i < (int)(sizeof(ZStreamState::of) / 4); i += L.n) st_out->of[i] = w.of[i];
    for (int i = L.lane; i < (1 << kHufLogMax); i += L.n) st_out->h.huf[i] = h.huf[i];
    if (L.lane == 0) {
      st_out->ll_log = w.ll_log;
      st_out->ml_log = w.ml_log;
      st_out->of_log = w.of_log;
      st_out->have_ll = w.have_ll;
      st_out->have_ml = w.have_ml;
      st_out->have_of = w.have_of;
      st_out->h.huf_log = h.huf_log;
      st_out->h.have_huf = h.have_huf;
      st_out->rep0 = rep0;
      st_out->rep1 = rep1;
      st_out->rep2 = rep2;
      st_out->pad = 0;
      st_out->produced = total;
      st_out->window = window;
      st_out->fcs = fcs;
    }
  }
  return ZS_OK;
}

}  // namespace s3s_zstd
