// decode_stream_core.h — the host arithmetic of the streaming reduce side (s3s_dstream_*, decode_stream.hip): which pieces of
// partitions a window holds, what the plain side of an encrypted window looks like, whether the words a kernel returned can
// be true, which verdict a feed gives and how the stream's position moves.  No HIP in here: the file builds for the host
// alone (tests/model/dstream_model.cpp runs it under the sanitizers against the Python models of the contract,
// tests/stream_damage.py and tests/stream_damage_encrypted.py).  The single feed and the batched feed both call it; the error
// texts and the sticky state stay with them.
//
// Every function works on arrays the caller provides (in the library: the pinned staging area) and allocates nothing.
// Offsets of a window are relative to its first byte.  STORED coordinates count the range as fetched, IVs included; PLAIN
// ones count what discovery and the decoders see.  Without the IO-encryption layer the two are the same.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace s3s_ds {

enum { kCodecNone = 0, kCodecLz4 = 1, kCodecSnappy = 2, kCodecZstd = 3, kCodecLzf = 4 };
enum { kSumNone = 0, kSumAdler32 = 1 };
enum { kOk = 0, kBadFrame = -3, kChecksum = -4, kUnsupported = -6 };  // S3S_OK, S3S_E_BAD_FRAME, S3S_E_CHECKSUM, S3S_E_UNSUPPORTED
constexpr int64_t kIv = 16;                  // the IV in front of every stored partition (one AES block)
constexpr int64_t kMaxCount = 0x7fffff00ll;  // pieces, segments, frames of one feed: they are int32 on the device

// the range as opened: read-only
struct Range {
  const int64_t* off;   // part_offsets[nparts + 1], stored
  const int64_t* ref;   // ref_checksums[nparts] (not read when algo is kSumNone)
  const int64_t* poff;  // encrypted streams: the plain offsets of the partitions [nparts + 1]; else null
  int32_t nparts;
  int algo;
  bool enc() const { return poff != nullptr; }
  bool sums() const { return algo != kSumNone; }
  int64_t total() const { return off[nparts]; }
};

// the stream's position: what a feed commits
struct Pos {
  int64_t pos = 0;    // stored bytes of the range consumed; never inside an IV
  int32_t cur = 0;    // partitions [0, cur) are verified; partition cur is open
  int64_t carry = 0;  // checksum state of partition cur over [off[cur], pos)
};

inline int64_t fresh(int algo) { return algo == kSumAdler32 ? 1 : 0; }  // getValue() of a new Adler32 / CRC32 / CRC32C

inline bool at_end(const Range& R, const Pos& p) { return p.pos == R.total() && p.cur == R.nparts; }

inline int32_t segs_of(int64_t bytes, int64_t seg_bytes) { return (int32_t)((bytes + seg_bytes - 1) / seg_bytes); }

// the smallest window that can hold a unit's header when the window shows nothing of it
inline int64_t min_unit(const Range& R, const Pos& p, int codec, bool zstd_frame_open) {
  const int64_t part_start = R.off[p.cur < R.nparts ? p.cur : R.nparts];
  if (R.enc() && p.pos == part_start) return kIv;  // the IV is the next unit
  switch (codec) {
    case kCodecLz4: return 21;
    case kCodecSnappy: return p.pos == part_start + (R.enc() ? kIv : 0) ? 16 : 4;  // the stream header; a chunk length
    case kCodecLzf: return 5;
    case kCodecZstd: return zstd_frame_open ? 3 : 6;  // a block header; a frame header's first step
    default: return 1;
  }
}

// S3S_CODEC_NONE under encryption: the stored bytes of the window [pos, pos + len) that a feed takes when dst holds cap bytes.
// Known before anything runs: a unit is a byte, or an IV (no output) that is whole in the window.  A window that shows a cut
// IV or a partition shorter than one is left whole - the feed itself decides on those, and its plain bytes fit cap.
inline int64_t none_cut_encrypted(const Range& R, const Pos& p, int64_t len, int64_t cap) {
  const int64_t wend = p.pos + len;
  int64_t out = 0;
  for (int32_t i = p.cur; i < R.nparts && R.off[i] < wend; i++) {
    const int64_t a = R.off[i], b = R.off[i + 1];
    if (b == a) continue;
    int64_t c = p.pos;  // the first cipher byte of the partition in the window: the open partition's is the position
    if (p.pos <= a) {
      if (b - a < kIv || a + kIv > wend) return len;
      c = a + kIv;
    }
    const int64_t e = b < wend ? b : wend;
    if (e - c > cap - out) return c + (cap - out) - p.pos;
    out += e - c;
  }
  return len;
}

// bytes of the window a feed looks at: S3S_CODEC_NONE's units are bytes, so its cut is known before anything runs
// (0 of a window that is not empty: the next unit is a byte and dst holds none)
inline int64_t window_len(const Range& R, const Pos& p, int codec, int64_t comp_len, int64_t cap) {
  if (codec != kCodecNone) return comp_len;
  if (R.enc()) return none_cut_encrypted(R, p, comp_len, cap);
  return cap < comp_len ? cap : comp_len;
}

// nothing to look at: the position still passes the empty partitions it stands in front of.  -> the partition whose checksum
// is wrong (p is left as it was), or -1
inline int32_t pass_empty(const Range& R, Pos& p) {
  int32_t q = p.cur;
  for (; q < R.nparts && R.off[q + 1] <= p.pos; q++)
    if (R.sums() && R.ref[q] != (q == p.cur ? p.carry : fresh(R.algo))) return q;
  if (q != p.cur) p.carry = fresh(R.algo);
  p.cur = q;
  return -1;
}

// ---- the pieces of partitions in the window [pos, pos + L): partition cur (open), the ones that start inside, and empty ones at its end
inline int32_t piece_count(const Range& R, const Pos& p, int64_t L) {
  const int64_t wend = p.pos + L;
  int32_t n = 0;
  while (p.cur + n < R.nparts && (R.off[p.cur + n] < wend || R.off[p.cur + n + 1] <= wend)) n++;
  return n;
}

inline void piece(const Range& R, const Pos& p, int64_t L, int32_t i, int64_t& a, int64_t& b) {  // piece i, clamped to the window
  a = std::max<int64_t>(R.off[p.cur + i] - p.pos, 0);
  b = std::min(R.off[p.cur + i + 1] - p.pos, L);
}

inline int64_t window_segs(const Range& R, const Pos& p, int64_t L, int32_t n, int64_t seg_bytes) {  // checksum segments of all pieces
  int64_t segs = 0, a, b;
  for (int32_t i = 0; i < n; i++) {
    piece(R, p, L, i, a, b);
    segs += segs_of(b - a, seg_bytes);
  }
  return segs;
}

// off[n + 1]: the piece offsets; seg[n + 1]: every piece's first checksum segment; seed[n]: the state its checksum continues
// from (the open partition's carry, a fresh one for the others).  -> the segments of all pieces
inline int64_t fill_pieces(const Range& R, const Pos& p, int64_t L, int32_t n, int64_t seg_bytes, int64_t* off, int32_t* seg, int64_t* seed) {
  int64_t segs = 0;
  for (int32_t i = 0; i < n; i++) {
    piece(R, p, L, i, off[i], off[i + 1]);
    seg[i] = (int32_t)segs;
    segs += segs_of(off[i + 1] - off[i], seg_bytes);
    seed[i] = i == 0 ? p.carry : fresh(R.algo);
  }
  if (n == 0) off[0] = 0;
  seg[n] = (int32_t)segs;
  return segs;
}

// ---- the plain side of a window: what discovery and the decoders see.  Without the layer it IS the stored side -----------------
struct Plain {
  int32_t m = 0;           // plain pieces: the first m pieces of the window
  int64_t PL = 0;          // plain bytes
  int64_t front = 0;       // encrypted: stored bytes of partition cur in front of the window, 0 or >= 16
  int64_t pfront = 0;      //            ... and plain ones
  bool iv_cut = false;     // piece m is a partition whose IV the window's end cuts: it contributes nothing yet
  bool short_part = false; // piece m is a partition shorter than an IV: corrupt, reported by the feed that consumes everything in front of it
  bool first_mid = false;  // piece 0 starts inside a codec stream (no Snappy stream header expected there)
  int64_t pleft = 0;       // what the RANGE still holds from the window's start, in plain bytes: a unit that crosses it is corrupt, not cut
  int64_t plast_pend = 0;  // where the last plain piece's partition ends (>= PL when the window cuts it)
  const int64_t* q = nullptr;  // encrypted: q[m + 1] plain piece offsets, c[m] the first cipher byte of every plain piece
  const int64_t* c = nullptr;
};

// off[n + 1]: fill_pieces' offsets.  Encrypted: q[n + 1] and c[n] are filled (as far as m); else they are not touched
inline Plain plain_side(const Range& R, const Pos& p, int64_t L, int32_t n, const int64_t* off, int64_t* q, int64_t* c) {
  Plain pl;
  const int32_t np = R.nparts;
  const int64_t last_pend = n > 0 ? R.off[p.cur + n] - p.pos : 0;  // where the last piece's partition ends (>= L: the window cuts it)
  if (!R.enc()) {
    pl.m = n;
    pl.PL = L;
    pl.first_mid = p.pos > R.off[p.cur];
    pl.pleft = R.total() - p.pos;
    pl.plast_pend = last_pend;
    return pl;
  }
  pl.front = p.cur < np ? p.pos - R.off[p.cur] : 0;
  pl.pfront = pl.front > 0 ? pl.front - kIv : 0;
  // the first m pieces, up to the first whose IV the window's end cuts or whose partition is shorter than an IV
  for (int32_t i = 0; i < n; i++) {
    const int64_t stored = R.off[p.cur + i + 1] - R.off[p.cur + i];
    int64_t c0;
    if (i == 0 && pl.front > 0) c0 = 0;
    else if (stored == 0) c0 = off[i];
    else if (stored < kIv) { pl.short_part = true; break; }
    else if (off[i + 1] - off[i] < kIv) { pl.iv_cut = true; break; }
    else c0 = off[i] + kIv;
    q[i] = pl.PL;
    c[i] = c0;
    pl.PL += off[i + 1] - c0;
    pl.m = i + 1;
  }
  q[pl.m] = pl.PL;
  pl.q = q;
  pl.c = c;
  pl.first_mid = pl.pfront > 0;
  if (pl.short_part) pl.pleft = pl.PL;  // the plain side ends at a partition shorter than its IV: nothing valid lies behind it
  else pl.pleft = R.poff[np] - (R.poff[p.cur] + pl.pfront);
  if (pl.m > 0) {
    const int64_t plain_len = R.poff[p.cur + pl.m] - R.poff[p.cur + pl.m - 1];       // of partition cur + m - 1
    pl.plast_pend = q[pl.m - 1] + plain_len - (pl.m == 1 ? pl.pfront : 0);  // (m == 1: it is the open partition, pfront of it lie in front)
  }
  return pl;
}

// a plain offset of the window as a stored one: add 16 for every IV passed (an IV in front of the next plain byte is passed:
// a unit of no output always fits)
inline int64_t to_stored(const Plain& pl, int64_t x) {
  if (!pl.q) return x;       // one coordinate system
  if (pl.m == 0) return 0;   // no plain piece (a cut IV or a short partition at the window's start): nothing can be consumed
  // the LAST piece that starts at or in front of x (q[0] = 0 <= x): of several pieces that start AT x - empty ones, and the
  // one x lies in - the last, so that the IVs (and empty partitions) between them are passed
  const int64_t i = (std::upper_bound(pl.q, pl.q + pl.m, x) - pl.q) - 1;
  return pl.c[i] + (x - pl.q[i]);
}

// the first unit does not fit dst and nothing in front of it (an IV) can be taken either: S3S_E_CAPACITY, nothing consumed
inline bool nothing_fits(const Plain& pl, int64_t consumed) { return consumed == 0 && to_stored(pl, 0) == 0; }

// the cut's plain answer back on the stored side
struct Stored {
  bool into_short_part;  // the feed would consume into a partition shorter than its IV: corrupt
  int64_t consumed, need_comp;
};
inline Stored back_to_stored(const Plain& pl, int64_t consumed, int64_t need_comp) {
  Stored s = {pl.short_part && consumed == pl.PL, 0, need_comp};
  if (s.into_short_part) return s;
  s.consumed = to_stored(pl, consumed);
  if (s.consumed == 0 && pl.iv_cut) s.need_comp = kIv;  // the window starts with a partition and shows less than its IV
  return s;
}

// ---- can the words a kernel returned be true? ----------------------------------------------------------------------------------
// discovery: the chain stopped at `stop`, and the unit there needs `need` bytes (0: it stopped on a unit boundary at PL)
inline bool stop_valid(int64_t stop, int64_t need, int64_t PL) { return stop >= 0 && stop <= PL && (stop == PL || need > PL - stop); }
// the capacity cut: k units, `consumed` bytes of the window, out_len decoded bytes
inline bool cut_valid(int64_t k, int64_t consumed, int64_t out_len, int64_t n_frames, int64_t stop, int64_t cap) {
  return k >= 0 && k <= n_frames && consumed >= 0 && consumed <= stop && out_len >= 0 && out_len <= cap;
}
// Zstandard: the frame that stays open behind the cut (frame_unit >= 0: it started in this feed, at out_start of its output)
inline bool open_frame_valid(int64_t open_after, int64_t frame_unit, int64_t window, int64_t out_start, int64_t wmax, int64_t out_len) {
  return !(open_after && frame_unit >= 0) || (window >= 0 && window <= wmax && out_start >= 0 && out_start <= out_len);
}

// ---- verdicts ------------------------------------------------------------------------------------------------------------------------
// sums[n]: the checksum state behind every piece (seeded).  The first partition whose last byte the window holds and whose
// checksum is wrong, or -1
inline int32_t wrong_sum(const Range& R, const Pos& p, int64_t L, int32_t n, const int64_t* sums) {
  if (R.sums())
    for (int32_t i = 0; i < n; i++)
      if (R.off[p.cur + i + 1] <= p.pos + L && sums[i] != R.ref[p.cur + i]) return p.cur + i;
  return -1;
}

// A kernel's non-zero status word (kBadFrame for a corrupt payload).  The one-shot call reports a wrong checksum before a
// corrupt frame: so does a feed for the partitions whose last byte its window holds (a corrupt frame in a partition that is
// still open comes first - nothing else is known about it yet).  A unit that claims more decoded bytes than any decoder
// takes is refused, not corrupt: nothing is consumed and nothing sticks, the same feed gets the same answer.
struct Refusal {
  int code;     // kChecksum (sticks, bad = the partition) | kUnsupported (does not stick) | kBadFrame (sticks)
  int32_t bad;
};
inline Refusal refusal(const Range& R, const Pos& p, int64_t L, int32_t n, const int64_t* sums, int status) {
  const int32_t bad = wrong_sum(R, p, L, n, sums);
  if (bad >= 0) return {kChecksum, bad};
  return {status == kUnsupported ? kUnsupported : kBadFrame, -1};
}

// the verdict of every partition whose last byte a feed that takes `consumed` (stored) bytes consumes, before anything is decoded
struct Verdict {
  int32_t bad;  // the first partition with a wrong checksum, or -1
  int32_t cur;  // else: the partition left open
};
inline Verdict verdict(const Range& R, const Pos& p, int64_t consumed, const int64_t* sums) {
  int32_t q = p.cur;
  for (; q < R.nparts && R.off[q + 1] <= p.pos + consumed; q++)
    if (R.sums() && sums[q - p.cur] != R.ref[q]) return {q, q};
  return {-1, q};
}

// the checksum state of the partition left open (q = verdict().cur): known already unless the capacity cut ended the feed
// inside its piece - then [a, b) of the window is summed again from `value`, behind the decode launch
struct Carry {
  enum Kind { kSeed, kKnown, kSecond } kind;
  int64_t value;  // kSeed, kKnown: the carry; kSecond: the seed of the second launch
  int64_t a, b;
};
inline Carry open_carry(const Range& R, const Pos& p, int32_t n, const int64_t* off, const int64_t* sums, int32_t q, int64_t consumed) {
  if (!R.sums() || q >= R.nparts) return {Carry::kSeed, fresh(R.algo), 0, 0};
  const int32_t i = q - p.cur;
  const int64_t seed = i == 0 ? p.carry : fresh(R.algo);
  if (i >= n || consumed <= off[i]) return {Carry::kSeed, seed, 0, 0};
  if (consumed == off[i + 1]) return {Carry::kKnown, sums[i], 0, 0};
  return {Carry::kSecond, seed, off[i], consumed};
}

// ---- the commit: the position moves, and the result's need_comp / at_end follow from it -----------------------------------------------
struct Commit {
  int64_t need_comp;
  int32_t at_end;
  int32_t iv_piece;  // encrypted: the piece whose IV is the open partition's from now on (it started in this window), or -1
};
inline Commit commit(const Range& R, Pos& p, int64_t front, int32_t q, int64_t consumed, int64_t carry, int64_t need_comp) {
  const int64_t new_pos = p.pos + consumed;
  Commit c = {consumed == 0 ? need_comp : 0, 0, -1};
  if (R.enc() && q < R.nparts && new_pos > R.off[q] && !(q == p.cur && front > 0)) c.iv_piece = q - p.cur;
  p.pos = new_pos;
  p.cur = q;
  p.carry = carry;
  c.at_end = at_end(R, p);
  return c;
}

}  // namespace s3s_ds
