// aes_ctr_stream_core.h — which key stream units a 16-byte chunk of a WINDOW owns: the arithmetic of the window form of the
// AES-CTR pass (aes_ctr_stream.hip), written once for the device and for the host.
//
// The streaming reduce side (decode_stream.hip) sees a fetched range through windows [pos, pos + L) of its
// stored bytes.  A window starts anywhere behind a partition's IV and ends anywhere, an IV included.  Its pieces of
// partitions are E[0] = 0 <= E[1] <= ... <= E[n] = L (window-relative stored offsets); piece 0's partition began `front`
// stored bytes in front of the window (0: the window starts with the partition, else >= 16: its IV was consumed by an
// earlier feed and travels as an argument).  Everything is 64-bit: front is as large as a partition.
//
// Units, as in aes_ctr.hip: the IV of a partition that starts in the window, or key stream block b of a partition - stored
// bytes [S + 16 + 16 b, + 16) where S is the partition's stored start (E[p], or -front for piece 0), cut at the
// partition's end AND at both ends of the window.  Chunks follow piece 0's key stream, not the window: chunk c is stored
// bytes [16 c - r, 16 c - r + 16) with r = front mod 16, so the unit that began in front of the window (at any residue of its
// block) starts exactly where chunk 0 does and chunk 0 owns it like any other.  A chunk owns the units that START inside it;
// every stored byte of the window that is not part of an IV belongs to exactly one unit, and a unit costs one block encryption.
// An IV that the window's end (or a partition shorter than 16 bytes) cuts is a unit of length 0: its partition contributes
// nothing to this window.
//
// Compiled by hipcc (S3S_AES_DEVICE: aes_ctr_stream.hip) and by g++ (tests/model/aes_ctr_stream_model.cpp).
#pragma once
#include "aes_ctr_core.h"

namespace s3s_aes {

struct WinUnit {
  int32_t part;   // piece of the window
  int32_t is_iv;  // 1: the partition's IV (len 16 when whole, else 0); 0: a key stream block
  int32_t skip;   // bytes of the unit in front of the window (piece 0's first block only), so key stream byte skip is the first used
  int32_t len;    // stored bytes of the unit inside the window and the partition, from start + skip
  int64_t start;  // window-relative stored offset where the unit begins (negative when skip > 0)
  int64_t block;  // key stream block number (-1 for the IV)
  int64_t plain;  // offset of the unit's first used byte in the plain partition (block 16 + skip)
};

struct WinCursor {
  int32_t p;
  int64_t ep, en, xs;  // start / end of piece p as its key stream sees them, the next unit start
};

AC_HD int64_t win_chunk_count(int64_t L, int64_t front) { return (L + (front & 15) + 15) >> 4; }
AC_HD int64_t win_chunk_start(int64_t c, int64_t front) { return 16 * c - (front & 15); }

// the last p in [lo, hi] with E[p] <= x, lo when there is none
AC_HD int32_t win_last_start_le(const int64_t* E, int32_t lo, int32_t hi, int64_t x) {
  while (lo < hi) {
    const int32_t mid = (int32_t)(((int64_t)lo + hi + 1) >> 1);
    if (E[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the chunk that starts at x0 lies in piece p (E[p] <= x0 < E[p + 1], or p = 0 for the chunk in front of the window)
AC_HD void win_open(WinCursor& c, const int64_t* E, int32_t p, int64_t front, int64_t x0) {
  c.p = p;
  c.ep = p == 0 ? E[0] - front : E[p];
  c.en = E[p + 1];
  c.xs = x0 + ((16 - ((x0 - c.ep) & 15)) & 15);  // the first unit start of piece p at or behind x0
}

// The next unit that starts in [x0, lim) -> whether there is one (u is filled either way: a lane without a unit still
// encrypts u.block).  L = E[n], the window's length; lim <= L the end of the chunk.
AC_HD bool win_next(WinCursor& c, const int64_t* E, int32_t n, int64_t L, int64_t lim, bool live, WinUnit& u) {
  // the piece ends in front of the unit and inside the chunk: the next non-empty one starts there with its IV
  while (live && c.xs >= c.en && c.en < lim && c.p + 1 < n) {
    c.p++;
    c.ep = c.en;
    c.en = E[c.p + 1];
    if (c.en > c.ep) c.xs = c.ep;
  }
  const bool has = live && c.xs < lim && c.xs < c.en;
  const int64_t j = c.xs - c.ep;  // 0: the IV; 16 (b + 1): key stream block b
  const int64_t end = c.en < L ? c.en : L;
  const int64_t lo = c.xs < 0 ? 0 : c.xs, hi = c.xs + 16 < end ? c.xs + 16 : end;
  u.part = c.p;
  u.is_iv = j == 0;
  u.start = c.xs;
  u.block = (j >> 4) - 1;
  u.skip = (int32_t)(lo - c.xs);
  u.len = has && hi > lo ? (int32_t)(hi - lo) : 0;
  if (u.is_iv && u.len < 16) u.len = 0;  // an IV the window's end cuts: nothing of its partition is in this window
  u.plain = j - 16 + u.skip;
  c.xs += 16;
  return has;
}

}  // namespace s3s_aes
