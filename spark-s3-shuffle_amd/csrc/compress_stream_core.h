// compress_stream_core.h — the arithmetic of the streaming map side (s3s_cstream_*, compress_stream.hip): which units a
// window holds, which of them a feed takes at a given capacity, and how the stream's host state moves.  No HIP in here: the
// file builds for the host alone (tests/model/cstream_model.cpp runs it under the sanitizers against the Python model of the
// contract, tests/cstream_units.py) and for the device (the cut kernel, compress_stream_kernels.hip, uses cut_lane).
//
// Units of a window (include/s3shuffle_codec.h, "map side, streaming"):
//   a block       blockSize source bytes of the open partition, or what is left of a partition whose end lies in the window;
//                 Snappy: the 16-byte stream header belongs to the unit of a partition's first block
//   an LZ4 end    the 21-byte end frame of a non-empty partition; no source bytes
// An end that has no bytes of its own (every codec but LZ4; an empty partition) is passed as soon as every unit in front of
// it is taken.  S3S_CODEC_NONE has bytes for units and is cut without a plan (none_cut).
// Under IO encryption (s3s_cstream_open_encrypted; tests/model/cstream_encrypted_model.cpp against
// tests/cstream_units_encrypted.py) the 16-byte IV of a non-empty partition belongs to the unit of its first block: one more
// plan record in front of that unit (iv_records), 17 image bytes for a partition's first byte under S3S_CODEC_NONE
// (none_cut_encrypted), 16 more bytes a piece in feed_bound_encrypted.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define S3S_CS_HD __host__ __device__
#else
#define S3S_CS_HD
#endif

namespace s3s_cs {

enum { kCodecNone = 0, kCodecLz4 = 1, kCodecSnappy = 2, kCodecZstd = 3, kCodecLzf = 4 };
constexpr int kLz4EndFrame = 21;
constexpr int kLzfBlock = 65535;

// what a stream carries from feed to feed (the open partition's checksum state travels next to it)
struct State {
  int64_t pos = 0;         // source bytes consumed
  int64_t written = 0;     // image bytes produced
  int64_t open_bytes = 0;  // source bytes of the open partition consumed so far (a multiple of the block size, or all of
                           // an LZ4 partition whose end frame is still to come)
  int64_t open_img = 0;    // image bytes of the open partition written so far
};

struct Unit {
  int64_t src_off;      // window-relative start of its source bytes
  int32_t len;          // source bytes; 0: the LZ4 end frame
  int32_t piece;        // piece of the window it lies in: j = the partition that ends at ends[j], n_ends = the one left open
  int32_t first;        // the partition's first block (Snappy: the stream header goes in front)
  int32_t ends_before;  // ends passed once every unit in front of this one is taken
};

struct Plan {
  int64_t n_units = 0;
  int64_t n_blocks = 0;
};

// ends: negative, descending or beyond src_len is the caller's S3S_E_INVALID
inline bool ends_valid(int64_t src_len, const int64_t* ends, int32_t n_ends) {
  int64_t prev = 0;
  for (int32_t j = 0; j < n_ends; j++) {
    if (ends[j] < prev || ends[j] > src_len) return false;
    prev = ends[j];
  }
  return true;
}

// the units of the window in image order; emit(const Unit&) is called once for each
template <typename F>
inline Plan plan_units(int codec, int64_t bs, int64_t open_bytes, int64_t src_len, const int64_t* ends, int32_t n_ends, F&& emit) {
  Plan pl;
  int64_t start = 0;
  for (int32_t j = 0; j <= n_ends; j++) {
    const bool closes = j < n_ends;
    const int64_t had = j == 0 ? open_bytes : 0;
    const int64_t L = (closes ? ends[j] : src_len) - start;
    const int64_t take = closes ? L : L - L % bs;  // behind the last end only whole blocks
    for (int64_t p = 0; p < take; p += bs) {
      const int64_t len = take - p < bs ? take - p : bs;
      emit(Unit{start + p, (int32_t)len, j, had == 0 && p == 0, j});
      pl.n_units++;
      pl.n_blocks++;
    }
    if (closes && codec == kCodecLz4 && had + L > 0) {
      emit(Unit{ends[j], 0, j, 0, j});
      pl.n_units++;
    }
    if (closes) start = ends[j];
  }
  return pl;
}

struct Cut {
  int64_t k = 0;             // units taken
  int64_t consumed = 0;
  int64_t out_len = 0;
  int64_t need_src = 0;
  int64_t need_dst = 0;      // != 0: S3S_E_CAPACITY, nothing taken
  int32_t parts_closed = 0;
};

// The cut, serially: units[0, n) with cum[i] = image bytes of the units in front of unit i (cum[n] = all of them).
// This is what the cut kernel computes with one wavefront.
inline Cut cut_units(const Unit* units, const int64_t* cum, int64_t n, int32_t n_ends, int64_t need_src_unit, int64_t cap) {
  Cut c;
  int64_t k = 0;
  while (k < n && cum[k + 1] <= cap) k++;
  c.parts_closed = k < n ? units[k].ends_before : n_ends;
  if (k == 0 && n > 0 && c.parts_closed == 0) {
    c.need_dst = cum[1];
    return c;
  }
  c.k = k;
  c.consumed = k > 0 ? units[k - 1].src_off + units[k - 1].len : 0;
  c.out_len = cum[k];
  if (n == 0 && n_ends == 0) c.need_src = need_src_unit;
  return c;
}

// S3S_CODEC_NONE: the units are bytes
inline Cut none_cut(int64_t src_len, const int64_t* ends, int32_t n_ends, int64_t cap) {
  Cut c;
  const int64_t take = src_len < cap ? src_len : cap;
  while (c.parts_closed < n_ends && ends[c.parts_closed] <= take) c.parts_closed++;
  if (take == 0 && src_len > 0 && c.parts_closed == 0) {
    c.need_dst = 1;
    return c;
  }
  c.k = c.consumed = c.out_len = take;
  if (src_len == 0 && n_ends == 0) c.need_src = 1;
  return c;
}

// S3S_CODEC_NONE under IO encryption (s3s_cstream_open_encrypted): the units are still bytes, but the unit of a partition's
// first byte is 17 image bytes - its IV goes in front.  open_img > 0: the open partition's IV was written by an earlier feed.
// piece_off[0, n_ends + 1] (or null) gets the stored piece offsets of the output, clamped to out_len (the E of the AES-CTR pass).
inline Cut none_cut_encrypted(int64_t open_img, int64_t src_len, const int64_t* ends, int32_t n_ends, int64_t cap, int64_t* piece_off) {
  Cut c;
  int64_t start = 0, out = 0, first_need = 0;
  bool open = true;  // every unit in front is taken
  for (int32_t j = 0; j <= n_ends; j++) {
    const int64_t end = j < n_ends ? ends[j] : src_len;
    const int64_t len = end - start, lead = len > 0 && !(j == 0 && open_img > 0) ? 16 : 0;
    if (piece_off) piece_off[j] = out;
    if (open && lead + len <= cap - out) {
      out += lead + len;
      c.consumed = end;
      if (j < n_ends) c.parts_closed = j + 1;
    } else if (open) {
      if (cap - out > lead) {  // the IV and at least one byte
        c.consumed = start + (cap - out - lead);
        out = cap;
      } else if (out == 0 && c.parts_closed == 0) {
        first_need = lead + 1;
      }
      open = false;
    }
    start = end;
  }
  if (piece_off) piece_off[n_ends + 1] = out;
  if (first_need) {
    c = Cut();
    c.need_dst = first_need;
    return c;
  }
  c.k = c.consumed;
  c.out_len = out;
  if (src_len == 0 && n_ends == 0) c.need_src = 1;
  return c;
}

// piece_off[0, n_ends + 1]: where the pieces of partitions start in this feed's output (clamped to out_len); piece j < n_ends
// is the partition that ends at ends[j].  The image lengths of the partitions the feed closes (the cut kernel writes the same):
inline void closed_lengths(const State& s, const Cut& c, const int64_t* piece_off, int64_t* lengths) {
  for (int32_t j = 0; j < c.parts_closed; j++) lengths[j] = piece_off[j + 1] - piece_off[j] + (j == 0 ? s.open_img : 0);
}

// the state behind a feed that took `c`
inline void advance(State* s, const Cut& c, const int64_t* ends, const int64_t* piece_off) {
  s->pos += c.consumed;
  s->written += c.out_len;
  if (c.parts_closed > 0) {
    s->open_bytes = c.consumed - ends[c.parts_closed - 1];
    s->open_img = c.out_len - piece_off[c.parts_closed];
  } else {
    s->open_bytes += c.consumed;
    s->open_img += c.out_len;
  }
}

// a dst_capacity that holds whatever a window of src_len bytes and n_ends ends compresses to
inline int64_t feed_bound(int codec, int64_t bs, int64_t src_len, int32_t n_ends) {
  if (codec == kCodecNone) return src_len;
  const int64_t blocks = src_len / bs + n_ends + 1;  // every piece may end in a short block
  if (codec == kCodecLz4) return src_len + kLz4EndFrame * (blocks + n_ends);
  if (codec == kCodecSnappy) return src_len + src_len / 6 + 37 * blocks + 16 * ((int64_t)n_ends + 1);  // 4 + MaxCompressedLength per block
  return src_len + 7 * blocks;  // LZF
}

// ... under IO encryption: every piece may start its partition, with a 16-byte IV
inline int64_t feed_bound_encrypted(int codec, int64_t bs, int64_t src_len, int32_t n_ends) {
  return feed_bound(codec, bs, src_len, n_ends) + 16 * ((int64_t)n_ends + 1);
}

// ---- the cut kernel's side ---------------------------------------------------------------------------------------------------
// One record per plan item (a unit is one or more items: a Snappy header, a chunk head and its fragments).
struct Mark {
  int64_t src_end;     // window bytes consumed once this item's unit is taken
  int32_t last;        // 1: the last item of its unit
  int32_t ends_after;  // ends passed once this item's unit is taken and the next is not
};

// IO encryption: one IV record (kItemIv, 16 image bytes) goes in front of the items of every unit that starts its partition.
// Like a Snappy stream header it is not the last item of its unit, so the cut takes or leaves it with the block behind it.
inline int32_t iv_records(const Unit& u, bool encrypted) { return encrypted && u.first ? 1 : 0; }

// the marks of one unit's items [i0, i1); ends_after is corrected when the next unit arrives (mark_ends_after)
inline void mark_unit(Mark* marks, int32_t i0, int32_t i1, const Unit& u, int32_t n_ends) {
  for (int32_t i = i0; i < i1; i++) marks[i] = Mark{u.src_off + u.len, i == i1 - 1, n_ends};
}
inline void mark_ends_after(Mark* marks, int32_t i0, int32_t i1, int32_t ends_before) {
  for (int32_t i = i0; i < i1; i++) marks[i].ends_after = ends_before;
}

// result words of the cut kernel
enum { kCutK = 0, kCutConsumed = 1, kCutOutLen = 2, kCutNeedDst = 3, kCutPartsClosed = 4, kCutWords = 8 };

// item i ends a unit that fits: ascending in i, so the largest such i is the cut
S3S_CS_HD inline bool cut_lane(const Mark& m, int64_t end_off, int64_t cap) { return m.last != 0 && end_off <= cap; }

}  // namespace s3s_cs
