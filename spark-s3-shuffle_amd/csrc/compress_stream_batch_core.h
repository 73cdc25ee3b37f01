// compress_stream_batch_core.h — the host rules of BOTH feeds of the streaming map side (s3s_cstream_feed* and
// s3s_cstream_feed_batch*, compress_stream.hip): what a window counts, which entries are refused, answered on the host or
// become windows, where the windows of one call lie in ONE plan (the single feed is a call of one window), what the device is
// told about each of them, and how a stream's host state moves once the download has come back (take_window).  No HIP in here
// and no allocation: the file builds for the host alone (tests/model/cstream_batch_model.cpp runs these very functions under
// the sanitizers against the Python model of the contract, tests/cstream_units.py) and for the device (cstream_cut_batch_kernel
// and gather_items_cut_batch_kernel, compress_stream_batch_kernels.hip, read CutEntry).  What a codec's unit is in items, slots
// and checksum segments (s3s_ctx.h) comes in through functors.
//
// Under IO encryption (tests/model/cstream_batch_encrypted_model.cpp against tests/cstream_units_encrypted.py)
// the up part of the arena grows by the call's IVs (16 bytes per piece, at first_piece), one PassWindow per batched window and
// the tile -> window map of the ONE encrypt pass (aes_ctr_cstream_batch.hip); plan_entry_encrypted puts the kItemIv records
// into the plan, commit_iv is the IV bookkeeping of the single and the batched feed.
//
// One call, m batched entries.  Every array of the call is packed entry after entry, in entry order:
//   per item            items, marks, item_size          entry e starts at first_item
//                       item_off                         ... at first_item + e: the scan writes n_items + 1 offsets an entry
//   n_pieces + 1 each   part_first, seg_start, piece_off ... at first_pp = first_piece + e
//   n_pieces each       seeds, sums, piece -> entry      ... at first_piece
//   n_ends each         lengths                          ... at first_len = first_piece - e
//   per entry           TaskTail, CutEntry, status word, kCutWords result words
// part_first and seg_start restart at 0 in every entry (item and segment numbers relative to the entry), slots and items are
// numbered through the call.  A plan item addresses its source as a signed offset from ONE base pointer - the first batched
// entry's d_src - so src_off = (entry's d_src - base) + the unit's offset in its window, and may be negative.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "compress_stream_core.h"

namespace s3s_cs {

// what the device side of one batched entry needs beside its TaskTail (s3s_internal.h)
struct CutEntry {
  int64_t dst_capacity;
  int64_t open_img;              // image bytes the open partition has already
  int32_t first_item, n_items;
  int32_t first_pp, n_pieces;
  int32_t first_piece, first_len;
  int32_t first_seg, n_segs;     // checksum segment slots (worst case, host-built)
  int32_t first_slot, n_slots;
  int32_t first_last, ends0;     // the last item of the first unit; ends passed in front of the first unit
};

// running totals of a call while its entries are reserved
struct Totals {
  int64_t items = 0, slots = 0, pieces = 0, segs = 0;
  int32_t m = 0;
  int64_t pp() const { return pieces + m; }    // entries of the n + 1 arrays
  int64_t lens() const { return pieces - m; }  // entries of the lengths
};

constexpr int64_t kBatchMax = 0x7fffff00ll;  // what an int32 index of the call may reach

// the arguments the single feed answers S3S_E_INVALID (null_with_length: a null pointer next to a non-zero length, the caller's test)
inline bool window_refused(int64_t src_len, const int64_t* ends, int32_t n_ends, int64_t dst_capacity, bool null_with_length) {
  return src_len < 0 || n_ends < 0 || dst_capacity < 0 || null_with_length || !ends_valid(src_len, ends, n_ends);
}

// what a window's units come to: plan items (with the IV records), codec slots, units.  items_of(u) / slots_of(u): of one unit
struct Count {
  int64_t items = 0, slots = 0, units = 0;
};
template <typename ItemsOf, typename SlotsOf>
inline Count count_window(int codec, int64_t bs, int64_t open_bytes, int64_t src_len, const int64_t* ends, int32_t n_ends, bool encrypted,
                          ItemsOf&& items_of, SlotsOf&& slots_of) {
  Count n;
  n.units = plan_units(codec, bs, open_bytes, src_len, ends, n_ends, [&](const Unit& u) {
    n.items += iv_records(u, encrypted) + items_of(u);
    n.slots += slots_of(u);
  }).n_units;
  return n;
}

// Worst-case checksum segments of a window's pieces: segs_of(source bytes of a piece) = the segments of the most image bytes
// it can become.  seg_start (or null): n_ends + 2 entries.  -1: more than an int32 index holds ("window too large")
template <typename SegsOf>
inline int64_t piece_segs(int64_t src_len, const int64_t* ends, int32_t n_ends, int32_t* seg_start, SegsOf&& segs_of) {
  int64_t segs = 0;
  for (int32_t j = 0; j <= n_ends; j++) {
    const int64_t a = j == 0 ? 0 : ends[j - 1], b = j < n_ends ? ends[j] : src_len;
    if (seg_start) seg_start[j] = (int32_t)segs;
    segs += segs_of(b - a);
    if (segs > kBatchMax) return -1;
  }
  if (seg_start) seg_start[n_ends + 1] = (int32_t)segs;
  return segs;
}

// An entry of a batched call: refused by its arguments (window_refused), answered on the host - its window launches nothing,
// or has more items or segments (segs < 0) than one feed takes: the single feed's answer either way - or a window of the batch
enum Route { kRouteRefused, kRouteHost, kRouteWindow };
inline Route route_entry(bool refused, const Count& n, int64_t segs) {
  if (refused) return kRouteRefused;
  return n.items == 0 || n.items > kBatchMax || segs < 0 ? kRouteHost : kRouteWindow;
}

// the cut of a window that launches nothing: every end is passed; without one the caller learns the window that holds a unit
inline Cut cut_nothing(int32_t n_ends, int64_t need_src_unit) {
  Cut c;
  c.parts_closed = n_ends;
  if (n_ends == 0) c.need_src = need_src_unit;
  return c;
}

// a plan item's source: the unit's offset in its window, seen from the call's base pointer (addresses as integers)
inline int64_t item_src_off(int64_t src_addr, int64_t base_addr, int64_t unit_off) { return (src_addr - base_addr) + unit_off; }

// the feed that wrote nothing: every end it passes closes a partition with what the stream already holds
inline void commit_nothing(State* st, int64_t* carry, int64_t fresh, int32_t parts_closed, int64_t* out_lengths, int64_t* out_checksums) {
  for (int32_t j = 0; j < parts_closed; j++) {
    out_lengths[j] = j == 0 ? st->open_img : 0;
    if (out_checksums) out_checksums[j] = j == 0 ? *carry : fresh;
  }
  if (parts_closed > 0) {
    *carry = fresh;
    st->open_bytes = st->open_img = 0;
  }
}

// does one more entry of this size keep every index of the call inside int32?
inline bool fits_call(const Totals& t, int64_t n_items, int64_t n_slots, int32_t n_ends, int64_t n_segs) {
  return t.items + n_items <= kBatchMax && t.slots + n_slots <= kBatchMax && t.pieces + n_ends + 1 + t.m + 1 <= kBatchMax &&
         t.segs + n_segs <= kBatchMax;
}

// the next entry's place in every packed array
inline CutEntry reserve(Totals* t, int64_t n_items, int64_t n_slots, int32_t n_ends, int64_t n_segs, int64_t dst_capacity, int64_t open_img) {
  CutEntry c = {};
  c.dst_capacity = dst_capacity;
  c.open_img = open_img;
  c.first_item = (int32_t)t->items;
  c.n_items = (int32_t)n_items;
  c.first_pp = (int32_t)t->pp();
  c.n_pieces = n_ends + 1;
  c.first_piece = (int32_t)t->pieces;
  c.first_len = (int32_t)t->lens();
  c.first_seg = (int32_t)t->segs;
  c.n_segs = (int32_t)n_segs;
  c.first_slot = (int32_t)t->slots;
  c.n_slots = (int32_t)n_slots;
  c.first_last = -1;
  t->items += n_items;
  t->slots += n_slots;
  t->pieces += (int64_t)n_ends + 1;
  t->segs += n_segs;
  t->m++;
  return c;
}

inline size_t arena_al(size_t x) { return (x + 15) & ~size_t(15); }
constexpr size_t kIvBytes = 16;

// The call's small arrays in one block, laid out alike in the pinned staging area and in device memory: [0, up) goes up in one
// copy in front of the kernels, [up, total) is zeroed on the device, written by the kernels and comes down in one copy.
struct Arena {
  size_t items = 0, marks = 0, pf = 0, seg = 0, seed = 0, pw = 0, tails = 0, cuts = 0, up = 0;
  size_t status = 0, res = 0, piece = 0, len = 0, sums = 0, total = 0;
  size_t ivs = 0, wins = 0, tile_win = 0;  // under IO encryption only (otherwise empty, at `up`)
  void lay_out(const Totals& t, size_t item_bytes, size_t tail_bytes) { lay_out_pass(t, item_bytes, tail_bytes, 0, 0, 0); }
  // ... of a call under IO encryption: win_bytes = sizeof(PassWindow), tiles = the grid of the encrypt pass
  void lay_out_encrypted(const Totals& t, size_t item_bytes, size_t tail_bytes, size_t win_bytes, int64_t tiles) {
    lay_out_pass(t, item_bytes, tail_bytes, kIvBytes, win_bytes, (size_t)tiles);
  }
  void lay_out_pass(const Totals& t, size_t item_bytes, size_t tail_bytes, size_t iv_bytes, size_t win_bytes, size_t tiles) {
    const size_t N = (size_t)t.items, PP = (size_t)t.pp(), P = (size_t)t.pieces, L = (size_t)t.lens(), M = (size_t)t.m;
    items = 0;
    marks = arena_al(items + item_bytes * N);
    pf = arena_al(marks + sizeof(Mark) * N);
    seg = arena_al(pf + 4 * PP);
    seed = arena_al(seg + 4 * PP);
    pw = arena_al(seed + 8 * P);
    tails = arena_al(pw + 4 * P);
    cuts = arena_al(tails + tail_bytes * M);
    ivs = arena_al(cuts + sizeof(CutEntry) * M);
    wins = arena_al(ivs + iv_bytes * P);
    tile_win = arena_al(wins + win_bytes * M);
    up = arena_al(tile_win + 4 * tiles);
    status = up;
    res = arena_al(status + 4 * M);
    piece = arena_al(res + 8 * (size_t)kCutWords * M);
    len = arena_al(piece + 8 * PP);
    sums = arena_al(len + 8 * L);
    total = arena_al(sums + 8 * P);
  }
};

// The plan records of one entry, written into the call's arrays: the ONE plan loop of both feeds (the single feed's window is
// an entry whose places are all 0).  items_of(u) = the plan items of unit u; emit(u, at, slot) writes them at item `at` of the CALL (slot: the
// call's slot counter, advanced) with src_off = src_delta + the unit's offset.  marks / part_first: the call's arrays.
// false: the plan does not match the counts the entry was reserved with (nothing may be launched).
// Under IO encryption one more record (emit_iv(u, at): kItemIv) goes in front of the items of every unit that starts its
// partition, as iv_records / mark_unit place it for the single feed: it is counted in n_items, part_first points at it.
template <typename ItemsOf, typename EmitIv, typename Emit>
inline bool plan_entry_records(CutEntry* c, int codec, int64_t bs, int64_t open_bytes, int64_t src_len, const int64_t* ends, int32_t n_ends,
                               Mark* marks, int32_t* part_first, bool encrypted, ItemsOf&& items_of, EmitIv&& emit_iv, Emit&& emit) {
  Mark* m = marks + c->first_item;
  int32_t* pf = part_first + c->first_pp;
  const int32_t n_items = c->n_items, n_pieces = c->n_pieces;
  int32_t it = 0, slot = c->first_slot, piece = 0, prev0 = 0;
  bool fits = true;
  pf[0] = 0;
  plan_units(codec, bs, open_bytes, src_len, ends, n_ends, [&](const Unit& u) {
    const int32_t lead = iv_records(u, encrypted);
    const int64_t mine = lead + items_of(u);
    if (!fits || it + mine > n_items) {
      fits = false;
      return;
    }
    mark_ends_after(m, prev0, it, u.ends_before);
    if (it == 0) c->ends0 = u.ends_before;
    while (piece < u.piece) pf[++piece] = it;
    prev0 = it;
    if (lead) emit_iv(u, c->first_item + it);
    it += lead;
    emit(u, c->first_item + it, slot);
    it += (int32_t)(mine - lead);
    mark_unit(m, prev0, it, u, n_ends);
    if (c->first_last < 0) c->first_last = it - 1;
  });
  while (piece < n_pieces) pf[++piece] = it;
  return fits && it == n_items && slot == c->first_slot + c->n_slots;
}

template <typename ItemsOf, typename Emit>
inline bool plan_entry(CutEntry* c, int codec, int64_t bs, int64_t open_bytes, int64_t src_len, const int64_t* ends, int32_t n_ends,
                       Mark* marks, int32_t* part_first, ItemsOf&& items_of, Emit&& emit) {
  return plan_entry_records(c, codec, bs, open_bytes, src_len, ends, n_ends, marks, part_first, false, items_of, [](const Unit&, int32_t) {}, emit);
}

template <typename ItemsOf, typename EmitIv, typename Emit>
inline bool plan_entry_encrypted(CutEntry* c, int codec, int64_t bs, int64_t open_bytes, int64_t src_len, const int64_t* ends, int32_t n_ends,
                                 Mark* marks, int32_t* part_first, ItemsOf&& items_of, EmitIv&& emit_iv, Emit&& emit) {
  return plan_entry_records(c, codec, bs, open_bytes, src_len, ends, n_ends, marks, part_first, true, items_of, emit_iv, emit);
}

// the seeds of an entry's pieces: the stream's carried state continues into the first, a fresh state starts the others
// (piece_entry: the call's piece -> entry map, or null)
inline void seed_pieces(const CutEntry& c, int32_t entry, int64_t carry, int64_t fresh, int64_t* seeds, int32_t* piece_entry) {
  for (int32_t j = 0; j < c.n_pieces; j++) {
    seeds[c.first_piece + j] = j == 0 ? carry : fresh;
    if (piece_entry) piece_entry[c.first_piece + j] = entry;
  }
}

// ---- under IO encryption: the IVs of the call and the ONE encrypt pass ----------------------------------------------------------
// ONE s3s_set_stream_ivs array holds the IVs of every entry of the call - refused and host-answered ones included - sliced in
// entry order, max(n_ends, 0) + 1 an entry.
inline int64_t iv_slice_len(int32_t n_ends) { return (int64_t)(n_ends > 0 ? n_ends : 0) + 1; }

struct IvSlicer {
  int64_t at = 0;  // IVs of the entries in front
  int64_t take(int32_t n_ends) {
    const int64_t mine = at;
    at += iv_slice_len(n_ends);
    return mine;
  }
};
// "the entries of the batch have N pieces": entry i's slice is [at[i], at[i + 1]) of the call's IVs, N = at[n] is returned
template <typename NEndsOf>
inline int64_t slice_ivs(int32_t n, NEndsOf&& n_ends_of, int64_t* at) {
  IvSlicer slices;
  for (int32_t i = 0; i < n; i++) at[i] = slices.take(n_ends_of(i));
  return at[n] = slices.at;
}

// the IVs of one batched window, into the call's array at its pieces: the entry's slice, entry 0 replaced by the IV the stream
// carries while its open partition already has image bytes
inline void window_ivs(const CutEntry& c, const uint8_t* call_ivs, int64_t slice_at, const uint8_t* carried, uint8_t* ivs) {
  uint8_t* mine = ivs + kIvBytes * (size_t)c.first_piece;
  const uint8_t* from = call_ivs + kIvBytes * (size_t)slice_at;
  for (size_t i = 0; i < kIvBytes * (size_t)c.n_pieces; i++) mine[i] = from[i];
  if (c.open_img > 0)
    for (size_t i = 0; i < kIvBytes; i++) mine[i] = carried[i];
}

// The encrypt pass works in tiles of kPassTile stored bytes that follow the open partition's key stream: tile t of a window is
// its output bytes [kPassTile t - (front & 15), + kPassTile).  out_len is the device's; the host bounds it by the window's
// capacity and by what its source can compress to, and the tiles behind out_len return whole.
constexpr int64_t kPassTile = 16384;
inline int64_t pass_tiles(int64_t dst_capacity, int64_t bound, int64_t front) {
  const int64_t len = dst_capacity < bound ? dst_capacity : bound;
  if (len <= 0) return 0;
  return (len + (front & 15) + kPassTile - 1) / kPassTile;
}

// what a workgroup of the pass needs of its window (device pointers; aes_ctr_cstream_batch.hip reads it through scalar loads)
struct PassWindow {
  uint8_t* out;         // the entry's d_dst
  const int64_t* E;     // its n_pieces + 1 clamped piece offsets (the cut kernel's)
  const uint8_t* ivs;   // its n_pieces IVs
  const int64_t* cut;   // its kCutWords result words
  int32_t n_pieces, tile0;
  int64_t front;        // stored bytes of the open partition in front of the output
};

inline PassWindow pass_window(const CutEntry* cuts, int32_t w, uint8_t* out, const int64_t* piece_off, const uint8_t* ivs, const int64_t* result,
                              int32_t tile0) {
  PassWindow p;
  p.out = out;
  p.E = piece_off + cuts[w].first_pp;
  p.ivs = ivs + kIvBytes * (size_t)cuts[w].first_piece;
  p.cut = result + (size_t)kCutWords * (size_t)w;
  p.n_pieces = cuts[w].n_pieces;
  p.tile0 = tile0;
  p.front = cuts[w].open_img;
  return p;
}

// tiles [tile0, tile0 + tiles) of the launch belong to window w -> the next window's tile0
inline int32_t map_tiles(int32_t* tile_win, int32_t tile0, int64_t tiles, int32_t w) {
  for (int64_t t = 0; t < tiles; t++) tile_win[tile0 + t] = w;
  return tile0 + (int32_t)tiles;
}

// The open partition's IV stays with the stream from the feed that took its first block until the partition closes.  st: the
// state behind the feed; front: open_img in front of it; feed_ivs: the IVs the feed ran with (entry 0 the carried one)
inline void wipe_iv(uint8_t* iv) {
  volatile uint8_t* v = iv;
  for (size_t i = 0; i < kIvBytes; i++) v[i] = 0;
}
inline void commit_iv(uint8_t* iv, const State& st, int64_t front, int32_t parts_closed, const uint8_t* feed_ivs) {
  if (st.open_img == 0) {
    wipe_iv(iv);
  } else if (parts_closed > 0 || front == 0) {
    for (size_t i = 0; i < kIvBytes; i++) iv[i] = feed_ivs[kIvBytes * (size_t)parts_closed + i];
  }
}
// ... behind a feed that wrote nothing (commit_nothing)
inline void commit_nothing_iv(uint8_t* iv, int32_t parts_closed) {
  if (parts_closed > 0) wipe_iv(iv);
}

// ---- behind the download ------------------------------------------------------------------------------------------------------
// The cut kernel's result words and the gather's status word of one feed, checked: false = "the capacity cut returned an
// impossible result" (S3S_E_HIP, nothing is committed).
inline bool cut_from_words(const int64_t* res, int32_t status_word, int64_t n_items, int64_t src_len, int64_t dst_capacity, int32_t n_ends,
                           Cut* c) {
  c->k = res[kCutK];
  c->consumed = res[kCutConsumed];
  c->out_len = res[kCutOutLen];
  c->need_dst = res[kCutNeedDst];
  c->parts_closed = (int32_t)res[kCutPartsClosed];
  return !(status_word != 0 || c->k < 0 || c->k > n_items || c->consumed < 0 || c->consumed > src_len || c->out_len < 0 ||
           c->out_len > dst_capacity || res[kCutPartsClosed] < 0 || res[kCutPartsClosed] > n_ends || c->need_dst < 0);
}

// The feed that took `c` (need_dst == 0): the lengths and checksums of the partitions it closed go to the caller, the open
// partition's checksum state and the stream's counters move.  piece_off[n_ends + 2]: the clamped piece offsets of the output;
// lengths: the cut kernel's (null: S3S_CODEC_NONE, they follow from piece_off); sums[n_ends + 1] (null: no checksums).
inline void commit(State* st, int64_t* carry, const Cut& c, const int64_t* ends, const int64_t* piece_off, const int64_t* lengths,
                   const int64_t* sums, int64_t* out_lengths, int64_t* out_checksums) {
  if (lengths) {
    for (int32_t j = 0; j < c.parts_closed; j++) out_lengths[j] = lengths[j];
  } else {
    closed_lengths(*st, c, piece_off, out_lengths);
  }
  if (sums) {
    for (int32_t j = 0; j < c.parts_closed; j++) out_checksums[j] = sums[j];
    *carry = sums[c.parts_closed];
  }
  advance(st, c, ends, piece_off);
}

// ---- the two ends of a feed, for the single feed and for every window of a batch ------------------------------------------------
// iv: the stream's carried IV (null: not under IO encryption); r: an s3s_cstream_result, zeroed.
// Answered on the host, nothing written (cut_nothing, or S3S_CODEC_NONE's cut with out_len 0):
template <typename Result>
inline void answer_on_host(State* st, int64_t* carry, uint8_t* iv, int64_t fresh, const Cut& c, int64_t* out_lengths, int64_t* out_checksums,
                           Result* r) {
  commit_nothing(st, carry, fresh, c.parts_closed, out_lengths, out_checksums);
  if (iv) commit_nothing_iv(iv, c.parts_closed);
  r->need_src = c.need_src;
  r->parts_closed = c.parts_closed;
}
// Behind the download, a cut that passed cut_from_words (or S3S_CODEC_NONE's).  false: S3S_E_CAPACITY - the first unit does not
// fit dst, r->need_dst says what does, nothing is taken and the stream stays usable.  feed_ivs: the IVs the feed ran with
template <typename Result>
inline bool take_window(State* st, int64_t* carry, uint8_t* iv, const Cut& c, const int64_t* ends, const int64_t* piece_off, const int64_t* lengths,
                        const int64_t* sums, const uint8_t* feed_ivs, int64_t* out_lengths, int64_t* out_checksums, Result* r) {
  if (c.need_dst > 0) {
    r->need_dst = c.need_dst;
    return false;
  }
  const State before = *st;
  commit(st, carry, c, ends, piece_off, lengths, sums, out_lengths, out_checksums);
  if (iv) commit_iv(iv, *st, before.open_img, c.parts_closed, feed_ivs);
  r->consumed = c.consumed;
  r->out_len = c.out_len;
  r->parts_closed = c.parts_closed;
  return true;
}

}  // namespace s3s_cs
