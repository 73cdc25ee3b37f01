// compress_stream_batch_core.h — the arithmetic of the batched feed of the streaming map side (s3s_cstream_feed_batch*,
// compress_stream.hip): where the windows of several streams lie in ONE plan, what the device is told about each of them, and
// how a stream's host state moves once the call's one download has come back.  No HIP in here: the file builds for the host
// alone (tests/model/cstream_batch_model.cpp runs it under the sanitizers against the Python model of the contract,
// tests/cstream_units.py) and for the device (cstream_cut_batch_kernel and gather_items_cut_batch_kernel,
// compress_stream_batch_kernels.hip, read CutEntry).  commit() is the single feed's commit step too.
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

// The call's small arrays in one block, laid out alike in the pinned staging area and in device memory: [0, up) goes up in one
// copy in front of the kernels, [up, total) is zeroed on the device, written by the kernels and comes down in one copy.
struct Arena {
  size_t items = 0, marks = 0, pf = 0, seg = 0, seed = 0, pw = 0, tails = 0, cuts = 0, up = 0;
  size_t status = 0, res = 0, piece = 0, len = 0, sums = 0, total = 0;
  void lay_out(const Totals& t, size_t item_bytes, size_t tail_bytes) {
    const size_t N = (size_t)t.items, PP = (size_t)t.pp(), P = (size_t)t.pieces, L = (size_t)t.lens(), M = (size_t)t.m;
    items = 0;
    marks = arena_al(items + item_bytes * N);
    pf = arena_al(marks + sizeof(Mark) * N);
    seg = arena_al(pf + 4 * PP);
    seed = arena_al(seg + 4 * PP);
    pw = arena_al(seed + 8 * P);
    tails = arena_al(pw + 4 * P);
    cuts = arena_al(tails + tail_bytes * M);
    up = arena_al(cuts + sizeof(CutEntry) * M);
    status = up;
    res = arena_al(status + 4 * M);
    piece = arena_al(res + 8 * (size_t)kCutWords * M);
    len = arena_al(piece + 8 * PP);
    sums = arena_al(len + 8 * L);
    total = arena_al(sums + 8 * P);
  }
};

// The plan records of one entry, written into the call's arrays: the single feed's loop (compress_stream.hip) with the entry's
// places added.  items_of(u) = the plan items of unit u; emit(u, at, slot) writes them at item `at` of the CALL (slot: the
// call's slot counter, advanced) with src_off = src_delta + the unit's offset.  marks / part_first: the call's arrays.
// false: the plan does not match the counts the entry was reserved with (nothing may be launched).
template <typename ItemsOf, typename Emit>
inline bool plan_entry(CutEntry* c, int codec, int64_t bs, int64_t open_bytes, int64_t src_len, const int64_t* ends, int32_t n_ends,
                       Mark* marks, int32_t* part_first, ItemsOf&& items_of, Emit&& emit) {
  Mark* m = marks + c->first_item;
  int32_t* pf = part_first + c->first_pp;
  const int32_t n_items = c->n_items, n_pieces = c->n_pieces;
  int32_t it = 0, slot = c->first_slot, piece = 0, prev0 = 0;
  bool fits = true;
  pf[0] = 0;
  plan_units(codec, bs, open_bytes, src_len, ends, n_ends, [&](const Unit& u) {
    const int64_t mine = items_of(u);
    if (!fits || it + mine > n_items) {
      fits = false;
      return;
    }
    mark_ends_after(m, prev0, it, u.ends_before);
    if (it == 0) c->ends0 = u.ends_before;
    while (piece < u.piece) pf[++piece] = it;
    prev0 = it;
    emit(u, c->first_item + it, slot);
    it += (int32_t)mine;
    mark_unit(m, prev0, it, u, n_ends);
    if (c->first_last < 0) c->first_last = it - 1;
  });
  while (piece < n_pieces) pf[++piece] = it;
  return fits && it == n_items && slot == c->first_slot + c->n_slots;
}

// the seeds of an entry's pieces: the stream's carried state continues into the first, a fresh state starts the others
inline void seed_pieces(const CutEntry& c, int32_t entry, int64_t carry, int64_t fresh, int64_t* seeds, int32_t* piece_entry) {
  for (int32_t j = 0; j < c.n_pieces; j++) {
    seeds[c.first_piece + j] = j == 0 ? carry : fresh;
    piece_entry[c.first_piece + j] = entry;
  }
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

}  // namespace s3s_cs
