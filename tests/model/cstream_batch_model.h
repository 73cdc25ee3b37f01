// cstream_batch_model.h — the one body of tests/model/cstream_batch_model.cpp (run<false>) and
// tests/model/cstream_batch_encrypted_model.cpp (run<true>): a batched feed of the streaming map side played on the host with
// the functions of spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h that compress_stream.hip calls - window_refused,
// count_window, route_entry, cut_nothing / answer_on_host, fits_call / reserve, plan_entry_records, seed_pieces, slice_ivs,
// window_ivs, pass_tiles / pass_window / map_tiles, cut_from_words and take_window - in ONE arena of exactly Arena::total bytes.
// What is typed here is only what the library takes from s3s_ctx.h (the items of a unit) and the pipe protocol the two
// programs' head comments describe.
#pragma once
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "compress_stream_batch_core.h"

namespace cs = s3s_cs;

struct MItem {  // s3s::Item
  int64_t src_off;
  int32_t len, kind, slot, piece;
};
struct MTail {  // as large as s3s::TaskTail
  int64_t w[8];
};
struct MResult {  // s3s_cstream_result
  int64_t consumed = 0, out_len = 0, need_src = 0, need_dst = 0;
  int32_t parts_closed = 0;
};
struct Stream {
  cs::State st;
  int64_t carry;
  int epoch = 1;  // 1: the context's current key setting, 0: an earlier one
  uint8_t iv[16] = {};
};
struct Entry {
  int stream;
  long long addr, src_len, cap;
  int n_ends;
  std::unique_ptr<int64_t[]> ends, lengths, sums;
  int status = -100;
  MResult r;
  cs::Cut c;
};

constexpr long long kDstBias = 1ll << 44;  // an entry's d_dst, as a number

inline bool read_ll(long long* x) { return scanf("%lld", x) == 1; }

inline void print_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

template <bool kKeyed>
int run() {
  int codec, with_sums, n_streams;
  long long bs, fresh, x;
  if (scanf("%d %lld %lld %d %d", &codec, &bs, &fresh, &with_sums, &n_streams) != 5) return 2;
  std::unique_ptr<Stream[]> S(new Stream[(size_t)n_streams]);
  for (int i = 0; i < n_streams; i++) {
    S[(size_t)i].carry = fresh;
    if (kKeyed && scanf("%d", &S[(size_t)i].epoch) != 1) return 2;
  }
  const auto items_of = [&](const cs::Unit& u) { return codec == cs::kCodecSnappy ? u.first + 1 : 1; };
  const auto slots_of = [](const cs::Unit& u) { return u.len > 0; };
  char tag[4];
  int n, n_ivs = 0;
  while (scanf("%3s %d", tag, &n) == 2) {
    std::vector<uint8_t> call_ivs(1);
    if (kKeyed) {
      if (scanf("%d", &n_ivs) != 1) return 2;
      call_ivs.resize((size_t)(n_ivs > 0 ? n_ivs : 0) * 16 + 1);
      for (size_t i = 0; i < (size_t)(n_ivs > 0 ? n_ivs : 0) * 16; i++) {
        unsigned b;
        if (scanf("%2x", &b) != 1) return 2;
        call_ivs[i] = (uint8_t)b;
      }
      char dash[4];
      if (n_ivs <= 0 && scanf("%3s", dash) != 1) return 2;
    }
    std::unique_ptr<Entry[]> E(new Entry[(size_t)n]);
    for (int i = 0; i < n; i++) {
      Entry& e = E[(size_t)i];
      if (scanf("%d %lld %lld %lld %d", &e.stream, &e.addr, &e.src_len, &e.cap, &e.n_ends) != 5) return 2;
      const size_t ne = e.n_ends > 0 ? (size_t)e.n_ends : 0;
      e.ends.reset(new int64_t[ne]);
      e.lengths.reset(new int64_t[ne]);
      e.sums.reset(new int64_t[ne]);
      for (size_t j = 0; j < ne; j++) {
        if (!read_ll(&x)) return 2;
        e.ends[j] = x;
      }
    }
    // the call's IVs, sliced in entry order; then which entries are windows, and where
    std::unique_ptr<int64_t[]> iv_at(new int64_t[(size_t)n + 1]);
    const bool refused_call = kKeyed && cs::slice_ivs(n, [&](int32_t i) { return E[(size_t)i].n_ends; }, iv_at.get()) != n_ivs;
    if (refused_call) printf("V\n");
    cs::Totals tot;
    std::vector<cs::CutEntry> cuts;
    std::vector<int> win_entry;
    std::vector<int64_t> win_tiles;
    int64_t tiles = 0;
    for (int i = 0; i < n && !refused_call; i++) {
      Entry& e = E[(size_t)i];
      Stream& s = S[(size_t)e.stream];
      const bool refused = s.epoch != 1 || cs::window_refused(e.src_len, e.ends.get(), e.n_ends, e.cap, false);  // (a stale key setting: S3S_E_INVALID)
      const cs::Count cnt = refused ? cs::Count() : cs::count_window(codec, bs, s.st.open_bytes, e.src_len, e.ends.get(), e.n_ends, kKeyed, items_of, slots_of);
      switch (cs::route_entry(refused, cnt, 0)) {
        case cs::kRouteRefused:
          e.status = -1;
          break;
        case cs::kRouteHost:  // (its slice of IVs is consumed all the same)
          if (cnt.items != 0) return 3;
          cs::answer_on_host(&s.st, &s.carry, kKeyed ? s.iv : nullptr, fresh, cs::cut_nothing(e.n_ends, codec == cs::kCodecLzf ? cs::kLzfBlock : bs),
                             e.lengths.get(), with_sums ? e.sums.get() : nullptr, &e.r);
          e.status = 0;
          break;
        case cs::kRouteWindow:
          if (!cs::fits_call(tot, cnt.items, cnt.slots, e.n_ends, 0)) return 3;
          cuts.push_back(cs::reserve(&tot, cnt.items, cnt.slots, e.n_ends, 0, e.cap, s.st.open_img));
          win_entry.push_back(i);
          win_tiles.push_back(kKeyed ? cs::pass_tiles(e.cap, cs::feed_bound_encrypted(codec, bs, e.src_len, e.n_ends), s.st.open_img) : 0);
          tiles += win_tiles.back();
      }
    }
    const int m = tot.m;
    if (m > 0) {
      cs::Arena A;
      if (kKeyed) A.lay_out_encrypted(tot, sizeof(MItem), sizeof(MTail), sizeof(cs::PassWindow), tiles);
      else A.lay_out(tot, sizeof(MItem), sizeof(MTail));
      std::unique_ptr<uint8_t[]> arena(new uint8_t[A.total]);
      memset(arena.get(), 0x5a, A.total);
      MItem* items = reinterpret_cast<MItem*>(arena.get() + A.items);
      cs::Mark* marks = reinterpret_cast<cs::Mark*>(arena.get() + A.marks);
      int32_t* pf = reinterpret_cast<int32_t*>(arena.get() + A.pf);
      int64_t* seed = reinterpret_cast<int64_t*>(arena.get() + A.seed);
      int32_t* pw = reinterpret_cast<int32_t*>(arena.get() + A.pw);
      cs::CutEntry* d_cuts = reinterpret_cast<cs::CutEntry*>(arena.get() + A.cuts);
      uint8_t* ivs = arena.get() + A.ivs;
      cs::PassWindow* wins = reinterpret_cast<cs::PassWindow*>(arena.get() + A.wins);
      int32_t* tile_win = reinterpret_cast<int32_t*>(arena.get() + A.tile_win);
      int32_t* status = reinterpret_cast<int32_t*>(arena.get() + A.status);
      int64_t* res = reinterpret_cast<int64_t*>(arena.get() + A.res);
      int64_t* piece = reinterpret_cast<int64_t*>(arena.get() + A.piece);
      int64_t* len = reinterpret_cast<int64_t*>(arena.get() + A.len);
      int64_t* sums = reinterpret_cast<int64_t*>(arena.get() + A.sums);
      const long long base = E[(size_t)win_entry[0]].addr;
      for (int wi = 0; wi < m; wi++) {
        Entry& e = E[(size_t)win_entry[(size_t)wi]];
        Stream& s = S[(size_t)e.stream];
        cs::CutEntry& c = cuts[(size_t)wi];
        const bool ok = cs::plan_entry_records(
            &c, codec, bs, s.st.open_bytes, e.src_len, e.ends.get(), e.n_ends, marks, pf, kKeyed, items_of,
            [&](const cs::Unit& u, int32_t at) { items[at] = MItem{0, 0, 2, -1, u.piece}; },  // (an IV record prints as kind 2: sixteen bytes without a slot)
            [&](const cs::Unit& u, int32_t at, int32_t& slot) {
              if (codec == cs::kCodecSnappy && u.first) items[at++] = MItem{0, 0, 2, -1, u.piece};
              if (u.len > 0) items[at] = MItem{cs::item_src_off(e.addr, base, u.src_off), u.len, 0, slot++, u.piece};
              else items[at] = MItem{0, 0, 1, -1, u.piece};
            });
        if (!ok) return 4;
        cs::seed_pieces(c, wi, s.carry, fresh, seed, pw);
        if (kKeyed) cs::window_ivs(c, call_ivs.data() + 16 * (size_t)iv_at[(size_t)win_entry[(size_t)wi]], 0, s.iv, ivs);
        d_cuts[wi] = c;
      }
      int32_t tile0 = 0;
      for (int wi = 0; wi < m && kKeyed; wi++) {
        wins[wi] = cs::pass_window(d_cuts, wi, reinterpret_cast<uint8_t*>((intptr_t)(E[(size_t)win_entry[(size_t)wi]].addr + kDstBias)), piece, ivs, res, tile0);
        tile0 = cs::map_tiles(tile_win, tile0, win_tiles[(size_t)wi], wi);
      }
      if (tile0 != tiles) return 5;
      printf("P %d %lld %lld %lld %lld\n", m, (long long)tot.items, (long long)tot.pp(), (long long)tot.pieces, (long long)tot.lens());
      for (int wi = 0; wi < m; wi++) {
        const cs::CutEntry& c = d_cuts[wi];
        printf("W %d %d %d %d %d %d %d %d %d %lld %lld\n", win_entry[(size_t)wi], c.first_item, c.n_items, c.first_pp, c.n_pieces, c.first_piece,
               c.first_len, c.first_last, c.ends0, (long long)c.dst_capacity, (long long)c.open_img);
      }
      printf("I");
      for (int64_t i = 0; i < tot.items; i++) printf(" %lld %d %d %d", (long long)items[i].src_off, items[i].len, items[i].kind, items[i].piece);
      printf("\nM");
      for (int64_t i = 0; i < tot.items; i++) printf(" %lld %d %d", (long long)marks[i].src_end, marks[i].last, marks[i].ends_after);
      printf("\nF");
      for (int64_t i = 0; i < tot.pp(); i++) printf(" %d", pf[i]);
      printf("\nS");
      for (int64_t i = 0; i < tot.pieces; i++) printf(" %lld", (long long)seed[i]);
      printf("\nE");
      for (int64_t i = 0; i < tot.pieces; i++) printf(" %d", pw[i]);
      printf("\n");
      if (kKeyed) {
        printf("T %lld\n", (long long)tiles);
        for (int wi = 0; wi < m; wi++) {
          const cs::PassWindow& w = wins[wi];
          printf("D %lld %lld %lld %d %d %lld %lld\n", (long long)(w.E - piece), (long long)((w.ivs - ivs) / 16), (long long)(w.cut - res), w.n_pieces,
                 w.tile0, (long long)w.front, (long long)reinterpret_cast<intptr_t>(w.out));
        }
        printf("Q");
        for (int64_t i = 0; i < tiles; i++) printf(" %d", tile_win[i]);
        printf("\nH ");
        print_hex(ivs, 16 * (size_t)tot.pieces);
        printf("\n");
      }
      fflush(stdout);
      // the "download": the down part of the arena, word for word
      for (int i = 0; i < m; i++) { if (!read_ll(&x)) return 2; status[i] = (int32_t)x; }
      for (int i = 0; i < cs::kCutWords * m; i++) { if (!read_ll(&x)) return 2; res[i] = x; }
      for (int64_t i = 0; i < tot.pp(); i++) { if (!read_ll(&x)) return 2; piece[i] = x; }
      for (int64_t i = 0; i < tot.lens(); i++) { if (!read_ll(&x)) return 2; len[i] = x; }
      for (int64_t i = 0; i < tot.pieces; i++) { if (!read_ll(&x)) return 2; sums[i] = x; }
      bool possible = true;  // every window's words are checked before any stream moves
      for (int wi = 0; wi < m; wi++) {
        Entry& e = E[(size_t)win_entry[(size_t)wi]];
        possible = possible && cs::cut_from_words(res + cs::kCutWords * wi, status[wi], d_cuts[wi].n_items, e.src_len, e.cap, e.n_ends, &e.c);
      }
      if (!possible) {
        printf("X\n");
        fflush(stdout);
        continue;
      }
      for (int wi = 0; wi < m; wi++) {
        Entry& e = E[(size_t)win_entry[(size_t)wi]];
        Stream& s = S[(size_t)e.stream];
        const cs::CutEntry& c = d_cuts[wi];
        e.status = cs::take_window(&s.st, &s.carry, kKeyed ? s.iv : nullptr, e.c, e.ends.get(), piece + c.first_pp, len + c.first_len,
                                   with_sums ? sums + c.first_piece : nullptr, ivs + 16 * (size_t)c.first_piece, e.lengths.get(), e.sums.get(), &e.r)
                       ? 0
                       : -2;
      }
    }
    for (int i = 0; i < n; i++) {
      const Entry& e = E[(size_t)i];
      const Stream& s = S[(size_t)e.stream];
      const int closed = e.r.parts_closed;
      printf("A %d %lld %lld %lld %lld %d %d", e.status, (long long)e.r.consumed, (long long)e.r.out_len, (long long)e.r.need_src, (long long)e.r.need_dst,
             closed, closed);
      for (int j = 0; j < closed; j++) printf(" %lld", (long long)e.lengths[(size_t)j]);
      if (with_sums)
        for (int j = 0; j < closed; j++) printf(" %lld", (long long)e.sums[(size_t)j]);
      printf(" %lld %lld %lld %lld %lld", (long long)s.st.pos, (long long)s.st.written, (long long)s.st.open_bytes, (long long)s.st.open_img,
             (long long)s.carry);
      if (kKeyed) {
        printf(" ");
        print_hex(s.iv, 16);
      }
      printf("\n");
    }
    fflush(stdout);
  }
  return 0;
}
