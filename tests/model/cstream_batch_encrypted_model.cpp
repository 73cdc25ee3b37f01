// cstream_batch_encrypted_model.cpp — the host arithmetic of the batched feed of the streaming map side UNDER IO ENCRYPTION
// (spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h) as a stand-alone program: the slices of the call's
// IVs, which entries are windows of the batch, the plan records WITH IV records, the IVs, the pass descriptors and the
// tile -> window map in ONE arena of exactly Arena::total bytes, and, behind the "download", the check of every window's
// words and the per-entry commit with the IV bookkeeping.  tests/test_compress_stream_batch_encrypted_cpu.py builds it with
// -fsanitize=address,undefined, plays the kernels over a pipe - the encrypt pass from the descriptors and the map this
// program prints - and compares every entry's answer and every stream's state, its IV included, with the Python model of the
// contract (tests/cstream_units_encrypted.py).  The protocol is tests/model/cstream_batch_model.cpp's, extended.
//
// stdin:   codec bs fresh with_sums n_streams, then n_streams epochs (1: the context's current key setting, 0: an earlier one)
//          rounds:  "R n n_ivs", n_ivs x 32 hex digits (or "-"), then n lines  stream addr src_len cap n_ends end...
// stdout:  "V" = the IV count is not the sum of the slices (S3S_E_INVALID for the call, every stream unchanged);
//          per round with windows:  "P m N PP P L", m lines "W ..." and "I", "M", "F", "S", "E" as in cstream_batch_model.cpp (an
//          IV record prints as kind 2: sixteen bytes without a slot), then "T tiles", m lines "D E ivs cut n_pieces tile0 front
//          out" (E / ivs / cut: the element the pointer names in the call's piece offsets / IVs / result words), "Q" the
//          tile -> window map, "H" the call's IVs in hex; then it READS the downloaded words.  "X" = impossible words.
//          per entry:  "A status consumed out_len need_src need_dst parts_closed n length... sum... pos written open_bytes
//          open_img carry iv"
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
struct Stream {
  cs::State st;
  int64_t carry;
  int epoch;
  uint8_t iv[16];
};
struct Entry {
  int stream;
  long long addr, src_len, cap;
  int n_ends;
  std::unique_ptr<int64_t[]> ends, lengths, sums;
  int status = -100;
  cs::Cut c;
  int window = -1;
  int64_t iv_at = 0;
};

constexpr long long kDstBias = 1ll << 44;  // an entry's d_dst, as a number

static int64_t unit_items(int codec, const cs::Unit& u) { return codec == cs::kCodecSnappy ? u.first + 1 : 1; }

static void print_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

int main() {
  int codec, with_sums, n_streams;
  long long bs, fresh;
  if (scanf("%d %lld %lld %d %d", &codec, &bs, &fresh, &with_sums, &n_streams) != 5) return 2;
  std::unique_ptr<Stream[]> S(new Stream[(size_t)n_streams]);
  for (int i = 0; i < n_streams; i++) {
    S[(size_t)i].carry = fresh;
    memset(S[(size_t)i].iv, 0, 16);
    if (scanf("%d", &S[(size_t)i].epoch) != 1) return 2;
  }
  char tag[4];
  int n, n_ivs;
  while (scanf("%3s %d %d", tag, &n, &n_ivs) == 3) {
    std::vector<uint8_t> call_ivs((size_t)(n_ivs > 0 ? n_ivs : 0) * 16 + 1);
    if (n_ivs > 0) {
      for (size_t i = 0; i < (size_t)n_ivs * 16; i++) {
        unsigned x;
        if (scanf("%2x", &x) != 1) return 2;
        call_ivs[i] = (uint8_t)x;
      }
    } else {
      char dash[4];
      if (scanf("%3s", dash) != 1) return 2;
    }
    std::unique_ptr<Entry[]> E(new Entry[(size_t)n]);
    int64_t want_ivs = 0;
    for (int i = 0; i < n; i++) {
      Entry& e = E[(size_t)i];
      if (scanf("%d %lld %lld %lld %d", &e.stream, &e.addr, &e.src_len, &e.cap, &e.n_ends) != 5) return 2;
      const size_t ne = e.n_ends > 0 ? (size_t)e.n_ends : 0;
      e.ends.reset(new int64_t[ne]);
      e.lengths.reset(new int64_t[ne]);
      e.sums.reset(new int64_t[ne]);
      for (size_t j = 0; j < ne; j++) {
        long long x;
        if (scanf("%lld", &x) != 1) return 2;
        e.ends[j] = x;
      }
      want_ivs += cs::iv_slice_len(e.n_ends);
    }
    cs::Totals tot;
    std::vector<cs::CutEntry> cuts;
    std::vector<int> win_entry;
    std::vector<int64_t> win_tiles;
    int64_t tiles = 0;
    const bool refused_call = want_ivs != n_ivs;
    if (refused_call) printf("V\n");
    cs::IvSlicer slices;
    for (int i = 0; i < n && !refused_call; i++) {
      Entry& e = E[(size_t)i];
      Stream& s = S[(size_t)e.stream];
      e.iv_at = slices.take(e.n_ends);
      if (s.epoch != 1) {  // bound to an earlier key setting: the single feed's S3S_E_INVALID
        e.status = -1;
        continue;
      }
      if (cs::window_refused(e.src_len, e.ends.get(), e.n_ends, e.cap, false)) {
        e.status = -1;
        continue;
      }
      int64_t n_items = 0, n_slots = 0;
      cs::plan_units(codec, bs, s.st.open_bytes, e.src_len, e.ends.get(), e.n_ends, [&](const cs::Unit& u) {
        n_items += cs::iv_records(u, true) + unit_items(codec, u);
        n_slots += u.len > 0;
      });
      if (n_items == 0) {  // answered on the host; its slice of IVs is consumed all the same
        e.c = cs::Cut();
        e.c.parts_closed = e.n_ends;
        if (e.n_ends == 0) e.c.need_src = codec == cs::kCodecLzf ? cs::kLzfBlock : bs;
        cs::commit_nothing(&s.st, &s.carry, fresh, e.c.parts_closed, e.lengths.get(), with_sums ? e.sums.get() : nullptr);
        cs::commit_nothing_iv(s.iv, e.c.parts_closed);
        e.status = 0;
        continue;
      }
      if (!cs::fits_call(tot, n_items, n_slots, e.n_ends, 0)) return 3;
      e.window = tot.m;
      cuts.push_back(cs::reserve(&tot, n_items, n_slots, e.n_ends, 0, e.cap, s.st.open_img));
      win_entry.push_back(i);
      win_tiles.push_back(cs::pass_tiles(e.cap, cs::feed_bound_encrypted(codec, bs, e.src_len, e.n_ends), s.st.open_img));
      tiles += win_tiles.back();
    }
    const int m = tot.m;
    if (m > 0) {
      cs::Arena A;
      A.lay_out_encrypted(tot, sizeof(MItem), sizeof(MTail), sizeof(cs::PassWindow), tiles);
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
        const bool ok = cs::plan_entry_encrypted(
            &c, codec, bs, s.st.open_bytes, e.src_len, e.ends.get(), e.n_ends, marks, pf, [&](const cs::Unit& u) { return unit_items(codec, u); },
            [&](const cs::Unit& u, int32_t at) { items[at] = MItem{0, 0, 2, -1, u.piece}; },
            [&](const cs::Unit& u, int32_t at, int32_t& slot) {
              if (codec == cs::kCodecSnappy && u.first) items[at++] = MItem{0, 0, 2, -1, u.piece};
              if (u.len > 0) items[at] = MItem{cs::item_src_off(e.addr, base, u.src_off), u.len, 0, slot++, u.piece};
              else items[at] = MItem{0, 0, 1, -1, u.piece};
            });
        if (!ok) return 4;
        cs::seed_pieces(c, wi, s.carry, fresh, seed, pw);
        cs::window_ivs(c, call_ivs.data(), e.iv_at, s.iv, ivs);
        d_cuts[wi] = c;
      }
      int32_t tile0 = 0;
      for (int wi = 0; wi < m; wi++) {
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
      printf("\nT %lld\n", (long long)tiles);
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
      fflush(stdout);
      // the "download": the down part of the arena, word for word
      auto rd = [](long long* x) { return scanf("%lld", x) == 1; };
      long long x;
      for (int i = 0; i < m; i++) { if (!rd(&x)) return 2; status[i] = (int32_t)x; }
      for (int i = 0; i < cs::kCutWords * m; i++) { if (!rd(&x)) return 2; res[i] = x; }
      for (int64_t i = 0; i < tot.pp(); i++) { if (!rd(&x)) return 2; piece[i] = x; }
      for (int64_t i = 0; i < tot.lens(); i++) { if (!rd(&x)) return 2; len[i] = x; }
      for (int64_t i = 0; i < tot.pieces; i++) { if (!rd(&x)) return 2; sums[i] = x; }
      bool possible = true;
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
        if (e.c.need_dst > 0) {
          e.status = -2;
          continue;
        }
        cs::commit(&s.st, &s.carry, e.c, e.ends.get(), piece + c.first_pp, len + c.first_len, with_sums ? sums + c.first_piece : nullptr,
                   e.lengths.get(), e.sums.get());
        cs::commit_iv(s.iv, s.st, c.open_img, e.c.parts_closed, ivs + 16 * (size_t)c.first_piece);
        e.status = 0;
      }
    }
    for (int i = 0; i < n; i++) {
      const Entry& e = E[(size_t)i];
      const Stream& s = S[(size_t)e.stream];
      const bool ok = e.status == 0;
      const int closed = ok ? e.c.parts_closed : 0;
      printf("A %d %lld %lld %lld %lld %d %d", e.status, ok ? (long long)e.c.consumed : 0, ok ? (long long)e.c.out_len : 0,
             ok ? (long long)e.c.need_src : 0, e.status == -2 ? (long long)e.c.need_dst : 0, closed, closed);
      for (int j = 0; j < closed; j++) printf(" %lld", (long long)e.lengths[(size_t)j]);
      if (with_sums)
        for (int j = 0; j < closed; j++) printf(" %lld", (long long)e.sums[(size_t)j]);
      printf(" %lld %lld %lld %lld %lld ", (long long)s.st.pos, (long long)s.st.written, (long long)s.st.open_bytes, (long long)s.st.open_img,
             (long long)s.carry);
      print_hex(s.iv, 16);
      printf("\n");
    }
    fflush(stdout);
  }
  return 0;
}
