// cstream_batch_model.cpp — the host arithmetic of the batched feed of the streaming map side
// (spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h) as a stand-alone program: which entries are windows of the batch,
// their places in the call's packed arrays, the plan records and descriptors in ONE arena of exactly Arena::total bytes, and,
// behind the "download", the check of every window's words and the per-entry commit.  tests/test_compress_stream_batch_cpu.py
// builds it with -fsanitize=address,undefined, plays the kernels over a pipe (the scan, the cut, the clamped piece offsets, the
// lengths, the seeded checksums - from the plan this program prints, by the indices the descriptors hold) and compares every
// entry's answer and every stream's state with the Python model of the contract (tests/cstream_units.py).
//
// stdin:   codec bs fresh with_sums n_streams
//          rounds:  "R n", then n lines  stream addr src_len cap n_ends end...      (n_ends < 0: no ends follow)
// stdout:  per round with windows:  "P m N PP P L", m lines "W e first_item n_items first_pp n_pieces first_piece first_len
//          first_last ends0 cap open_img", "I" N x (src_off len kind piece), "M" N x (src_end last ends_after), "F" PP
//          part_first, "S" P seeds, "E" P piece -> window; then it READS one line: m status words, 8 m result words, PP piece
//          offsets, L lengths, P sums.  "X" = the words were impossible (S3S_E_HIP, nothing committed).
//          per entry:  "A status consumed out_len need_src need_dst parts_closed n length... sum... pos written open_bytes
//          open_img carry"
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
};
struct Entry {
  int stream;
  long long addr, src_len, cap;
  int n_ends;
  std::unique_ptr<int64_t[]> ends, lengths, sums;
  int status = -100;
  cs::Cut c;
  int window = -1;
};

static int64_t unit_items(int codec, const cs::Unit& u) { return codec == cs::kCodecSnappy ? u.first + 1 : 1; }

int main() {
  int codec, with_sums, n_streams;
  long long bs, fresh;
  if (scanf("%d %lld %lld %d %d", &codec, &bs, &fresh, &with_sums, &n_streams) != 5) return 2;
  std::unique_ptr<Stream[]> S(new Stream[(size_t)n_streams]);
  for (int i = 0; i < n_streams; i++) S[(size_t)i].carry = fresh;
  char tag[4];
  int n;
  while (scanf("%3s %d", tag, &n) == 2) {
    std::unique_ptr<Entry[]> E(new Entry[(size_t)n]);
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
    }
    // which entries are windows, and where
    cs::Totals tot;
    std::vector<cs::CutEntry> cuts;
    std::vector<int> win_entry;
    for (int i = 0; i < n; i++) {
      Entry& e = E[(size_t)i];
      Stream& s = S[(size_t)e.stream];
      if (cs::window_refused(e.src_len, e.ends.get(), e.n_ends, e.cap, false)) {
        e.status = -1;
        continue;
      }
      int64_t n_items = 0, n_slots = 0, n_units = 0;
      cs::plan_units(codec, bs, s.st.open_bytes, e.src_len, e.ends.get(), e.n_ends, [&](const cs::Unit& u) {
        n_items += unit_items(codec, u);
        n_slots += u.len > 0;
        n_units++;
      });
      if (n_items == 0) {  // answered on the host
        e.c = cs::Cut();
        e.c.parts_closed = e.n_ends;
        if (e.n_ends == 0) e.c.need_src = codec == cs::kCodecLzf ? cs::kLzfBlock : bs;
        cs::commit_nothing(&s.st, &s.carry, fresh, e.c.parts_closed, e.lengths.get(), with_sums ? e.sums.get() : nullptr);
        e.status = 0;
        continue;
      }
      if (!cs::fits_call(tot, n_items, n_slots, e.n_ends, 0)) return 3;
      e.window = tot.m;
      cuts.push_back(cs::reserve(&tot, n_items, n_slots, e.n_ends, 0, e.cap, s.st.open_img));
      win_entry.push_back(i);
    }
    const int m = tot.m;
    if (m > 0) {
      cs::Arena A;
      A.lay_out(tot, sizeof(MItem), sizeof(MTail));
      std::unique_ptr<uint8_t[]> arena(new uint8_t[A.total]);
      memset(arena.get(), 0x5a, A.total);
      MItem* items = reinterpret_cast<MItem*>(arena.get() + A.items);
      cs::Mark* marks = reinterpret_cast<cs::Mark*>(arena.get() + A.marks);
      int32_t* pf = reinterpret_cast<int32_t*>(arena.get() + A.pf);
      int64_t* seed = reinterpret_cast<int64_t*>(arena.get() + A.seed);
      int32_t* pw = reinterpret_cast<int32_t*>(arena.get() + A.pw);
      cs::CutEntry* d_cuts = reinterpret_cast<cs::CutEntry*>(arena.get() + A.cuts);
      const long long base = E[(size_t)win_entry[0]].addr;
      for (int wi = 0; wi < m; wi++) {
        Entry& e = E[(size_t)win_entry[(size_t)wi]];
        Stream& s = S[(size_t)e.stream];
        cs::CutEntry& c = cuts[(size_t)wi];
        const bool ok = cs::plan_entry(
            &c, codec, bs, s.st.open_bytes, e.src_len, e.ends.get(), e.n_ends, marks, pf, [&](const cs::Unit& u) { return unit_items(codec, u); },
            [&](const cs::Unit& u, int32_t at, int32_t& slot) {
              if (codec == cs::kCodecSnappy && u.first) items[at++] = MItem{0, 0, 2, -1, u.piece};
              if (u.len > 0) items[at] = MItem{cs::item_src_off(e.addr, base, u.src_off), u.len, 0, slot++, u.piece};
              else items[at] = MItem{0, 0, 1, -1, u.piece};
            });
        if (!ok) return 4;
        cs::seed_pieces(c, wi, s.carry, fresh, seed, pw);
        d_cuts[wi] = c;
      }
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
      fflush(stdout);
      // the "download": the down part of the arena, word for word
      int32_t* status = reinterpret_cast<int32_t*>(arena.get() + A.status);
      int64_t* res = reinterpret_cast<int64_t*>(arena.get() + A.res);
      int64_t* piece = reinterpret_cast<int64_t*>(arena.get() + A.piece);
      int64_t* len = reinterpret_cast<int64_t*>(arena.get() + A.len);
      int64_t* sums = reinterpret_cast<int64_t*>(arena.get() + A.sums);
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
      printf(" %lld %lld %lld %lld %lld\n", (long long)s.st.pos, (long long)s.st.written, (long long)s.st.open_bytes, (long long)s.st.open_img,
             (long long)s.carry);
    }
    fflush(stdout);
  }
  return 0;
}
