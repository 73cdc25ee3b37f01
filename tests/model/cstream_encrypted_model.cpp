// cstream_encrypted_model.cpp — the host side of the streaming map side under IO encryption as a stand-alone program: TEST
// INFRASTRUCTURE.  tests/test_compress_stream_encrypted_cpu.py builds it with -fsanitize=address,undefined; every array has
// exactly the size in use, so that an index one too far is a sanitizer report.
//
//   plan   the arithmetic of spark-s3-shuffle_amd/csrc/compress_stream_core.h and, as the single feed calls it for a batch of one,
//          compress_stream_batch_core.h: a window's count and its plan with IV records (count_window, plan_entry_encrypted), the
//          empty window and the take step, the cut over the marks as cstream_cut_kernel makes it (cut_lane), the encrypted NONE cut
//          (none_cut_encrypted), feed_bound_encrypted and the stream's state, driven by a schedule of feeds and the PLAIN image
//          sizes of a map output's units; compared field for field with the Python model (tests/cstream_units_encrypted.py).
//            stdin:   codec bs nparts / nparts lines: n_units size... / feeds, one a line: src_len cap n_ends end...
//            stdout:  one line a feed: code consumed out_len need_src need_dst parts_closed bound length...
//   own    the ownership of aes_ctr_stream_core.h in the map-side geometry: walks the chunks of one feed's output exactly as
//          aes_ctr_cstream_kernel does (win_open / win_next), applies every unit with the host build of aes_ctr_core.h, in place
//          on a buffer of exactly out_len bytes and from plain, and counts how often every stored byte was touched.
//            cases file: u32 count, then per case  u32 key_bytes | key | i32 n | i64 front | i64 tile_chunks | E[n + 1] | Q[n + 1] |
//                        ivs[16 n] | i64 src_len | src | holed[E[n]]
//            output per case: in place[E[n]] | from plain[E[n]] | cover[E[n]]
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/aes_ctr_stream_core.h"
#include "../../spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h"

namespace {

struct Result {  // s3s_cstream_result
  int64_t consumed = 0, out_len = 0, need_src = 0, need_dst = 0;
  int32_t parts_closed = 0;
};

int run_plan() {
  int codec = 0, nparts = 0;
  long long bs = 0;
  if (scanf("%d %lld %d", &codec, &bs, &nparts) != 3) return 2;
  std::vector<std::unique_ptr<int64_t[]>> sizes((size_t)nparts);
  std::vector<int64_t> n_sizes((size_t)nparts);
  for (int p = 0; p < nparts; p++) {
    long long n = 0;
    if (scanf("%lld", &n) != 1) return 2;
    n_sizes[(size_t)p] = n;
    sizes[(size_t)p].reset(new int64_t[(size_t)n]);
    for (long long i = 0; i < n; i++) {
      long long x;
      if (scanf("%lld", &x) != 1) return 2;
      sizes[(size_t)p][(size_t)i] = x;
    }
  }
  s3s_cs::State st;
  int64_t n_closed = 0, carry = 0;
  uint8_t iv[16] = {};
  long long src_len, cap;
  int n_ends;
  while (scanf("%lld %lld %d", &src_len, &cap, &n_ends) == 3) {
    std::unique_ptr<int64_t[]> ends(new int64_t[(size_t)n_ends]);
    for (int j = 0; j < n_ends; j++) {
      long long e;
      if (scanf("%lld", &e) != 1) return 2;
      ends[(size_t)j] = e;
    }
    if (!s3s_cs::ends_valid(src_len, ends.get(), n_ends)) {
      printf("-1 0 0 0 0 0 0\n");
      continue;
    }
    const int64_t unit_bs = codec == s3s_cs::kCodecNone ? 1 : bs;
    const long long bound = s3s_cs::feed_bound_encrypted(codec, unit_bs, src_len, n_ends);
    const int n_pieces = n_ends + 1;
    s3s_cs::Cut c;
    std::unique_ptr<int64_t[]> piece_off(new int64_t[(size_t)n_pieces + 1]);
    if (codec == s3s_cs::kCodecNone) {
      const s3s_cs::Cut counted = s3s_cs::none_cut_encrypted(st.open_img, src_len, ends.get(), n_ends, cap, nullptr);
      c = s3s_cs::none_cut_encrypted(st.open_img, src_len, ends.get(), n_ends, cap, piece_off.get());
      if (counted.consumed != c.consumed || counted.out_len != c.out_len || counted.need_dst != c.need_dst || counted.parts_closed != c.parts_closed)
        return 4;
    } else {
      // count, then build - the single feed's batch of one: the records of every unit (an IV record in front of a partition's
      // first block, a Snappy header, the block itself), their marks and the first record of every piece; here with their image sizes
      const auto items_of = [&](const s3s_cs::Unit& u) { return (codec == s3s_cs::kCodecSnappy && u.first) + 1; };
      const s3s_cs::Count cnt = s3s_cs::count_window(codec, bs, st.open_bytes, src_len, ends.get(), n_ends, true, items_of,
                                                     [](const s3s_cs::Unit& u) { return u.len > 0; });
      const int64_t n_items = cnt.items;
      s3s_cs::Totals tot;
      s3s_cs::CutEntry plan = s3s_cs::reserve(&tot, cnt.items, cnt.slots, n_ends, 0, cap, st.open_img);
      std::unique_ptr<s3s_cs::Mark[]> marks(new s3s_cs::Mark[(size_t)n_items]);
      std::unique_ptr<int64_t[]> size(new int64_t[(size_t)n_items]), item_off(new int64_t[(size_t)n_items + 1]);
      std::unique_ptr<int32_t[]> part_first(new int32_t[(size_t)n_pieces + 1]);
      const bool planned = s3s_cs::plan_entry_encrypted(
          &plan, codec, bs, st.open_bytes, src_len, ends.get(), n_ends, marks.get(), part_first.get(), items_of,
          [&](const s3s_cs::Unit&, int32_t at) { size[(size_t)at] = 16; },
          [&](const s3s_cs::Unit& u, int32_t at, int32_t& slot) {
            const int64_t part = n_closed + u.piece;
            const int64_t piece_start = u.piece == 0 ? 0 : ends[(size_t)u.piece - 1];
            const int64_t had = u.piece == 0 ? st.open_bytes : 0;
            const int64_t idx = u.len > 0 ? (had + u.src_off - piece_start) / bs : n_sizes[(size_t)part] - 1;
            int64_t body = sizes[(size_t)part][(size_t)idx];
            if (codec == s3s_cs::kCodecSnappy && u.first) {
              size[(size_t)at++] = 16;
              body -= 16;
            }
            size[(size_t)at] = body;
            slot += u.len > 0;
          });
      if (!planned) return 4;
      item_off[0] = 0;
      for (int64_t i = 0; i < n_items; i++) item_off[(size_t)i + 1] = item_off[(size_t)i] + size[(size_t)i];
      const int32_t first_last = plan.first_last, ends0 = plan.ends0;
      if (n_items == 0) {
        c = s3s_cs::cut_nothing(n_ends, codec == s3s_cs::kCodecLzf ? s3s_cs::kLzfBlock : bs);
        for (int j = 0; j <= n_pieces; j++) piece_off[(size_t)j] = 0;
      } else {  // cstream_cut_kernel, serially
        int32_t best = -1;
        for (int32_t i = 0; i < n_items; i++)
          if (s3s_cs::cut_lane(marks[(size_t)i], item_off[(size_t)i + 1], cap)) best = i;
        c.k = best + 1;
        c.out_len = item_off[(size_t)c.k];
        c.consumed = best >= 0 ? marks[(size_t)best].src_end : 0;
        c.parts_closed = best >= 0 ? marks[(size_t)best].ends_after : ends0;
        c.need_dst = best < 0 && first_last >= 0 && ends0 == 0 ? item_off[(size_t)first_last + 1] : 0;
        for (int j = 0; j <= n_pieces; j++) {
          const int64_t o = item_off[(size_t)part_first[(size_t)j]];
          piece_off[(size_t)j] = o < c.out_len ? o : c.out_len;
        }
      }
    }
    std::unique_ptr<int64_t[]> lengths(new int64_t[(size_t)c.parts_closed]);
    std::unique_ptr<uint8_t[]> feed_ivs(new uint8_t[16 * (size_t)n_pieces]());
    Result r;
    if (!s3s_cs::take_window(&st, &carry, iv, c, ends.get(), piece_off.get(), nullptr, nullptr, feed_ivs.get(), lengths.get(), nullptr, &r)) {
      printf("-2 0 0 0 %lld 0 %lld\n", (long long)r.need_dst, bound);
      continue;
    }
    n_closed += r.parts_closed;
    printf("0 %lld %lld %lld 0 %d %lld", (long long)r.consumed, (long long)r.out_len, (long long)c.need_src, (int)r.parts_closed, bound);
    for (int j = 0; j < r.parts_closed; j++) printf(" %lld", (long long)lengths[(size_t)j]);
    printf("\n");
  }
  return 0;
}

// one feed's output, walked as aes_ctr_cstream_kernel walks it.  from_plain: src -> out; else out in place.
void walk(const uint32_t* rk, int nr, const uint8_t* ivs, const uint8_t* src, const int64_t* E, const int64_t* Q, int32_t n, int64_t front,
          int64_t tile_chunks, bool from_plain, uint8_t* out, uint8_t* cover) {
  using namespace s3s_aes;
  const int64_t L = E[n];
  const int64_t chunks = win_chunk_count(L, front);
  for (int64_t t0 = 0; t0 < chunks; t0 += tile_chunks) {
    const int64_t tile0 = win_chunk_start(t0, front);
    if (L <= 0 || tile0 >= L) break;
    const int64_t tile_end = tile0 + 16 * tile_chunks < L ? tile0 + 16 * tile_chunks : L;
    const int32_t p_lo = win_last_start_le(E, 0, n - 1, tile0), p_hi = win_last_start_le(E, p_lo, n - 1, tile_end - 1);
    for (int64_t k = 0; k < tile_chunks; k++) {
      const int64_t x0 = tile0 + 16 * k;
      const bool live = x0 < tile_end;
      const int64_t lim = x0 + 16 < tile_end ? x0 + 16 : tile_end;
      WinCursor c;
      win_open(c, E, win_last_start_le(E, p_lo, p_hi, x0), front, x0);
      for (;;) {
        WinUnit u;
        if (!win_next(c, E, n, L, lim, live, u)) break;
        if (u.len == 0) continue;
        const uint8_t* ivp = ivs + 16 * (int64_t)u.part;
        if (u.is_iv) {
          for (int i = 0; i < 16; i++) {
            out[u.start + i] = ivp[i];
            if (cover) cover[u.start + i]++;
          }
          continue;
        }
        const uint32_t ivw[4] = {load_be32(ivp), load_be32(ivp + 4), load_be32(ivp + 8), load_be32(ivp + 12)};
        uint32_t ks[4];
        keystream_block(rk, nr, ivw, (uint64_t)u.block, ks, TableSbox{});
        uint8_t* d = out + (u.start + u.skip);
        const uint8_t* s = from_plain ? src + (Q[u.part] - (u.part == 0 && front > 0 ? front - 16 : 0) + u.plain) : d;
        for (int i = 0; i < u.len; i++) {
          const int b = u.skip + i;
          d[i] = (uint8_t)(s[i] ^ (ks[b >> 2] >> (24 - 8 * (b & 3))));
          if (cover) cover[u.start + u.skip + i]++;
        }
      }
    }
  }
}

int run_own(const char* path_in, const char* path_out) {
  FILE* in = fopen(path_in, "rb");
  FILE* outf = fopen(path_out, "wb");
  if (!in || !outf) return 2;
  uint32_t count = 0;
  if (fread(&count, sizeof count, 1, in) != 1) return 2;
  for (uint32_t cs = 0; cs < count; cs++) {
    uint32_t kb;
    int32_t n;
    int64_t front, tile_chunks, src_len;
    if (fread(&kb, sizeof kb, 1, in) != 1 || kb > 32) return 2;
    std::vector<uint8_t> key(kb);
    if (kb && fread(key.data(), 1, kb, in) != kb) return 2;
    if (fread(&n, sizeof n, 1, in) != 1 || n < 1 || fread(&front, sizeof front, 1, in) != 1 || fread(&tile_chunks, sizeof tile_chunks, 1, in) != 1)
      return 2;
    std::vector<int64_t> E((size_t)n + 1), Q((size_t)n + 1);
    std::vector<uint8_t> ivs((size_t)16 * (size_t)n);
    if (fread(E.data(), 8, E.size(), in) != E.size() || fread(Q.data(), 8, Q.size(), in) != Q.size()) return 2;
    if (fread(ivs.data(), 1, ivs.size(), in) != ivs.size() || fread(&src_len, sizeof src_len, 1, in) != 1) return 2;
    // exactly the sizes in use: a read or write one byte outside is a heap-buffer-overflow (sizes of 0 get no buffer at all)
    const size_t L = (size_t)E[(size_t)n], SL = (size_t)src_len;
    uint8_t* src = SL ? new uint8_t[SL] : nullptr;
    uint8_t* inplace = L ? new uint8_t[L] : nullptr;
    uint8_t* plain_out = L ? new uint8_t[L]() : nullptr;
    uint8_t* cover = L ? new uint8_t[L]() : nullptr;
    if (SL && fread(src, 1, SL, in) != SL) return 2;
    if (L && fread(inplace, 1, L, in) != L) return 2;
    std::vector<uint32_t> rk((size_t)4 * (size_t)(s3s_aes::rounds_for_key((int)kb) + 1));
    const int nr = s3s_aes::expand_key(key.data(), (int)kb, rk.data());
    if (nr == 0) return 3;
    walk(rk.data(), nr, ivs.data(), nullptr, E.data(), Q.data(), n, front, tile_chunks, false, inplace, cover);
    walk(rk.data(), nr, ivs.data(), src, E.data(), Q.data(), n, front, tile_chunks, true, plain_out, nullptr);
    if (L) {
      fwrite(inplace, 1, L, outf);
      fwrite(plain_out, 1, L, outf);
      fwrite(cover, 1, L, outf);
    }
    delete[] src;
    delete[] inplace;
    delete[] plain_out;
    delete[] cover;
  }
  fclose(outf);
  fclose(in);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
  if (argc == 4 && !strcmp(argv[1], "own")) return run_own(argv[2], argv[3]);
  return 2;
}
