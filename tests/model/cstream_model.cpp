// cstream_model.cpp — the host arithmetic of the streaming map side (spark-s3-shuffle_amd/csrc/compress_stream_core.h) as a
// stand-alone program: the plan of a window's units, the cut at a capacity and the stream's state (the take step of
// compress_stream_batch_core.h, as the feeds call it), driven by a schedule of feeds and the image sizes of a map output's units.  tests/test_compress_stream_cpu.py builds it with
// -fsanitize=address,undefined and compares every feed, field for field, with the Python model (tests/cstream_units.py).
// Every array has exactly the size in use, so that an index one too far is a sanitizer report.
//
// stdin:   codec bs nparts
//          nparts lines:  n_units size...
//          feeds, one a line:  src_len cap n_ends end...
// stdout:  one line a feed:  code consumed out_len need_src need_dst parts_closed length...
#include <cstdio>
#include <memory>
#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/compress_stream_batch_core.h"

struct Result {  // s3s_cstream_result
  int64_t consumed = 0, out_len = 0, need_src = 0, need_dst = 0;
  int32_t parts_closed = 0;
};

int main() {
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
      printf("-1 0 0 0 0 0\n");
      continue;
    }
    s3s_cs::Cut c;
    std::unique_ptr<int64_t[]> piece_off(new int64_t[(size_t)n_ends + 2]);
    if (codec == s3s_cs::kCodecNone) {
      c = s3s_cs::none_cut(src_len, ends.get(), n_ends, cap);
      piece_off[0] = 0;
      for (int j = 0; j < n_ends; j++) piece_off[(size_t)j + 1] = ends[(size_t)j] < c.out_len ? ends[(size_t)j] : c.out_len;
      piece_off[(size_t)n_ends + 1] = c.out_len;
    } else {
      int64_t n_units = 0;
      s3s_cs::plan_units(codec, bs, st.open_bytes, src_len, ends.get(), n_ends, [&](const s3s_cs::Unit&) { n_units++; });
      std::unique_ptr<s3s_cs::Unit[]> units(new s3s_cs::Unit[(size_t)n_units]);
      std::unique_ptr<int64_t[]> cum(new int64_t[(size_t)n_units + 1]);
      std::unique_ptr<int64_t[]> piece_first(new int64_t[(size_t)n_ends + 2]);  // first unit of every piece
      int64_t i = 0;
      int piece = 0;
      cum[0] = 0;
      piece_first[0] = 0;
      s3s_cs::plan_units(codec, bs, st.open_bytes, src_len, ends.get(), n_ends, [&](const s3s_cs::Unit& u) {
        while (piece < u.piece) piece_first[(size_t)++piece] = i;
        const int64_t part = n_closed + u.piece;
        const int64_t piece_start = u.piece == 0 ? 0 : ends[(size_t)u.piece - 1];
        const int64_t had = u.piece == 0 ? st.open_bytes : 0;
        const int64_t idx = u.len > 0 ? (had + u.src_off - piece_start) / bs : n_sizes[(size_t)part] - 1;
        units[(size_t)i] = u;
        cum[(size_t)i + 1] = cum[(size_t)i] + sizes[(size_t)part][(size_t)idx];
        i++;
      });
      while (piece < n_ends + 1) piece_first[(size_t)++piece] = i;
      c = s3s_cs::cut_units(units.get(), cum.get(), n_units, n_ends, codec == s3s_cs::kCodecLzf ? s3s_cs::kLzfBlock : bs, cap);
      for (int j = 0; j <= n_ends + 1; j++) {
        const int64_t o = cum[(size_t)piece_first[(size_t)j]];
        piece_off[(size_t)j] = o < c.out_len ? o : c.out_len;
      }
    }
    std::unique_ptr<int64_t[]> lengths(new int64_t[(size_t)c.parts_closed]);
    Result r;
    if (!s3s_cs::take_window(&st, &carry, nullptr, c, ends.get(), piece_off.get(), nullptr, nullptr, nullptr, lengths.get(), nullptr, &r)) {
      printf("-2 0 0 0 %lld 0\n", (long long)r.need_dst);
      continue;
    }
    n_closed += r.parts_closed;
    printf("0 %lld %lld %lld 0 %d", (long long)r.consumed, (long long)r.out_len, (long long)c.need_src, (int)r.parts_closed);
    for (int j = 0; j < r.parts_closed; j++) printf(" %lld", (long long)lengths[(size_t)j]);
    printf("\n");
  }
  return 0;
}
