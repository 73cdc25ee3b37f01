// Host build of the resumable Zstandard decoder and its unit walk (spark-s3-shuffle_amd/csrc/zstd_stream_core.h), driven feed
// by feed the way s3s_dstream_feed_device drives the kernels: TEST INFRASTRUCTURE (tests/zstd_stream_lib.py builds it under
// ASan / UBSan and runs it directly).  Every buffer a feed touches is a heap block of EXACTLY its size - the window, dst, the
// staging area [saved history | what the resumed frame decodes], the history kept between feeds - and between two feeds the
// state record and the history move to fresh allocations while the old ones are poisoned and freed.  A decoder that leans on
// whole-frame history, on bytes past the window or on a pointer into a previous window stops the run with a sanitizer report.
//
//   zstd_stream_model decode <file>   cases: i64 n, i64 content size (-1: none; with an expected code != 0: what the output must be a prefix of), i32 expected code, i32 wlog, i64 cap
//                                     (0: unlimited), i32 mode (0: the cuts given, 1: a feed per unit, 2: one byte short of and one
//                                     byte past every unit boundary), i32 ncuts, ncuts x i64 window ends, the bytes, the content
//   zstd_stream_model report <file>   the same cases, nothing expected of them (the expected code and the content are ignored):
//                                     one line per case - the code the stream ended with, the bytes it handed out, their CRC32
//   zstd_stream_model units <file>    records: i64 L, i64 pend, i32 open, i32 wlog, L bytes  ->  one line per record:
//                                     n stop need, then off:kind:payload per unit
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../spark-s3-shuffle_amd/csrc/zstd_stream_core.h"

using namespace s3s_zstd;

namespace {

template <class T>
std::unique_ptr<T[]> exact(size_t n) {
  return std::unique_ptr<T[]>(new T[n ? n : 1]);
}

struct Stream {
  bool open = false;
  ZStreamState* st = nullptr;
  uint8_t* hist = nullptr;
  int64_t hist_len = 0, window = 0, produced = 0, pos = 0;
  int64_t held_max = 0;  // the most history bytes held between feeds
  ~Stream() { drop(); }
  void drop() {
    if (st) {
      memset(st, 0xDD, sizeof *st);
      delete st;
    }
    if (hist) {
      memset(hist, 0xDD, (size_t)(hist_len ? hist_len : 1));
      delete[] hist;
    }
    st = nullptr;
    hist = nullptr;
    hist_len = 0;
  }
};

Work g_w;
HufWork g_h;

struct FeedOut {
  int64_t consumed = 0, out_len = 0, need_comp = 0, need_dst = 0;
};

// one feed: the window part[pos, wend) of a partition of n bytes, dst_capacity cap.  0, or a decoder code (ZS_BAD, ZS_UNSUPPORTED, ZS_CAPACITY)
int feed(Stream& s, const uint8_t* part, int64_t n, int64_t wend, int64_t cap, int wlog, std::vector<uint8_t>& out, FeedOut* fo) {
  const int64_t L = wend - s.pos;
  if (L == 0) return 0;
  auto win = exact<uint8_t>((size_t)L);
  memcpy(win.get(), part + s.pos, (size_t)L);
  const int64_t wmax = (int64_t)1 << wlog;
  int64_t stop = 0, need = 0;
  const int cnt = walk_piece(win.get(), 0, L, n - s.pos, s.open, wmax, false, nullptr, nullptr, 0, &stop, &need);
  if (cnt < 0) return cnt == -2 ? ZS_UNSUPPORTED : ZS_BAD;
  fo->need_comp = need;
  if (cnt == 0) return 0;
  auto units = exact<ZUnit>((size_t)cnt);
  auto dsize = exact<uint32_t>((size_t)cnt);
  auto unit_out = exact<int64_t>((size_t)cnt + 1);
  int64_t stop2 = 0;
  if (walk_piece(win.get(), 0, L, n - s.pos, s.open, wmax, true, units.get(), dsize.get(), 0, &stop2, &need) != cnt || stop2 != stop) return -100;
  const Lanes ln{0, 1};
  uint8_t dummy[8];
  ZPieceRes res;
  // ---- the size pass: the saved state is read, never written ----
  std::unique_ptr<ZStreamState> before;
  if (s.open) {
    before.reset(new ZStreamState);
    memcpy(before.get(), s.st, sizeof(ZStreamState));
  }
  int rc = run_piece(g_w, g_h, win.get(), units.get(), dsize.get(), nullptr, 0, cnt, false, s.open, s.st, nullptr, dummy, nullptr, s.hist_len,
                     nullptr, ln, &res);
  if (s.open && memcmp(before.get(), s.st, sizeof(ZStreamState)) != 0) return -101;
  if (rc != ZS_OK) return rc;
  unit_out[0] = 0;
  for (int i = 0; i < cnt; i++) unit_out[i + 1] = unit_out[i] + dsize[i];
  int k = cnt;
  if (cap > 0)
    for (k = 0; k < cnt && unit_out[k + 1] <= cap; k++) {}
  if (k == 0) {
    fo->need_dst = dsize[0];
    return ZS_CAPACITY;
  }
  const int64_t consumed = k < cnt ? units[k].off : stop, out_len = unit_out[k];
  bool open_after;
  int32_t fu = -1;
  {
    const ZUnit u = units[k - 1];
    const int kind = u.kind & 15;
    open_after = kind == ZU_FRAME || (kind >= ZU_RAW && !(u.kind & ZU_LAST));
    if (open_after) fu = u.frame_unit;
  }
  int64_t window = s.window, start = 0;
  if (open_after && fu >= 0) {
    FrameHdr fh;
    if (frame_header(win.get() + units[fu].off, units[fu].payload, &fh) != ZS_OK) return -102;
    window = fh.window;
    start = unit_out[fu];
  }
  // ---- the execute pass ----
  int64_t resumed_units = 0;
  while (resumed_units < k && ((units[resumed_units].kind & 15) >= ZU_RAW) && units[resumed_units].frame_unit == -1) resumed_units++;
  const int64_t resumed_expect = s.open ? unit_out[resumed_units] : 0;
  auto dst = exact<uint8_t>((size_t)out_len);
  auto staging = exact<uint8_t>((size_t)(s.hist_len + resumed_expect));
  if (s.open && s.hist_len) memcpy(staging.get(), s.hist, (size_t)s.hist_len);
  auto lit = exact<uint8_t>(kMaxBlock + 64);
  std::unique_ptr<ZStreamState> st_new(open_after ? new ZStreamState : nullptr);
  if (st_new) memset(st_new.get(), 0xEE, sizeof(ZStreamState));
  rc = run_piece(g_w, g_h, win.get(), units.get(), dsize.get(), unit_out.get(), 0, k, true, s.open, s.st, st_new.get(), dst.get(), staging.get(),
                 s.hist_len, lit.get(), ln, &res);
  if (rc != ZS_OK) return rc;
  if ((res.open != 0) != open_after || res.resumed_out != resumed_expect) return -103;
  if (resumed_expect) memcpy(dst.get(), staging.get() + s.hist_len, (size_t)resumed_expect);
  // ---- what survives the feed: the record and the last min(Window_Size, produced) bytes, in fresh allocations ----
  uint8_t* nhist = nullptr;
  int64_t nh = 0, produced = 0;
  if (open_after) {
    if (fu < 0) {
      produced = s.produced + out_len;
      nh = std::min(window, produced);
      nhist = new uint8_t[nh ? nh : 1];
      memcpy(nhist, staging.get() + (s.hist_len + out_len - nh), (size_t)nh);
    } else {
      produced = out_len - start;
      nh = std::min(window, produced);
      nhist = new uint8_t[nh ? nh : 1];
      memcpy(nhist, dst.get() + (out_len - nh), (size_t)nh);
    }
    if (st_new->produced != produced || st_new->window != window) return -104;
  }
  s.drop();
  s.open = open_after;
  s.st = st_new.release();
  s.hist = nhist;
  s.hist_len = nh;
  s.window = open_after ? window : 0;
  s.produced = produced;
  s.held_max = std::max(s.held_max, nh);
  if (nh > wmax) return -105;
  out.insert(out.end(), dst.get(), dst.get() + out_len);
  s.pos += consumed;
  fo->consumed = consumed;
  fo->out_len = out_len;
  fo->need_comp = 0;
  return 0;
}

// the whole partition through the window ends given; returns the first code that is not 0
int run_case(const uint8_t* part, int64_t n, int wlog, int64_t cap, int mode, std::vector<int64_t> cuts, std::vector<uint8_t>& out) {
  Stream s;
  if (mode != 0) cuts.clear();
  cuts.push_back(n);
  size_t ci = 0;
  int64_t wend = mode != 0 ? std::min<int64_t>(n, 1) : cuts[0];
  int guard = 0, unit_no = 0;
  while (s.pos < n) {
    if (++guard > 1 << 22) return -110;
    FeedOut fo;
    const int rc = feed(s, part, n, wend, cap, wlog, out, &fo);
    if (rc != 0) return rc;
    if (fo.consumed > 0 && mode == 0) continue;  // (the capacity may have ended the feed: the same window again)
    if (mode == 0) {
      if (wend == n) return -111;  // no progress with the whole rest in the window
      while (ci < cuts.size() && cuts[ci] <= wend) ci++;
      wend = cuts[ci];
    } else if (fo.consumed > 0) {  // a feed per unit: start over with one byte
      unit_no++;
      wend = std::min(n, s.pos + 1);
    } else {
      if (wend == n) return -111;
      // mode 1: exactly what the feed asked for.  mode 2: one byte short of it first (the same answer must come back), then it -
      // and for every other unit one byte more, a window that ends one byte past the unit's end
      int64_t next = s.pos + fo.need_comp;
      if (mode == 2 && wend < next - 1) next -= 1;
      else if (mode == 2 && (unit_no & 1)) next += 1;
      if (next <= wend) return -112;  // need_comp did not grow
      wend = std::min(n, next);
    }
  }
  if (s.open) return -113;
  return 0;
}

uint32_t crc32_of(const uint8_t* p, size_t n) {  // (zlib's: the caller compares it with zlib.crc32 of the bytes it expects)
  static uint32_t table[256];
  if (!table[1])
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
      table[i] = c;
    }
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
  return ~c;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 2;
  if (!strcmp(argv[1], "units")) {
    for (;;) {
      int64_t L, pend;
      int32_t open, wlog;
      if (fread(&L, 8, 1, f) != 1 || fread(&pend, 8, 1, f) != 1 || fread(&open, 4, 1, f) != 1 || fread(&wlog, 4, 1, f) != 1) break;
      auto win = exact<uint8_t>((size_t)L);
      if (L && fread(win.get(), 1, (size_t)L, f) != (size_t)L) return 2;
      int64_t stop = 0, need = 0;
      const int cnt = walk_piece(win.get(), 0, L, pend, open != 0, (int64_t)1 << wlog, false, nullptr, nullptr, 0, &stop, &need);
      printf("%d %lld %lld", cnt, (long long)(cnt < 0 ? 0 : stop), (long long)(cnt < 0 ? 0 : need));
      if (cnt > 0) {
        auto units = exact<ZUnit>((size_t)cnt);
        auto dsize = exact<uint32_t>((size_t)cnt);
        walk_piece(win.get(), 0, L, pend, open != 0, (int64_t)1 << wlog, true, units.get(), dsize.get(), 0, &stop, &need);
        for (int i = 0; i < cnt; i++) printf(" %lld:%d:%d", (long long)units[i].off, units[i].kind, units[i].payload);
      }
      printf("\n");
    }
    fclose(f);
    return 0;
  }
  const bool report = !strcmp(argv[1], "report");
  long n_cases = 0, n_wrong = 0;
  for (;;) {
    int64_t n, usize, cap;
    int32_t want, wlog, mode, ncuts;
    if (fread(&n, 8, 1, f) != 1 || fread(&usize, 8, 1, f) != 1 || fread(&want, 4, 1, f) != 1 || fread(&wlog, 4, 1, f) != 1 ||
        fread(&cap, 8, 1, f) != 1 || fread(&mode, 4, 1, f) != 1 || fread(&ncuts, 4, 1, f) != 1)
      break;
    std::vector<int64_t> cuts((size_t)ncuts);
    if (ncuts && fread(cuts.data(), 8, (size_t)ncuts, f) != (size_t)ncuts) return 2;
    auto part = exact<uint8_t>((size_t)n);
    auto content = exact<uint8_t>((size_t)(usize > 0 ? usize : 0));
    if (n && fread(part.get(), 1, (size_t)n, f) != (size_t)n) return 2;
    if (usize > 0 && fread(content.get(), 1, (size_t)usize, f) != (size_t)usize) return 2;
    std::vector<uint8_t> out;
    const int rc = run_case(part.get(), n, wlog, cap, mode, cuts, out);
    if (report) {  // nothing is expected: what the stream answered, for the caller to judge
      printf("%d %zu %u\n", rc, out.size(), crc32_of(out.data(), out.size()));
      n_cases++;
      continue;
    }
    bool ok = rc == want;
    if (ok && want == 0) ok = (int64_t)out.size() == usize && (usize == 0 || memcmp(out.data(), content.get(), (size_t)usize) == 0);
    // refused or corrupt with a content given: what was handed out before the verdict is a prefix of it
    if (ok && want != 0 && usize >= 0) ok = (int64_t)out.size() <= usize && (out.empty() || memcmp(out.data(), content.get(), out.size()) == 0);
    printf("case %ld: code %d (expected %d), %zu bytes (expected %lld)%s\n", n_cases, rc, (int)want, out.size(), (long long)usize, ok ? "" : "  WRONG");
    if (!ok) n_wrong++;
    n_cases++;
  }
  fclose(f);
  if (report) return 0;
  printf("zstd_stream_model: %ld cases, %ld wrong\n", n_cases, n_wrong);
  return n_wrong ? 1 : 0;
}
