// dstream_model.cpp — the host side of the streaming reduce side (csrc/decode_stream_core.h) as a stand-alone program:
// tests/test_decode_stream_core_cpu.py builds it with -fsanitize=address,undefined and talks to it over a pipe.  The program
// plays what decode_stream.hip does between the launches, in the same order; the kernels' part - discovery, the cut, the
// checksums, the decode status - is played by the test (the Python model of the contract), so none of it is in here.
// Every array has exactly the size in use: a rule that reads or writes one element too far is AddressSanitizer's.
//
//   R codec algo enc nparts off[nparts + 1] ref[nparts]      a new stream over this range, at position 0
//   F window_len cap                                         one feed:
//     -> D ppos PL pleft first_mid plast_pend n m  off[n + 1]  seed[n]  q[m + 1] c[m] (encrypted only)
//        what the device is handed: the plain window starts at plain range offset ppos and holds PL bytes
//     <- K status stop need n_frames  cut_status k consumed out_len need_dst  decode_status  sums[n]
//     -> S a b seed       the second checksum launch over [a, b) of the window       <- its sum
//     -> A code consumed out_len need_comp need_dst bad_partition at_end pos cur carry
//   (a feed that needs no device work answers A at once)
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "decode_stream_core.h"

namespace ds = s3s_ds;

namespace {

constexpr int kInvalid = -1, kCapacity = -2, kHip = -5;
constexpr int64_t kSegBytes = 16384;

struct Stream {
  int codec = 0, algo = 0, enc = 0;
  int32_t nparts = 0;
  std::unique_ptr<int64_t[]> off, ref, poff;
  ds::Pos at;
  int err = 0;
  int32_t bad = -1;
  ds::Range range() const { return {off.get(), ref.get(), enc ? poff.get() : nullptr, nparts, algo}; }
};

struct Result {
  int code = 0;
  int64_t consumed = 0, out_len = 0, need_comp = 0, need_dst = 0;
  int32_t bad = -1, at_end = 0;
};

long long rd() {
  long long v;
  if (scanf("%lld", &v) != 1) {
    fprintf(stderr, "dstream_model: short input\n");
    exit(2);
  }
  return v;
}

int stick(Stream& s, Result& r, int code, int32_t bad) {
  s.err = code;
  s.bad = bad;
  r.consumed = r.out_len = 0;
  r.bad = bad;
  return code;
}

int refuse(Stream& s, Result& r, ds::Refusal v) { return v.code == ds::kUnsupported ? v.code : stick(s, r, v.code, v.bad); }

int feed(Stream& s, int64_t comp_len, int64_t cap, Result& r) {
  if (s.err) {
    r.bad = s.bad;
    return s.err;
  }
  const ds::Range R = s.range();
  if (comp_len < 0 || cap < 0 || comp_len > R.total() - s.at.pos) return kInvalid;
  const int64_t L = ds::window_len(R, s.at, s.codec, comp_len, cap);
  if (comp_len > 0 && L == 0) {
    r.need_dst = 1;
    return kCapacity;
  }
  if (L == 0) {
    const int32_t bad = ds::pass_empty(R, s.at);
    if (bad >= 0) return stick(s, r, ds::kChecksum, bad);
    r.at_end = ds::at_end(R, s.at);
    if (R.total() > s.at.pos) r.need_comp = ds::min_unit(R, s.at, s.codec, false);
    return 0;
  }
  // the staging area
  const int32_t n = ds::piece_count(R, s.at, L);
  std::unique_ptr<int64_t[]> off(new int64_t[n + 1]), seed(new int64_t[n]), sums(new int64_t[n]);
  std::unique_ptr<int32_t[]> seg(new int32_t[n + 1]);
  std::unique_ptr<int64_t[]> q(new int64_t[s.enc ? n + 1 : 0]), c(new int64_t[s.enc ? n : 0]);
  if (ds::fill_pieces(R, s.at, L, n, kSegBytes, off.get(), seg.get(), seed.get()) > ds::kMaxCount) return ds::kUnsupported;
  int64_t segs = 0;
  for (int32_t i = 0; i < n; i++) {  // (the segment starts are the running sum of the pieces' segments)
    if (seg[i] != segs) return kHip;
    segs += ds::segs_of(off[i + 1] - off[i], kSegBytes);
  }
  if (seg[n] != segs || segs != ds::window_segs(R, s.at, L, n, kSegBytes)) return kHip;
  const ds::Plain pl = ds::plain_side(R, s.at, L, n, off.get(), s.enc ? q.get() : nullptr, s.enc ? c.get() : nullptr);
  printf("D %lld %lld %lld %d %lld %d %d ", (long long)(s.enc ? s.poff[s.at.cur] + pl.pfront : s.at.pos), (long long)pl.PL, (long long)pl.pleft,
         pl.first_mid ? 1 : 0, (long long)pl.plast_pend, n, pl.m);
  for (int32_t i = 0; i <= n; i++) printf(" %lld", (long long)off[i]);
  for (int32_t i = 0; i < n; i++) printf(" %lld", (long long)seed[i]);
  if (s.enc) {
    for (int32_t i = 0; i <= pl.m; i++) printf(" %lld", (long long)q[i]);
    for (int32_t i = 0; i < pl.m; i++) printf(" %lld", (long long)c[i]);
  }
  printf("\n");
  fflush(stdout);
  // the device's words
  const int status = (int)rd();
  const int64_t stop = rd(), need = rd(), n_frames = rd();
  const int cut_status = (int)rd();
  const int64_t cut_k = rd(), cut_consumed = rd(), cut_out = rd(), cut_need = rd();
  const int dec_status = (int)rd();
  for (int32_t i = 0; i < n; i++) sums[i] = rd();

  int64_t k = 0, consumed = pl.PL, out_len = pl.PL, need_comp = 0;
  if (s.codec != ds::kCodecNone && pl.PL != 0) {
    if (status != 0) return refuse(s, r, ds::refusal(R, s.at, L, n, sums.get(), status));
    need_comp = need;
    if (!ds::stop_valid(stop, need, pl.PL)) return kHip;
    if (n_frames > ds::kMaxCount) return ds::kUnsupported;
    consumed = stop;
    out_len = 0;
    if (n_frames > 0) {
      if (cut_status != 0) return refuse(s, r, ds::refusal(R, s.at, L, n, sums.get(), cut_status));
      k = cut_k, consumed = cut_consumed, out_len = cut_out;
      if (!ds::cut_valid(k, consumed, out_len, n_frames, stop, cap)) return kHip;
      if (ds::nothing_fits(pl, consumed)) {
        r.need_dst = cut_need;
        return kCapacity;
      }
    }
  }
  const ds::Stored st = ds::back_to_stored(pl, consumed, need_comp);
  if (st.into_short_part) return refuse(s, r, ds::refusal(R, s.at, L, n, sums.get(), ds::kBadFrame));
  consumed = st.consumed;
  need_comp = st.need_comp;
  const ds::Verdict v = ds::verdict(R, s.at, consumed, sums.get());
  if (v.bad >= 0) return stick(s, r, ds::kChecksum, v.bad);
  ds::Carry carry = ds::open_carry(R, s.at, n, off.get(), sums.get(), v.cur, consumed);
  const bool second = carry.kind == ds::Carry::kSecond;
  if (s.codec != ds::kCodecNone && (k > 0 || second)) {
    if (second) {
      printf("S %lld %lld %lld\n", (long long)carry.a, (long long)carry.b, (long long)carry.value);
      fflush(stdout);
      carry.value = rd();
    }
    if (dec_status == ds::kUnsupported) return dec_status;
    if (dec_status != 0) return refuse(s, r, ds::refusal(R, s.at, L, n, sums.get(), ds::kBadFrame));
  }
  const ds::Commit cm = ds::commit(R, s.at, pl.front, v.cur, consumed, carry.value, need_comp);
  if (cm.iv_piece >= pl.m) return kHip;  // the IV it names came back with the window's
  r.consumed = consumed;
  r.out_len = out_len;
  r.need_comp = cm.need_comp;
  r.at_end = cm.at_end;
  return 0;
}

}  // namespace

int main() {
  Stream s;
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'R') {
      s = Stream();
      s.codec = (int)rd(), s.algo = (int)rd(), s.enc = (int)rd(), s.nparts = (int32_t)rd();
      s.off.reset(new int64_t[s.nparts + 1]);
      s.ref.reset(new int64_t[s.nparts]);
      for (int32_t p = 0; p <= s.nparts; p++) s.off[p] = rd();
      for (int32_t p = 0; p < s.nparts; p++) s.ref[p] = rd();
      s.at.carry = ds::fresh(s.algo);
      if (s.enc) {
        s.poff.reset(new int64_t[s.nparts + 1]);
        s.poff[0] = 0;
        for (int32_t p = 0; p < s.nparts; p++) {
          const int64_t len = s.off[p + 1] - s.off[p];
          s.poff[p + 1] = s.poff[p] + (len >= ds::kIv ? len - ds::kIv : 0);
        }
      }
    } else if (cmd == 'F') {
      const int64_t comp_len = rd(), cap = rd();
      Result r;
      r.code = feed(s, comp_len, cap, r);
      printf("A %d %lld %lld %lld %lld %d %d %lld %d %lld\n", r.code, (long long)r.consumed, (long long)r.out_len, (long long)r.need_comp,
             (long long)r.need_dst, r.bad, r.at_end, (long long)s.at.pos, s.at.cur, (long long)s.at.carry);
      fflush(stdout);
    } else {
      fprintf(stderr, "dstream_model: unknown command %c\n", cmd);
      return 2;
    }
  }
  return 0;
}
