// decode_stream.hip — the streaming reduce side of the C-ABI: a fetched range decoded window by window, in bounded memory.
//
// The reference never holds a whole block: storage/S3BufferedInputStreamAdaptor.scala:13-19 buffers
// min(maxBufferSizeTask, block length), storage/S3ChecksumValidationStream.scala:54-86 validates a partition as its last byte
// streams past, and the codec input streams decode frame by frame.  An s3s_dstream does the same with the one-shot path's
// kernels: a feed discovers the whole units of its window (stream-mode discovery: a unit cut by the window's end is a place
// to stop, not corruption), cuts the frame table at the caller's output capacity (frames_cut_kernel), continues the open
// partition's checksum (checksum_seed_kernel) - decode_stream_kernels.hip - and launches the unchanged decoders on the cut table.
//
// Host waits per feed, as in s3s_decompress_range_device: discovery, frame table + cut, decode.  The checksums of the
// window's pieces of partitions are queued in front of discovery and arrive with its first wait; only the piece of a partition
// that the CUT leaves open (the capacity ended the feed inside it) is summed again, behind the decode launch.
//
// Under Spark IO encryption (s3s_dstream_open_encrypted) a feed has two sides.  The STORED side - the window as fetched, IVs
// included - is what the checksums run over and what consumed, need_comp and the position count.  The PLAIN side is the window
// decrypted into the crypt workspace by the window form of the AES-CTR pass (aes_ctr_stream.hip), queued in front of
// discovery: discovery, the emit kernels, the cut and the decoders read it with plain offsets and do not know of the layer.
// The host maps a plain offset back by adding 16 for every IV passed.  No wait is added: the IVs that start in the window
// come back with the first wait, and the one of the partition a feed leaves open stays in the stream (host memory).
//
// Zstandard (s3s_dstream_open_zstd) is the one codec whose stream is not host-only: the units are frame headers,
// blocks and skippable frames, a block's decoded size is known only after a size pass (one more wait per feed), and the frame
// that is open at the position keeps a state record and its last min(Window_Size, produced) bytes in device memory of the
// stream's own.  The kernels are zstd_decode_stream.hip; the frame resumed by a feed decodes behind its saved history in a
// staging area of the workspace and is copied to dst, frames that start in the feed decode straight into dst.
#include <algorithm>
#include <atomic>
#include <new>

#define S3S_AES_DEVICE
#include "aes_ctr_core.h"
#include "s3s_ctx.h"
#include "zstd_decode_stream.h"

using namespace s3s;

struct s3s_dstream {
  s3s_ctx* ctx;
  int codec, algo;
  int32_t nparts;
  std::vector<int64_t> off, ref;  // part_offsets[nparts + 1], ref_checksums[nparts] (copies)
  int64_t pos = 0;                // bytes of the range consumed
  int32_t cur = 0;                // partitions [0, cur) are verified; partition cur is open
  int64_t carry = 0;              // checksum state of partition cur over [off[cur], pos)
  int err = S3S_OK;               // sticky: S3S_E_CHECKSUM / S3S_E_BAD_FRAME
  int32_t bad_partition = -1;
  // s3s_dstream_open_encrypted: pos and off are STORED coordinates.  pos is never inside an IV: it is off[cur] (the IV of
  // partition cur not consumed yet) or at least off[cur] + 16, and then iv holds that IV
  bool enc = false;
  uint64_t epoch = 0;         // the context's key setting the stream is bound to (s3s_ctx::enc_epoch)
  std::vector<int64_t> poff;  // plain offsets of the partitions: a stored partition of 16 bytes or more loses its IV, a shorter one is empty
  uint8_t iv[16] = {};
  // s3s_dstream_open_zstd: the one frame that is open at the position.  zmem = [ZStreamState | the last zhist_len bytes of the
  // frame's output], device memory of the stream's own (not the context's workspace: other calls run between two feeds),
  // allocated when a frame first stays open across a feed, sized by that frame's Window_Size, freed when the frame ends
  int wlog = 0;               // window_log_max (0: not a Zstandard stream)
  bool zopen = false;
  void* zmem = nullptr;
  int64_t zwindow = 0, zproduced = 0, zhist_len = 0;
  int64_t zheld = 0;          // bytes of zmem as allocated
};

namespace {

constexpr size_t kZStateBytes = (sizeof(s3s_zstd::ZStreamState) + 255) & ~size_t(255);  // the history bytes start behind the record

// device bytes that Zstandard streams hold between feeds: this stream's (zheld) and the process's (s3s_dstream_held_bytes)
std::atomic<int64_t> g_zheld{0};

void zfree(s3s_dstream* s) {
  if (s->zmem) (void)hipFree(s->zmem);
  g_zheld -= s->zheld;
  s->zheld = 0;
  s->zmem = nullptr;
  s->zopen = false;
  s->zwindow = s->zproduced = s->zhist_len = 0;
}
struct ZNew {  // device memory of a frame that may stay open: the stream's once the feed has succeeded, freed otherwise
  void* p = nullptr;
  ~ZNew() {
    if (p) (void)hipFree(p);
  }
};

inline int64_t fresh(int algo) { return algo == S3S_CHECKSUM_ADLER32 ? 1 : 0; }  // getValue() of a new Adler32 / CRC32 / CRC32C

inline bool at_end(const s3s_dstream* s) { return s->pos == s->off[(size_t)s->nparts] && s->cur == s->nparts; }

// the smallest window that can hold a unit's header when the window shows nothing of it
inline int64_t min_unit(const s3s_dstream* s) {
  const int64_t part_start = s->off[(size_t)(s->cur < s->nparts ? s->cur : s->nparts)];
  if (s->enc && s->pos == part_start) return s3s_aes::kBlock;  // the IV is the next unit
  switch (s->codec) {
    case S3S_CODEC_LZ4: return kLz4FrameHeader;
    case S3S_CODEC_SNAPPY: return s->pos == part_start + (s->enc ? s3s_aes::kBlock : 0) ? kSnappyStreamHeader : 4;
    case S3S_CODEC_LZF: return 5;
    case S3S_CODEC_ZSTD: return s->zopen ? 3 : 6;  // a block header; a frame header's first step
    default: return 1;
  }
}

int stick(s3s_dstream* s, s3s_dstream_result* r, int code, int32_t bad_partition, const char* what) {
  s->err = code;
  s->bad_partition = bad_partition;
  r->consumed = r->out_len = 0;
  r->bad_partition = bad_partition;
  if (code == S3S_E_CHECKSUM) return fail(s->ctx, code, "Invalid checksum detected for partition %d of the range", bad_partition);
  return fail(s->ctx, code, "Stream is corrupted (%s, range offset %lld)", what, (long long)s->pos);
}

// S3S_CODEC_NONE under encryption: the stored bytes of the window [pos, pos + len) that a feed takes when dst holds cap bytes.
// Known before anything runs: a unit is a byte, or an IV (no output) that is whole in the window.  A window that shows a cut
// IV or a partition shorter than one is left whole - the feed itself decides on those, and its plain bytes fit cap.
int64_t none_cut_encrypted(const s3s_dstream* s, int64_t len, int64_t cap) {
  const int64_t wend = s->pos + len;
  int64_t out = 0;
  for (int32_t p = s->cur; p < s->nparts && s->off[(size_t)p] < wend; p++) {
    const int64_t a = s->off[(size_t)p], b = s->off[(size_t)p + 1];
    if (b == a) continue;
    int64_t c = s->pos;  // the first cipher byte of the partition in the window: the open partition's is the position
    if (s->pos <= a) {
      if (b - a < s3s_aes::kBlock || a + s3s_aes::kBlock > wend) return len;
      c = a + s3s_aes::kBlock;
    }
    const int64_t e = b < wend ? b : wend;
    if (e - c > cap - out) return c + (cap - out) - s->pos;
    out += e - c;
  }
  return len;
}

int open_stream(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums, int32_t nparts,
                s3s_dstream** out, bool encrypted, int zstd_wlog = 0) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  if (!out) return fail(ctx, S3S_E_INVALID, "null/invalid argument");
  *out = nullptr;
  if (nparts < 0 || !part_offsets) return fail(ctx, S3S_E_INVALID, "null/invalid argument");
  if (codec != S3S_CODEC_NONE && codec != S3S_CODEC_LZ4 && codec != S3S_CODEC_SNAPPY && codec != S3S_CODEC_ZSTD && codec != S3S_CODEC_LZF)
    return fail(ctx, S3S_E_INVALID, "unknown codec %d", codec);
  if (checksum_algo != S3S_CHECKSUM_NONE && checksum_algo != S3S_CHECKSUM_ADLER32 && checksum_algo != S3S_CHECKSUM_CRC32 &&
      checksum_algo != S3S_CHECKSUM_CRC32C)
    return fail(ctx, S3S_E_INVALID, "Unsupported shuffle checksum algorithm: %d", checksum_algo);
  if (part_offsets[0] != 0) return fail(ctx, S3S_E_INVALID, "part_offsets must start at 0");
  for (int32_t p = 0; p < nparts; p++)
    if (part_offsets[p + 1] < part_offsets[p]) return fail(ctx, S3S_E_INVALID, "part_offsets not monotonic at %d", p);
  if (checksum_algo != S3S_CHECKSUM_NONE && nparts > 0 && !ref_checksums)
    return fail(ctx, S3S_E_INVALID, "ref_checksums is null but a checksum algorithm is selected");
  if (encrypted && !enc_on(ctx)) return fail(ctx, S3S_E_INVALID, "s3s_dstream_open_encrypted on a context without IO encryption");
  if (codec == S3S_CODEC_ZSTD && !zstd_wlog)  // the units and the device state of a Zstandard stream are the opt-in of s3s_dstream_open_zstd
    return fail(ctx, S3S_E_UNSUPPORTED, "Zstandard ranges are streamed by s3s_dstream_open_zstd (or use s3s_decompress_range*)");
  if (!encrypted && enc_on(ctx))  // the caller has to know the IV unit: s3s_dstream_open_encrypted is the opt-in
    return fail(ctx, S3S_E_UNSUPPORTED, "ranges under IO encryption are streamed by s3s_dstream_open_encrypted");
  s3s_dstream* s = new (std::nothrow) s3s_dstream();
  if (!s) return fail(ctx, S3S_E_NOMEM, "out of host memory");
  s->ctx = ctx;
  s->codec = codec;
  s->algo = checksum_algo;
  s->nparts = nparts;
  s->off.assign(part_offsets, part_offsets + nparts + 1);
  if (checksum_algo != S3S_CHECKSUM_NONE && nparts > 0) s->ref.assign(ref_checksums, ref_checksums + nparts);
  s->carry = fresh(checksum_algo);
  s->wlog = zstd_wlog;
  if (encrypted) {
    s->enc = true;
    s->epoch = ctx->enc_epoch;
    s->poff.assign((size_t)nparts + 1, 0);
    for (int32_t p = 0; p < nparts; p++) {
      const int64_t len = part_offsets[p + 1] - part_offsets[p];
      s->poff[(size_t)p + 1] = s->poff[(size_t)p] + (len >= s3s_aes::kBlock ? len - s3s_aes::kBlock : 0);
    }
  }
  *out = s;
  return S3S_OK;
}

}  // namespace

extern "C" {

int s3s_dstream_open(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                     int32_t nparts, s3s_dstream** out) {
  return open_stream(ctx, codec, checksum_algo, part_offsets, ref_checksums, nparts, out, false);
}

int s3s_dstream_open_encrypted(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                               int32_t nparts, s3s_dstream** out) {
  return open_stream(ctx, codec, checksum_algo, part_offsets, ref_checksums, nparts, out, true);
}

int s3s_dstream_open_zstd(s3s_ctx* ctx, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums, int32_t nparts,
                          int32_t window_log_max, s3s_dstream** out) {
  if (!ctx) return S3S_E_INVALID;
  if (out) *out = nullptr;
  if (window_log_max < 10 || window_log_max > 27) return fail(ctx, S3S_E_INVALID, "window_log_max %d is outside 10 .. 27", window_log_max);
  return open_stream(ctx, S3S_CODEC_ZSTD, checksum_algo, part_offsets, ref_checksums, nparts, out, false, window_log_max);
}

int64_t s3s_dstream_held_bytes(const s3s_dstream* s) { return s ? s->zheld : g_zheld.load(); }

int64_t s3s_dstream_position(const s3s_dstream* s) { return s ? s->pos : (int64_t)S3S_E_INVALID; }

int s3s_dstream_close(s3s_dstream* s) {
  if (!s) return S3S_E_INVALID;
  const int rc = s->err != S3S_OK ? s->err : at_end(s) ? S3S_OK : S3S_E_BAD_FRAME;
  wipe(s->iv, sizeof s->iv);
  if (s->zmem) {  // (a close in the middle of a range: the open frame's state goes with the stream)
    (void)hipSetDevice(s->ctx->device);
    zfree(s);
  }
  delete s;
  return rc;
}

int s3s_dstream_feed_device(s3s_dstream* s, const uint8_t* d_comp, int64_t comp_len, uint8_t* d_dst, int64_t dst_capacity,
                            s3s_dstream_result* r) {
  if (!s || !r) return S3S_E_INVALID;
  s3s_ctx* ctx = s->ctx;
  ctx->err[0] = 0;
  memset(r, 0, sizeof *r);
  r->bad_partition = -1;
  if (s->err != S3S_OK) {
    r->bad_partition = s->bad_partition;
    return fail(ctx, s->err, "the stream failed in an earlier feed (%s)", s->err == S3S_E_CHECKSUM ? "Invalid checksum detected" : "Stream is corrupted");
  }
  const int32_t np = s->nparts;
  const int64_t total = s->off[(size_t)np], left = total - s->pos;
  if (comp_len < 0 || dst_capacity < 0 || (comp_len > 0 && !d_comp) || (dst_capacity > 0 && !d_dst))
    return fail(ctx, S3S_E_INVALID, "null/invalid argument");
  if (comp_len > left) return fail(ctx, S3S_E_INVALID, "the window reaches %lld bytes past the end of the range", (long long)(comp_len - left));
  const bool enc = s->enc;
  if (enc && (s->epoch != ctx->enc_epoch || !enc_on(ctx)))  // bound to the key setting it was opened under: it can only be closed
    return fail(ctx, S3S_E_INVALID, "s3s_set_io_encryption was called on the context after the stream was opened");
  if (!enc && enc_on(ctx)) return fail(ctx, S3S_E_UNSUPPORTED, "IO encryption was switched on after the stream was opened");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& v : ctx->stage_ms) v = 0;
  const bool do_sum = s->algo != S3S_CHECKSUM_NONE;
  const int codec = s->codec;

  // bytes this feed looks at: S3S_CODEC_NONE's units are bytes, so its cut is known before anything runs
  int64_t L = comp_len;
  if (codec == S3S_CODEC_NONE && !enc && dst_capacity < L) L = dst_capacity;
  if (codec == S3S_CODEC_NONE && enc) L = none_cut_encrypted(s, comp_len, dst_capacity);  // (0: the next unit is a byte and dst holds none)
  if (comp_len > 0 && L == 0) {
    r->need_dst = 1;
    return fail(ctx, S3S_E_CAPACITY, "dst_capacity 0 < 1");
  }
  // pieces of partitions in [pos, pos + L): partition cur (open), the ones that start inside, and empty ones at its end
  const int64_t wend = s->pos + L;
  int32_t n = 0;
  while (s->cur + n < np && (s->off[(size_t)(s->cur + n)] < wend || s->off[(size_t)(s->cur + n) + 1] <= wend)) n++;

  if (L == 0) {  // nothing to look at: the position may still pass empty partitions
    int32_t q = s->cur;
    for (; q < np && s->off[(size_t)q + 1] <= s->pos; q++)
      if (do_sum && s->ref[(size_t)q] != (q == s->cur ? s->carry : fresh(s->algo))) return stick(s, r, S3S_E_CHECKSUM, q, "");
    if (q != s->cur) s->carry = fresh(s->algo);
    s->cur = q;
    r->at_end = at_end(s);
    if (left > 0) r->need_comp = min_unit(s);
    return S3S_OK;
  }

  // pinned staging: [piece offsets n + 1][second-launch offsets 2][seg_start n + 1][second seg_start 2][seeds n + 1][sums n + 1][misc 8]
  auto al = [](size_t x) { return (x + 15) & ~size_t(15); };
  const size_t n1 = (size_t)n + 1;
  const size_t o_off2 = al(8 * n1), o_seg = al(o_off2 + 16), o_seg2 = al(o_seg + 4 * n1), o_seed = al(o_seg2 + 8),
               o_sums = al(o_seed + 8 * n1), o_misc = al(o_sums + 8 * n1),
               // encrypted: [plain piece offsets n + 1][first cipher byte of every piece n + 1][the IVs that start in the window n + 1]
               o_q = al(o_misc + 128), o_c = al(o_q + 8 * n1), o_iv = al(o_c + 8 * n1), stage_total = enc ? o_iv + 16 * n1 : o_misc + 128;
  int rc;
  if ((rc = ensure_stage(ctx, stage_total))) return rc;
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  int64_t* h_off = reinterpret_cast<int64_t*>(hs);
  int64_t* h_off2 = reinterpret_cast<int64_t*>(hs + o_off2);
  int32_t* h_seg = reinterpret_cast<int32_t*>(hs + o_seg);
  int32_t* h_seg2 = reinterpret_cast<int32_t*>(hs + o_seg2);
  int64_t* h_seed = reinterpret_cast<int64_t*>(hs + o_seed);
  int64_t* h_sums = reinterpret_cast<int64_t*>(hs + o_sums);  // [n] = the second launch's sum
  int64_t* h_misc = reinterpret_cast<int64_t*>(hs + o_misc);  // [0] n_frames, [1] status, [2..5] stop, need / k, consumed, out_len, need; Zstandard: [6..9] open, frame unit, window, out start, [10] resumed bytes
  int64_t* h_q = reinterpret_cast<int64_t*>(hs + o_q);
  int64_t* h_c = reinterpret_cast<int64_t*>(hs + o_c);
  const uint8_t* h_iv = hs + o_iv;
  int64_t segs = 0;
  for (int32_t i = 0; i < n; i++) {
    const int64_t a = s->off[(size_t)(s->cur + i)] - s->pos, b = s->off[(size_t)(s->cur + i) + 1] - s->pos;
    h_off[i] = a < 0 ? 0 : a;
    h_off[i + 1] = b < L ? b : L;
    h_seg[i] = (int32_t)segs;
    segs += worst_segs(h_off[i + 1] - h_off[i]);
    h_seed[i] = i == 0 ? s->carry : fresh(s->algo);
  }
  if (n == 0) h_off[0] = 0;
  h_seg[n] = (int32_t)segs;
  if (segs > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "window too large for one feed");
  const int64_t last_pend = n > 0 ? s->off[(size_t)(s->cur + n)] - s->pos : 0;  // where the last piece's partition ends (>= L: the window cuts it)
  // ---- the plain side: what discovery and the decoders see.  Without the layer it IS the stored side ----------------------
  // Encrypted: the first m pieces, up to the first whose IV the window's end cuts (iv_cut: it contributes nothing yet) or
  // whose partition is shorter than an IV (short_part: corrupt, reported by the feed that consumes everything in front of it)
  const int64_t front = enc && s->cur < np ? s->pos - s->off[(size_t)s->cur] : 0;  // stored bytes of partition cur in front of the window: 0 or >= 16
  const int64_t pfront = front > 0 ? front - s3s_aes::kBlock : 0;                  // ... and plain ones
  int32_t m = n;
  int64_t PL = L;
  bool iv_cut = false, short_part = false;
  if (enc) {
    m = 0;
    PL = 0;
    for (int32_t i = 0; i < n; i++) {
      const int64_t stored = s->off[(size_t)(s->cur + i) + 1] - s->off[(size_t)(s->cur + i)];
      int64_t c;
      if (i == 0 && front > 0) c = 0;
      else if (stored == 0) c = h_off[i];
      else if (stored < s3s_aes::kBlock) { short_part = true; break; }
      else if (h_off[i + 1] - h_off[i] < s3s_aes::kBlock) { iv_cut = true; break; }
      else c = h_off[i] + s3s_aes::kBlock;
      h_q[i] = PL;
      h_c[i] = c;
      PL += h_off[i + 1] - c;
      m = i + 1;
    }
    h_q[m] = PL;
  }
  // a plain offset of the window as a stored one: add 16 for every IV passed (an IV in front of the next plain byte is passed:
  // a unit of no output always fits)
  auto to_stored = [&](int64_t x) -> int64_t {
    if (!enc) return x;    // one coordinate system
    if (m == 0) return 0;  // no plain piece (a cut IV or a short partition at the window's start): nothing can be consumed
    // the LAST piece that starts at or in front of x (h_q[0] = 0 <= x): of several pieces that start AT x - empty ones, and the
    // one x lies in - the last, so that the IVs (and empty partitions) between them are passed
    const int64_t i = (std::upper_bound(h_q, h_q + m, x) - h_q) - 1;
    return h_c[i] + (x - h_q[i]);
  };
  const int32_t pn = m;
  // piece 0 starts inside a codec stream (no Snappy stream header expected there): plain bytes of its partition lie in front
  const bool first_mid = enc ? pfront > 0 : s->pos > s->off[(size_t)s->cur];
  // what the RANGE still holds from the window's start, in plain bytes: a unit that crosses it is corrupt, not cut
  int64_t pleft = left;
  if (enc && short_part) pleft = PL;  // the plain side ends at a partition shorter than its IV: nothing valid lies behind it
  else if (enc) pleft = s->poff[(size_t)np] - (s->poff[(size_t)s->cur] + pfront);
  // where the last plain piece's partition ends, window-relative in plain bytes (>= PL when the window cuts it)
  int64_t plast_pend = last_pend;
  if (enc && m == 0) plast_pend = 0;  // no plain piece at all
  else if (enc) {
    const int64_t plain_len = s->poff[(size_t)(s->cur + m)] - s->poff[(size_t)(s->cur + m) - 1];  // of partition cur + m - 1
    plast_pend = h_q[m - 1] + plain_len - (m == 1 ? pfront : 0);  // (m == 1: it is the open partition, pfront of it lie in front)
  }
  // device: B_OFFSETS [piece offsets n + 1][2], B_REF_SUMS [seeds n + 1], B_SUMS [n + 1], B_STATUS [status][pad][result 9 x int64]
  if ((rc = ensure(ctx, B_OFFSETS, 8 * (n1 + 2)))) return rc;
  if ((rc = ensure(ctx, B_REF_SUMS, 8 * n1))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * n1))) return rc;
  if ((rc = ensure(ctx, B_STATUS, 128))) return rc;
  int64_t* d_off = dev<int64_t>(ctx, B_OFFSETS);
  const uint8_t* P = d_comp;      // the plain bytes of the window
  const int64_t* d_poff = d_off;  // ... and their pieces
  if (enc) {  // device: B_CRYPT [the window decrypted], B_CRYPT_OFF [plain piece offsets n + 1][IVs n + 1]
    if ((rc = ensure(ctx, B_CRYPT, (size_t)PL + 64))) return rc;
    if ((rc = ensure(ctx, B_CRYPT_OFF, 24 * n1))) return rc;
    d_off = dev<int64_t>(ctx, B_OFFSETS);
    P = dev<uint8_t>(ctx, B_CRYPT);
    d_poff = dev<int64_t>(ctx, B_CRYPT_OFF);
  }
  int32_t* d_status = dev<int32_t>(ctx, B_STATUS);
  int64_t* d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + 16);
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, 128, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_off, h_off, 8 * n1, hipMemcpyHostToDevice, ctx->stream));
  if (enc && m > 0 && h_off[m] > 0) {  // the decrypt pass, in front of discovery; the IVs it gathers arrive with the first wait
    uint8_t* d_iv = dev<uint8_t>(ctx, B_CRYPT_OFF) + 8 * n1;
    const AesWindowIv iv0 = {{s3s_aes::load_be32(s->iv), s3s_aes::load_be32(s->iv + 4), s3s_aes::load_be32(s->iv + 8), s3s_aes::load_be32(s->iv + 12)}};
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_CRYPT_OFF].p, h_q, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, ctx->stream));
    launch_aes_ctr_window(ctx->enc_keys, ctx->enc_rounds, iv0, d_comp, dev<uint8_t>(ctx, B_CRYPT), d_off, d_poff, d_iv, m, front, h_off[m], ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hs + o_iv, d_iv, 16 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (do_sum && n > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_REF_SUMS].p, h_seed, 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_checksum(ctx, s->algo, d_comp, d_off, n, h_seg, dev<int64_t>(ctx, B_SUMS), L))) return rc;
    launch_checksum_seed(s->algo, d_off, n, ctx->buf[B_TABLES].p, dev<int64_t>(ctx, B_REF_SUMS), dev<int64_t>(ctx, B_SUMS), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_sums, ctx->buf[B_SUMS].p, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  // the one-shot call reports a wrong checksum before a corrupt frame: so does a feed for the partitions whose last byte its
  // window holds (a corrupt frame in a partition that is still open comes first - nothing else is known about it yet)
  auto wrong_sum = [&]() -> int32_t {  // the first partition whose last byte the window holds and whose checksum is wrong, or -1
    if (do_sum)
      for (int32_t i = 0; i < n; i++)
        if (s->off[(size_t)(s->cur + i) + 1] <= wend && h_sums[i] != s->ref[(size_t)(s->cur + i)]) return s->cur + i;
    return -1;
  };
  auto corrupt = [&](const char* what) -> int {
    const int32_t bad = wrong_sum();
    return bad >= 0 ? stick(s, r, S3S_E_CHECKSUM, bad, "") : stick(s, r, S3S_E_BAD_FRAME, -1, what);
  };
  // discovery's status word: a unit that claims more decoded bytes than any decoder takes is refused, not corrupt - nothing is
  // consumed, need_dst stays 0 (never S3S_E_CAPACITY: the caller would be sent for up to 4 GiB), and the same feed gets the
  // same answer.  A wrong checksum of a partition whose last byte the window holds still comes first.
  auto refused = [&](int32_t st, const char* what) -> int {
    if (st != S3S_E_UNSUPPORTED) return corrupt(what);
    const int32_t bad = wrong_sum();
    if (bad >= 0) return stick(s, r, S3S_E_CHECKSUM, bad, "");
    if (codec == S3S_CODEC_ZSTD)
      return fail(ctx, S3S_E_UNSUPPORTED, "Zstandard frame outside the streaming contract (content checksum, dictionary id, window above "
                                          "1 << %d, or a skippable frame above 32 MiB)", s->wlog);
    return fail(ctx, S3S_E_UNSUPPORTED, "codec block larger than the decoder takes");
  };

  // ---- discovery: the whole units of the window, then the cut at dst_capacity -----------------------------------------------
  // (consumed and need_comp are plain offsets here; they are mapped back behind the cut)
  int64_t n_frames = 0, k = 0, consumed = PL, out_len = PL, need_comp = 0;
  int64_t z_open_after = 0, z_fu = -1, z_window = 0, z_start = 0;  // Zstandard: the frame open behind the last unit taken
  int64_t* d_zbase = nullptr;
  ZStreamRun zrun = {};
  if (codec == S3S_CODEC_NONE || PL == 0) {  // (no plain byte: the window holds IVs, whole or cut, and nothing else)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else if (codec == S3S_CODEC_ZSTD) {
    // the unit walk (counts, scan, units), the size pass over every block of the window - a compressed block's decoded size is
    // not in its header - the scan of the sizes and the cut: as for the other codecs, with one pass more
    const size_t cnt_bytes = al(sizeof(uint32_t) * n1);
    if ((rc = ensure(ctx, B_PART_NFRAMES, cnt_bytes + sizeof(int64_t) * (n1 + 1)))) return rc;
    uint32_t* d_cnt = dev<uint32_t>(ctx, B_PART_NFRAMES);
    d_zbase = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_PART_NFRAMES) + cnt_bytes);
    const int64_t wmax = (int64_t)1 << s->wlog;
    launch_zstd_walk(P, d_poff, pn, s->zopen ? 1 : 0, plast_pend, wmax, false, nullptr, d_cnt, nullptr, nullptr, d_status, d_result, ctx->stream);
    launch_scan_u32(d_cnt, pn, d_zbase, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&h_misc[0], d_zbase + pn, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&h_misc[2], d_result, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*reinterpret_cast<int32_t*>(&h_misc[1]) != 0) return refused(*reinterpret_cast<int32_t*>(&h_misc[1]), "frame or block header");
    n_frames = h_misc[0];
    const int64_t stop = h_misc[2];
    need_comp = h_misc[3];
    if (stop < 0 || stop > PL || (stop < PL && need_comp <= PL - stop)) return fail(ctx, S3S_E_HIP, "unit discovery returned an impossible stop offset");
    if (n_frames > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "too many units in one feed");
    k = 0;
    consumed = stop;
    out_len = 0;
    z_open_after = s->zopen ? 1 : 0;
    if (n_frames > 0) {
      if ((rc = ensure(ctx, B_FRAMES, sizeof(s3s_zstd::ZUnit) * (size_t)(n_frames + 1)))) return rc;
      if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * (size_t)(n_frames + 1)))) return rc;
      if ((rc = ensure(ctx, B_FRAME_OUT, sizeof(int64_t) * (size_t)(n_frames + 1)))) return rc;
      launch_zstd_walk(P, d_poff, pn, s->zopen ? 1 : 0, plast_pend, wmax, true, d_zbase, nullptr, ctx->buf[B_FRAMES].p,
                       dev<uint32_t>(ctx, B_ITEM_SIZE), d_status, d_result, ctx->stream);
      zrun.comp = P;
      zrun.units = dev<s3s_zstd::ZUnit>(ctx, B_FRAMES);
      zrun.dsize = dev<uint32_t>(ctx, B_ITEM_SIZE);
      zrun.unit_out = dev<int64_t>(ctx, B_FRAME_OUT);
      zrun.unit_base = d_zbase;
      zrun.k = n_frames;
      zrun.execute = 0;
      zrun.resumed = s->zopen ? 1 : 0;
      zrun.st_in = static_cast<const s3s_zstd::ZStreamState*>(s->zmem);
      zrun.st_out = nullptr;
      zrun.dst = d_dst;
      zrun.staging = nullptr;
      zrun.hist_len = s->zhist_len;
      zrun.lit = nullptr;
      zrun.lit_stride = 0;
      zrun.status = d_status;
      zrun.result = d_result + 8;
      launch_zstd_stream(zrun, pn, ctx->stream);  // the size pass: no stores but the sizes, the saved state is only read
      launch_scan_u32(dev<uint32_t>(ctx, B_ITEM_SIZE), n_frames, dev<int64_t>(ctx, B_FRAME_OUT), ctx->stream);
      launch_zstd_units_cut(P, ctx->buf[B_FRAMES].p, dev<uint32_t>(ctx, B_ITEM_SIZE), dev<int64_t>(ctx, B_FRAME_OUT), n_frames, dst_capacity,
                            stop, s->zopen ? 1 : 0, d_result, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[2], d_result, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      if (*reinterpret_cast<int32_t*>(&h_misc[1]) != 0) return refused(*reinterpret_cast<int32_t*>(&h_misc[1]), "block");
      k = h_misc[2];
      consumed = h_misc[3];
      out_len = h_misc[4];
      if (k < 0 || k > n_frames || consumed < 0 || consumed > stop || out_len < 0 || out_len > dst_capacity)
        return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible unit index");
      if (consumed == 0) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
        r->need_dst = h_misc[5];
        return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld decoded bytes of the next block", (long long)dst_capacity, (long long)h_misc[5]);
      }
      z_open_after = h_misc[6];
      z_fu = h_misc[7];
      z_window = h_misc[8];
      z_start = h_misc[9];
      if (z_open_after && z_fu >= 0 && (z_window < 0 || z_window > wmax || z_start < 0 || z_start > out_len))
        return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible open frame");
    }
  } else {
    const int cf = codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy;
    const int32_t n_tiles = codec == S3S_CODEC_LZ4 ? lz4_tile_count(PL) : 0;
    int64_t *d_true_entry = nullptr, *d_base = nullptr;
    if (codec == S3S_CODEC_LZ4) {
      const size_t tile_i64 = sizeof(int64_t) * (size_t)(n_tiles + 1);
      if ((rc = ensure(ctx, B_PART_NFRAMES, 4 * tile_i64 + sizeof(int32_t) * (size_t)(n_tiles + 1)))) return rc;
      int64_t* d_spec_entry = dev<int64_t>(ctx, B_PART_NFRAMES);
      int64_t* d_spec_exit = d_spec_entry + (n_tiles + 1);
      d_true_entry = d_spec_exit + (n_tiles + 1);
      d_base = d_true_entry + (n_tiles + 1);
      int32_t* d_spec_count = reinterpret_cast<int32_t*>(d_base + (n_tiles + 1));
      launch_lz4_discover_stream(P, PL, pleft, n_tiles, d_spec_entry, d_spec_exit, d_spec_count, d_true_entry, d_base, d_status,
                                 d_result, ctx->stream);
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[0], d_base + n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    } else {
      const size_t cnt_bytes = al(sizeof(uint32_t) * n1);
      if ((rc = ensure(ctx, B_PART_NFRAMES, cnt_bytes + sizeof(int64_t) * (n1 + 1)))) return rc;
      uint32_t* d_cnt = dev<uint32_t>(ctx, B_PART_NFRAMES);
      d_base = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_PART_NFRAMES) + cnt_bytes);
      launch_snappy_count_frames_stream(P, d_poff, pn, first_mid, plast_pend, d_cnt, d_status, d_result, ctx->stream, cf);
      launch_scan_u32(d_cnt, pn, d_base, ctx->stream);
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[0], d_base + pn, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&h_misc[2], d_result, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (*reinterpret_cast<int32_t*>(&h_misc[1]) != 0)
      return refused(*reinterpret_cast<int32_t*>(&h_misc[1]), codec == S3S_CODEC_LZ4 ? "frame chain" : "chunk chain");
    n_frames = h_misc[0];
    const int64_t stop = h_misc[2];
    need_comp = h_misc[3];
    if (stop < 0 || stop > PL || (stop < PL && need_comp <= PL - stop)) return fail(ctx, S3S_E_HIP, "frame discovery returned an impossible stop offset");
    if (n_frames > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "too many frames in one feed");
    k = 0;
    consumed = stop;
    out_len = 0;
    if (n_frames > 0) {
      if ((rc = ensure(ctx, B_FRAMES, sizeof(Frame) * (size_t)(n_frames + 1)))) return rc;
      if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * (size_t)(n_frames + 1)))) return rc;
      if ((rc = ensure(ctx, B_FRAME_OUT, sizeof(int64_t) * (size_t)(n_frames + 1)))) return rc;
      if (codec == S3S_CODEC_LZ4) {  // the one-shot emit, with the stop offset as the end of the bytes: the chain ends exactly there
        launch_lz4_emit_frames(P, stop, lz4_tile_count(stop), d_true_entry, d_base, dev<Frame>(ctx, B_FRAMES),
                               dev<uint32_t>(ctx, B_ITEM_SIZE), n_frames, dev<int64_t>(ctx, B_FRAME_OUT), d_status, ctx->stream);
      } else {
        launch_snappy_emit_frames_stream(P, d_poff, pn, first_mid, plast_pend, d_base, dev<Frame>(ctx, B_FRAMES),
                                         dev<uint32_t>(ctx, B_ITEM_SIZE), d_status, ctx->stream, cf);
        launch_scan_u32(dev<uint32_t>(ctx, B_ITEM_SIZE), n_frames, dev<int64_t>(ctx, B_FRAME_OUT), ctx->stream);
      }
      launch_frames_cut(codec, dev<Frame>(ctx, B_FRAMES), dev<uint32_t>(ctx, B_ITEM_SIZE), dev<int64_t>(ctx, B_FRAME_OUT), n_frames,
                        dst_capacity, stop, d_result, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[2], d_result, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      if (*reinterpret_cast<int32_t*>(&h_misc[1]) != 0) return refused(*reinterpret_cast<int32_t*>(&h_misc[1]), "frame header");
      k = h_misc[2];
      consumed = h_misc[3];
      out_len = h_misc[4];
      if (k < 0 || k > n_frames || consumed < 0 || consumed > stop || out_len < 0 || out_len > dst_capacity)
        return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible frame index");
      if (consumed == 0 && to_stored(0) == 0) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
        r->need_dst = h_misc[5];
        return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld decoded bytes of the next unit", (long long)dst_capacity, (long long)h_misc[5]);
      }
    }
  }

  if (enc) {  // back to the stored side
    if (short_part && consumed == PL) return corrupt("partition shorter than its IV");  // this feed would consume into it
    consumed = to_stored(consumed);
    if (consumed == 0 && iv_cut) need_comp = s3s_aes::kBlock;  // the window starts with a partition and shows less than its IV
  }

  // ---- the verdict of every partition whose last byte this feed consumes, before anything is decoded ---------------------
  const int64_t new_pos = s->pos + consumed;
  int32_t q = s->cur;
  for (; q < np && s->off[(size_t)q + 1] <= new_pos; q++)
    if (do_sum && h_sums[q - s->cur] != s->ref[(size_t)q]) return stick(s, r, S3S_E_CHECKSUM, q, "");
  // the state of the partition left open: known already unless the capacity cut ended the feed inside its piece
  int64_t carry = fresh(s->algo);
  bool second = false;
  if (do_sum && q < np) {
    const int32_t i = q - s->cur;
    const int64_t seed = i == 0 ? s->carry : fresh(s->algo);
    if (i >= n || consumed <= h_off[i]) carry = seed;
    else if (consumed == h_off[i + 1]) carry = h_sums[i];
    else {
      second = true;
      h_off2[0] = h_off[i];
      h_off2[1] = consumed;
      h_seg2[0] = 0;
      h_seg2[1] = worst_segs(consumed - h_off[i]);
      h_seed[n] = seed;
    }
  }

  // ---- decode the cut frame table with the one-shot path's decoders ----------------------------------------------------------
  if (codec == S3S_CODEC_NONE) {
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, P, (size_t)out_len, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else if (k > 0 || second) {
    ZNew z_new;
    if (k > 0 && codec == S3S_CODEC_ZSTD) {
      // the frame that was open decodes behind its saved history in a staging area, so that every offset it may use is there;
      // a frame that starts in this feed and stays open gets its memory now: a failure consumes nothing
      if (z_open_after && z_fu >= 0) {
        const size_t bytes = kZStateBytes + (size_t)(z_window > 0 ? z_window : 1);
        if (hipMalloc(&z_new.p, bytes) != hipSuccess) {
          (void)hipGetLastError();
          z_new.p = nullptr;
          r->consumed = r->out_len = 0;
          return fail(ctx, S3S_E_NOMEM, "hipMalloc(%zu) for the open frame's history failed", bytes);
        }
      }
      int64_t max_piece = 0;
      for (int32_t i = 0; i < pn; i++) max_piece = std::max(max_piece, h_off[i + 1] - h_off[i]);
      const int64_t by_size = 8 * max_piece + 256;
      const int64_t lit_stride = ((std::min<int64_t>(by_size, s3s_zstd::kMaxBlock) + 64) + 15) & ~int64_t(15);
      if ((rc = ensure(ctx, B_ZBLOCK_LIT, (size_t)lit_stride * (size_t)pn + 64))) return rc;
      if (s->zopen) {
        if ((rc = ensure(ctx, B_ZSCRATCH, (size_t)(s->zhist_len + out_len) + 256))) return rc;
        if (s->zhist_len > 0)
          HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_ZSCRATCH].p, static_cast<uint8_t*>(s->zmem) + kZStateBytes, (size_t)s->zhist_len,
                                      hipMemcpyDeviceToDevice, ctx->stream));
      }
      zrun.k = k;
      zrun.execute = 1;
      zrun.st_out = !z_open_after ? nullptr : static_cast<s3s_zstd::ZStreamState*>(z_fu >= 0 ? z_new.p : s->zmem);
      zrun.staging = s->zopen ? dev<uint8_t>(ctx, B_ZSCRATCH) : nullptr;
      zrun.lit = dev<uint8_t>(ctx, B_ZBLOCK_LIT);
      zrun.lit_stride = lit_stride;
      launch_zstd_stream(zrun, pn, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[10], d_result + 8, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    } else if (k > 0) {
      if (codec == S3S_CODEC_LZ4)
        launch_lz4_decompress(P, dev<Frame>(ctx, B_FRAMES), (int32_t)k, dev<int64_t>(ctx, B_FRAME_OUT), d_dst, d_status,
                              ctx->lz4_decode_variant, ctx->stream);
      else
        launch_snappy_decompress(P, dev<Frame>(ctx, B_FRAMES), (int32_t)k, dev<int64_t>(ctx, B_FRAME_OUT), d_dst, d_status,
                                 ctx->lz4_decode_variant, ctx->stream, codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy);
      HIP_TRY(ctx, hipGetLastError());
    }
    if (second) {
      HIP_TRY(ctx, hipMemcpyAsync(d_off + n1, h_off2, 16, hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(dev<int64_t>(ctx, B_REF_SUMS) + n, &h_seed[n], 8, hipMemcpyHostToDevice, ctx->stream));
      if ((rc = run_checksum(ctx, s->algo, d_comp, d_off + n1, 1, h_seg2, dev<int64_t>(ctx, B_SUMS) + n, L))) return rc;
      launch_checksum_seed(s->algo, d_off + n1, 1, ctx->buf[B_TABLES].p, dev<int64_t>(ctx, B_REF_SUMS) + n, dev<int64_t>(ctx, B_SUMS) + n,
                           ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&h_sums[n], dev<int64_t>(ctx, B_SUMS) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int32_t st = *reinterpret_cast<int32_t*>(&h_misc[1]);
    if (st == S3S_E_UNSUPPORTED && codec == S3S_CODEC_LZ4 && ctx->lz4_decode_variant != 3) {  // a frame above 32 MiB: the ring decoder, as in the one-shot call
      HIP_TRY(ctx, hipMemsetAsync(d_status, 0, 16, ctx->stream));
      launch_lz4_decompress(P, dev<Frame>(ctx, B_FRAMES), (int32_t)k, dev<int64_t>(ctx, B_FRAME_OUT), d_dst, d_status, 3, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      st = *reinterpret_cast<int32_t*>(&h_misc[1]);
    }
    if (st == S3S_E_UNSUPPORTED) return fail(ctx, S3S_E_UNSUPPORTED, "codec block larger than the decoder takes");
    if (st != 0) return corrupt("frame payload");  // (the capacity cut may have left a partition's end, which the window holds, unconsumed)
    if (second) carry = h_sums[n];
    if (k > 0 && codec == S3S_CODEC_ZSTD) {  // the resumed frame's bytes to dst, the open frame's last bytes to the stream
      const int64_t resumed_out = s->zopen ? h_misc[10] : 0;
      if (resumed_out < 0 || resumed_out > out_len || (z_open_after && z_fu < 0 && resumed_out != out_len))
        return fail(ctx, S3S_E_HIP, "the resumed frame reported an impossible size");
      const uint8_t* staging = dev<uint8_t>(ctx, B_ZSCRATCH);
      if (resumed_out > 0)
        HIP_TRY(ctx, hipMemcpyAsync(d_dst, staging + s->zhist_len, (size_t)resumed_out, hipMemcpyDeviceToDevice, ctx->stream));
      if (!z_open_after) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        zfree(s);
      } else if (z_fu < 0) {  // still the same frame
        const int64_t produced = s->zproduced + out_len, nh = std::min(s->zwindow, produced), end = s->zhist_len + out_len;
        if (nh > 0)
          HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(s->zmem) + kZStateBytes, staging + (end - nh), (size_t)nh, hipMemcpyDeviceToDevice,
                                      ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        s->zproduced = produced;
        s->zhist_len = nh;
      } else {  // a frame that started in this feed
        const int64_t produced = out_len - z_start, nh = std::min(z_window, produced);
        if (nh > 0)
          HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(z_new.p) + kZStateBytes, d_dst + (out_len - nh), (size_t)nh, hipMemcpyDeviceToDevice,
                                      ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        zfree(s);
        s->zmem = z_new.p;
        z_new.p = nullptr;
        s->zheld = (int64_t)(kZStateBytes + (size_t)(z_window > 0 ? z_window : 1));
        g_zheld += s->zheld;
        s->zopen = true;
        s->zwindow = z_window;
        s->zproduced = produced;
        s->zhist_len = nh;
      }
    }
  }

  if (enc && q < np && new_pos > s->off[(size_t)q] && !(q == s->cur && front > 0))  // the open partition's IV: it started in this window
    memcpy(s->iv, h_iv + 16 * (size_t)(q - s->cur), sizeof s->iv);
  s->pos = new_pos;
  s->cur = q;
  s->carry = carry;
  r->consumed = consumed;
  r->out_len = out_len;
  r->need_comp = consumed == 0 ? need_comp : 0;
  r->at_end = at_end(s);
  return S3S_OK;
}

int s3s_dstream_feed(s3s_dstream* s, const uint8_t* comp, int64_t comp_len, uint8_t* dst, int64_t dst_capacity, s3s_dstream_result* r) {
  if (!s || !r) return S3S_E_INVALID;
  s3s_ctx* ctx = s->ctx;
  ctx->err[0] = 0;
  if (comp_len < 0 || (comp_len > 0 && !comp) || dst_capacity < 0 || (dst_capacity > 0 && !dst)) {
    memset(r, 0, sizeof *r);
    r->bad_partition = -1;
    return fail(ctx, S3S_E_INVALID, "null/invalid host buffer");
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  // both device buffers are the context's workspace, sized by the window and by dst_capacity: the caller's two bounds
  if ((rc = ensure(ctx, B_SRC, (size_t)comp_len + 64))) return rc;
  if ((rc = ensure(ctx, B_DST, (size_t)dst_capacity + 64))) return rc;
  if (comp_len > 0 && s->err == S3S_OK)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_SRC].p, comp, (size_t)comp_len, hipMemcpyHostToDevice, ctx->stream));
  rc = s3s_dstream_feed_device(s, dev<uint8_t>(ctx, B_SRC), comp_len, dev<uint8_t>(ctx, B_DST), dst_capacity, r);
  if (rc != S3S_OK) return rc;
  if (r->out_len > 0) HIP_TRY(ctx, hipMemcpy(dst, ctx->buf[B_DST].p, (size_t)r->out_len, hipMemcpyDeviceToHost));
  return S3S_OK;
}

}  // extern "C"

// ---- the batched feed: one window of each of several streams per call ----------------------------------------------------
// The path of s3s_dstream_feed_device for plain LZ4 / Snappy / LZF streams with every kernel launched once per CALL
// (decode_stream_batch.hip) and the same three host waits whatever n is: checksums + discovery, frame tables + cut, decode.
// Every verdict is made on the host by the single feed's rules from the same device words, and NO stream's state is committed
// before the decode's verdict is known: when the batch's one decode status word comes back non-zero, the undecided entries go
// through the single feed one by one, which says whose it was - nothing was committed, so its answers are the single feed's.
namespace {

struct BatchWin {         // one entry that takes part in the batched path
  int32_t e;              // its index in the caller's array
  int32_t n;              // pieces of partitions in its window
  size_t piece0, seg0;    // its first piece / first checksum segment slot in the batch-wide lists (offsets: piece0 + its index)
  bool decided = false;   // it has its verdict and has left the batch
  int64_t n_frames = 0, stop = 0, first_frame = 0;
  int64_t k = 0, consumed = 0, out_len = 0, need_comp = 0;
  // the commit, made behind the decode's verdict
  int32_t q = 0;
  int64_t carry = 0;
  int32_t second = -1;    // its task in the second checksum launch (the cut ended the feed inside a piece), or -1
};

}  // namespace

extern "C" {

int s3s_dstream_feed_batch_device(s3s_ctx* ctx, s3s_dstream_feed_entry* E, int32_t n_entries) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  if (n_entries < 0 || (n_entries > 0 && !E)) return fail(ctx, S3S_E_INVALID, "null entry array or negative count");
  BatchVerdict<s3s_dstream_feed_entry> verdict(E, n_entries);
  if (n_entries == 0) return verdict.finish(S3S_OK);
  // ---- call-level refusals: nothing has been touched ---------------------------------------------------------------------
  bool plain = n_entries > 1 && !enc_on(ctx);
  {
    std::vector<const s3s_dstream*> seen;
    seen.reserve((size_t)n_entries);
    for (int32_t i = 0; i < n_entries; i++) {
      const s3s_dstream* s = E[i].stream;
      if (!s) return fail(ctx, S3S_E_INVALID, "entry %d: null stream", i);
      if (s->ctx != ctx) return fail(ctx, S3S_E_INVALID, "entry %d: the stream was opened on another context", i);
      if (s->codec != E[0].stream->codec || s->algo != E[0].stream->algo)
        return fail(ctx, S3S_E_INVALID, "entry %d: the streams of a batch must share codec and checksum algorithm", i);
      if (s->enc || s->wlog != 0 || s->codec == S3S_CODEC_NONE) plain = false;
      seen.push_back(s);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(ctx, S3S_E_INVALID, "the same stream twice in one batch");
  }
  auto single = [&](s3s_dstream_feed_entry& e) {
    e.status = s3s_dstream_feed_device(e.stream, e.d_comp, e.comp_len, e.d_dst, e.dst_capacity, &e.result);
  };
  auto first_error = [&]() -> int {
    for (int32_t i = 0; i < n_entries; i++)
      if (E[i].status != S3S_OK) {
        char msg[sizeof ctx->err];
        snprintf(msg, sizeof msg, "%s", ctx->err);
        return fail(ctx, E[i].status, "entry %d of the batch failed%s%.400s", i, msg[0] ? ": " : "", msg);
      }
    return S3S_OK;
  };
  if (!plain) {  // nothing to batch: one by one, in order
    for (int32_t i = 0; i < n_entries; i++) single(E[i]);
    return verdict.finish(first_error());
  }
  const int codec = E[0].stream->codec, algo = E[0].stream->algo;
  const bool do_sum = algo != S3S_CHECKSUM_NONE;
  const int cf = codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy;

  // ---- entries the single feed answers without device work keep its answer: a sticky error, an argument it refuses, an empty
  // window.  The others are the windows of the batch
  std::vector<BatchWin> W;
  W.reserve((size_t)n_entries);
  size_t P = 0, SG = 0;  // pieces and checksum segment slots of all windows
  int64_t T = 0;         // LZ4: tiles of all windows
  for (int32_t i = 0; i < n_entries; i++) {
    s3s_dstream_feed_entry& e = E[i];
    const s3s_dstream* s = e.stream;
    const int64_t left = s->off[(size_t)s->nparts] - s->pos;
    if (s->err != S3S_OK || e.comp_len <= 0 || e.dst_capacity < 0 || !e.d_comp || (e.dst_capacity > 0 && !e.d_dst) || e.comp_len > left) {
      single(e);
      continue;
    }
    BatchWin w;
    w.e = i;
    const int64_t wend = s->pos + e.comp_len;
    int32_t n = 0;
    while (s->cur + n < s->nparts && (s->off[(size_t)(s->cur + n)] < wend || s->off[(size_t)(s->cur + n) + 1] <= wend)) n++;
    w.n = n;
    w.piece0 = P;
    w.seg0 = SG;
    P += (size_t)n;
    for (int32_t p = 0; p < n; p++) {
      const int64_t a = std::max<int64_t>(s->off[(size_t)(s->cur + p)] - s->pos, 0), b = std::min(s->off[(size_t)(s->cur + p) + 1] - s->pos, e.comp_len);
      SG += (size_t)worst_segs(b - a);
    }
    if (codec == S3S_CODEC_LZ4) T += lz4_tile_count(e.comp_len);
    W.push_back(w);
  }
  const int32_t m = (int32_t)W.size();
  if (m == 0) return verdict.finish(first_error());
  if (P > 0x7fffff00ull || SG > 0x7fffff00ull || T > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "batch too large for one call");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& v : ctx->stage_ms) v = 0;

  // ---- one arena, host (pinned) and device, uploaded in one copy -----------------------------------------------------------
  // [offsets P + m][seeds P][seg_start P + m][piece -> window P][tile -> window T][tails m][windows: LzRange m][StreamWin m]
  // [second checksum launch: offsets 2 m | seeds m | seg_start 2 m | piece -> task m | tails m]
  auto al = [](size_t x) { return (x + 15) & ~size_t(15); };
  const size_t M = (size_t)m, PM = P + M;
  const size_t a_off = 0, a_seed = al(a_off + 8 * PM), a_seg = al(a_seed + 8 * (P + 1)), a_pw = al(a_seg + 4 * PM), a_tw = al(a_pw + 4 * (P + 1)),
               a_tail = al(a_tw + 4 * ((size_t)T + 1)), a_rng = al(a_tail + sizeof(TaskTail) * M), a_win = al(a_rng + sizeof(LzRange) * M),
               a_off2 = al(a_win + sizeof(StreamWin) * M), a_seed2 = al(a_off2 + 16 * M), a_seg2 = al(a_seed2 + 8 * M), a_pw2 = al(a_seg2 + 8 * M),
               a_tail2 = al(a_pw2 + 4 * M), a_total = al(a_tail2 + sizeof(TaskTail) * M);
  // downloads: [status words m + 1][result words kWinWords x m][sums P][second sums m]
  const size_t h_st_o = al(a_total), h_res_o = al(h_st_o + 4 * (M + 1)), h_sum_o = al(h_res_o + 8 * kWinWords * M), h_sum2_o = al(h_sum_o + 8 * (P + 1)),
               stage_total = al(h_sum2_o + 8 * M);
  int rc;
  if ((rc = ensure_stage(ctx, stage_total))) return rc;
  if ((rc = ensure(ctx, B_PLAN, a_total))) return rc;
  const size_t st_bytes = al(4 * (M + 1)), res_bytes = 8 * kWinWords * M;
  if ((rc = ensure(ctx, B_STATUS, st_bytes + res_bytes + 16))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * (P + M + 1)))) return rc;
  if ((rc = ensure(ctx, B_PARTIAL, 16 * (SG > 0 ? SG : 1)))) return rc;
  // discovery workspace per window: LZ4 4 x (tiles + 1) int64 + (tiles + 1) int32; Snappy / LZF (n + 1) int32 + (n + 2) int64
  std::vector<size_t> ws_off(M + 1);
  {
    size_t w = 0;
    for (size_t i = 0; i < M; i++) {
      ws_off[i] = w;
      const size_t c1 = codec == S3S_CODEC_LZ4 ? (size_t)lz4_tile_count(E[W[i].e].comp_len) + 1 : (size_t)W[i].n + 2;
      w += al(4 * 8 * c1 + 4 * c1);
    }
    ws_off[M] = w;
  }
  if ((rc = ensure(ctx, B_PART_NFRAMES, ws_off[M] + 16))) return rc;
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  uint8_t* da = dev<uint8_t>(ctx, B_PLAN);
  int64_t* h_off = reinterpret_cast<int64_t*>(hs + a_off);
  int64_t* h_seed = reinterpret_cast<int64_t*>(hs + a_seed);
  int32_t* h_seg = reinterpret_cast<int32_t*>(hs + a_seg);
  int32_t* h_pw = reinterpret_cast<int32_t*>(hs + a_pw);
  int32_t* h_tw = reinterpret_cast<int32_t*>(hs + a_tw);
  TaskTail* h_tail = reinterpret_cast<TaskTail*>(hs + a_tail);
  LzRange* h_rng = reinterpret_cast<LzRange*>(hs + a_rng);
  StreamWin* h_win = reinterpret_cast<StreamWin*>(hs + a_win);
  int64_t* h_off2 = reinterpret_cast<int64_t*>(hs + a_off2);
  int64_t* h_seed2 = reinterpret_cast<int64_t*>(hs + a_seed2);
  int32_t* h_seg2 = reinterpret_cast<int32_t*>(hs + a_seg2);
  int32_t* h_pw2 = reinterpret_cast<int32_t*>(hs + a_pw2);
  TaskTail* h_tail2 = reinterpret_cast<TaskTail*>(hs + a_tail2);
  int32_t* h_st = reinterpret_cast<int32_t*>(hs + h_st_o);
  int64_t* h_res = reinterpret_cast<int64_t*>(hs + h_res_o);
  int64_t* h_sums = reinterpret_cast<int64_t*>(hs + h_sum_o);
  int64_t* h_sums2 = reinterpret_cast<int64_t*>(hs + h_sum2_o);
  const LzRange* d_rng = reinterpret_cast<const LzRange*>(da + a_rng);
  const StreamWin* d_win = reinterpret_cast<const StreamWin*>(da + a_win);
  const int64_t* d_off = reinterpret_cast<const int64_t*>(da + a_off);
  const int32_t* d_pw = reinterpret_cast<const int32_t*>(da + a_pw);
  const int32_t* d_tw = reinterpret_cast<const int32_t*>(da + a_tw);
  int32_t* d_status = dev<int32_t>(ctx, B_STATUS);
  int64_t* d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + st_bytes);
  int64_t* d_sums = dev<int64_t>(ctx, B_SUMS);
  int32_t* d_dec_status = d_status + m;

  memset(hs + a_tail, 0, a_off2 - a_tail);
  int32_t tile0 = 0;
  for (int32_t wi = 0; wi < m; wi++) {
    BatchWin& w = W[(size_t)wi];
    const s3s_dstream_feed_entry& e = E[w.e];
    const s3s_dstream* s = e.stream;
    const int64_t L = e.comp_len;
    const size_t o0 = w.piece0 + (size_t)wi;  // the window's first offset
    int64_t segs = 0;
    for (int32_t p = 0; p < w.n; p++) {
      const int64_t a = s->off[(size_t)(s->cur + p)] - s->pos, b = s->off[(size_t)(s->cur + p) + 1] - s->pos;
      h_off[o0 + (size_t)p] = a < 0 ? 0 : a;
      h_off[o0 + (size_t)p + 1] = b < L ? b : L;
      h_seg[o0 + (size_t)p] = (int32_t)segs;
      segs += worst_segs(h_off[o0 + (size_t)p + 1] - h_off[o0 + (size_t)p]);
      h_seed[w.piece0 + (size_t)p] = p == 0 ? s->carry : fresh(algo);
      h_pw[w.piece0 + (size_t)p] = wi;
    }
    h_seg[o0 + (size_t)w.n] = (int32_t)segs;
    TaskTail& t = h_tail[wi];
    t.first_pp = (int32_t)o0;
    t.n_parts = w.n;
    t.first_part = (int32_t)w.piece0;
    t.first_seg = (int32_t)w.seg0;
    t.n_segs = (int32_t)segs;
    t.data = e.d_comp;
    t.data_len = L;
    LzRange& r = h_rng[wi];
    uint8_t* ws = dev<uint8_t>(ctx, B_PART_NFRAMES) + ws_off[(size_t)wi];
    const int32_t nt = codec == S3S_CODEC_LZ4 ? lz4_tile_count(L) : 0;
    const size_t c1 = codec == S3S_CODEC_LZ4 ? (size_t)nt + 1 : (size_t)w.n + 2;
    r.comp = e.d_comp;
    r.comp_len = L;
    r.n_tiles = nt;
    r.tile0 = tile0;
    r.spec_entry = reinterpret_cast<int64_t*>(ws);
    r.spec_exit = r.spec_entry + c1;
    r.true_entry = r.spec_exit + c1;
    r.frame_base = r.true_entry + c1;
    r.spec_count = reinterpret_cast<int32_t*>(r.frame_base + c1);
    r.status = d_status + wi;
    r.result = d_result + (size_t)kWinWords * (size_t)wi;
    r.dst_base = (int64_t)reinterpret_cast<uintptr_t>(e.d_dst);
    r.dst_capacity = e.dst_capacity;
    for (int32_t t2 = 0; t2 < nt; t2++) h_tw[tile0 + t2] = wi;
    tile0 += nt;
    StreamWin& x = h_win[wi];
    x.range_left = s->off[(size_t)s->nparts] - s->pos;
    x.last_pend = s->off[(size_t)(s->cur + w.n)] - s->pos;  // (>= L: the window cuts the last piece's partition, or ends with it)
    x.first_piece = (int32_t)w.piece0;
    x.n_pieces = w.n;
    x.first_mid = s->pos > s->off[(size_t)s->cur] ? 1 : 0;  // piece 0 starts inside a codec stream
  }

  // ---- phase 1: the checksums of every piece, seeded, and stream-mode discovery of every window; one wait -------------------
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, st_bytes + res_bytes, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(da, hs, a_off2, hipMemcpyHostToDevice, ctx->stream));
  record(ctx, 0);
  if (do_sum) {
    launch_checksum_batch(algo, reinterpret_cast<const TaskTail*>(da + a_tail), m, (int32_t)SG, (int32_t)P, d_off,
                          reinterpret_cast<const int32_t*>(da + a_seg), ctx->buf[B_TABLES].p, dev<uint32_t>(ctx, B_PARTIAL), d_sums, ctx->stream);
    launch_checksum_seed_batch(algo, d_off, d_pw, (int32_t)P, ctx->buf[B_TABLES].p, reinterpret_cast<const int64_t*>(da + a_seed), d_sums,
                               ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_sums, d_sums, 8 * P, hipMemcpyDeviceToHost, ctx->stream));
  }
  record(ctx, 1);
  if (codec == S3S_CODEC_LZ4) {
    launch_lz4_speculate_batch(d_rng, d_tw, (int32_t)T, ctx->stream);
    launch_lz4_resolve_stream_batch(d_rng, d_win, m, ctx->stream);
  } else {
    launch_snappy_count_stream_batch(d_rng, d_win, m, d_off, d_pw, (int32_t)P, cf, ctx->stream);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(h_st, d_status, st_bytes + res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

  // the single feed's verdicts, per window, from the same words
  auto wrong_sum = [&](const BatchWin& w) -> int32_t {  // the first partition whose last byte the window holds and whose checksum is wrong, or -1
    const s3s_dstream_feed_entry& e = E[w.e];
    const s3s_dstream* s = e.stream;
    if (do_sum)
      for (int32_t i = 0; i < w.n; i++)
        if (s->off[(size_t)(s->cur + i) + 1] <= s->pos + e.comp_len && h_sums[w.piece0 + (size_t)i] != s->ref[(size_t)(s->cur + i)]) return s->cur + i;
    return -1;
  };
  auto decide = [&](BatchWin& w, int status) {
    E[w.e].status = status;
    w.decided = true;
  };
  auto corrupt = [&](BatchWin& w, const char* what) {
    s3s_dstream_feed_entry& e = E[w.e];
    const int32_t bad = wrong_sum(w);
    decide(w, bad >= 0 ? stick(e.stream, &e.result, S3S_E_CHECKSUM, bad, "") : stick(e.stream, &e.result, S3S_E_BAD_FRAME, -1, what));
  };
  auto refused = [&](BatchWin& w, int32_t st, const char* what) {
    if (st != S3S_E_UNSUPPORTED) return corrupt(w, what);
    s3s_dstream_feed_entry& e = E[w.e];
    const int32_t bad = wrong_sum(w);
    decide(w, bad >= 0 ? stick(e.stream, &e.result, S3S_E_CHECKSUM, bad, "") : fail(ctx, S3S_E_UNSUPPORTED, "codec block larger than the decoder takes"));
  };
  const int64_t* h_words = h_res;  // (the status words and the result words come down in one copy: h_res_o = h_st_o + st_bytes)
  int64_t total_frames = 0;
  for (int32_t wi = 0; wi < m; wi++) {
    BatchWin& w = W[(size_t)wi];
    s3s_dstream_feed_entry& e = E[w.e];
    memset(&e.result, 0, sizeof e.result);
    e.result.bad_partition = -1;
    w.first_frame = total_frames;
    if (h_st[wi] != 0) {
      refused(w, h_st[wi], codec == S3S_CODEC_LZ4 ? "frame chain" : "chunk chain");
      continue;
    }
    const int64_t* res = h_words + (size_t)kWinWords * (size_t)wi;
    w.stop = res[0];
    w.need_comp = res[1];
    w.n_frames = res[2];
    if (w.stop < 0 || w.stop > e.comp_len || (w.stop < e.comp_len && w.need_comp <= e.comp_len - w.stop) || w.n_frames < 0) {
      decide(w, fail(ctx, S3S_E_HIP, "frame discovery returned an impossible stop offset"));
      w.n_frames = 0;
      continue;
    }
    if (w.n_frames > 0x7fffff00ll || total_frames + w.n_frames > 0x7fffff00ll) {
      decide(w, fail(ctx, S3S_E_UNSUPPORTED, "too many frames in one feed"));
      w.n_frames = 0;
      continue;
    }
    w.k = 0;
    w.consumed = w.stop;
    w.out_len = 0;
    total_frames += w.n_frames;
  }

  // ---- phase 2: the frame records of every window, the scan of its decoded sizes, its cut at its own dst_capacity; one wait ----
  if (total_frames > 0) {
    const size_t nf1 = (size_t)total_frames + M + 1;
    if ((rc = ensure(ctx, B_FRAMES, sizeof(Frame) * nf1))) return rc;
    if ((rc = ensure(ctx, B_ITEM_SIZE, 4 * nf1))) return rc;
    if ((rc = ensure(ctx, B_FRAME_OUT, 8 * nf1))) return rc;
    if ((rc = ensure(ctx, B_ITEM_OFF, 8 * nf1))) return rc;
    for (int32_t wi = 0; wi < m; wi++) {
      const BatchWin& w = W[(size_t)wi];
      LzRange& r = h_rng[wi];
      const int64_t f0 = w.first_frame;
      r.n_frames = w.decided ? 0 : w.n_frames;
      r.skip = w.decided ? 1 : 0;
      if (codec == S3S_CODEC_LZ4 && !w.decided) r.comp_len = w.stop;  // the one-shot emit, with the stop offset as the end of the bytes
      r.frames = dev<Frame>(ctx, B_FRAMES) + f0;
      r.frame_orig = dev<uint32_t>(ctx, B_ITEM_SIZE) + f0 + wi;
      r.frame_out = dev<int64_t>(ctx, B_FRAME_OUT) + f0 + wi;
      r.out_abs = dev<int64_t>(ctx, B_ITEM_OFF) + f0;
      h_win[wi].stop = w.stop;
      h_win[wi].first_frame = f0;
    }
    HIP_TRY(ctx, hipMemcpyAsync(da + a_rng, hs + a_rng, a_off2 - a_rng, hipMemcpyHostToDevice, ctx->stream));
    if (codec == S3S_CODEC_LZ4) launch_lz4_emit_batch(d_rng, d_tw, (int32_t)T, ctx->stream);
    else launch_snappy_emit_stream_batch(d_rng, d_win, m, d_off, d_pw, (int32_t)P, cf, ctx->stream);
    launch_frames_cut_batch(codec, d_rng, d_win, m, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_st, d_status, st_bytes + res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    record(ctx, 2);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  int32_t n_second = 0;
  bool any_decode = false;
  for (int32_t wi = 0; wi < m; wi++) {
    BatchWin& w = W[(size_t)wi];
    if (w.decided) continue;
    s3s_dstream_feed_entry& e = E[w.e];
    s3s_dstream* s = e.stream;
    if (w.n_frames > 0) {
      if (h_st[wi] != 0) {
        refused(w, h_st[wi], "frame header");
        continue;
      }
      const int64_t* res = h_words + (size_t)kWinWords * (size_t)wi;
      w.k = res[4];
      w.consumed = res[5];
      w.out_len = res[6];
      if (w.k < 0 || w.k > w.n_frames || w.consumed < 0 || w.consumed > w.stop || w.out_len < 0 || w.out_len > e.dst_capacity) {
        decide(w, fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible frame index"));
        continue;
      }
      if (w.consumed == 0) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
        e.result.need_dst = res[7];
        decide(w, fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld decoded bytes of the next unit", (long long)e.dst_capacity, (long long)res[7]));
        continue;
      }
    }
    // the verdict of every partition whose last byte this feed consumes, before anything is decoded
    const int64_t new_pos = s->pos + w.consumed;
    int32_t q = s->cur;
    bool bad = false;
    for (; q < s->nparts && s->off[(size_t)q + 1] <= new_pos; q++)
      if (do_sum && h_sums[w.piece0 + (size_t)(q - s->cur)] != s->ref[(size_t)q]) {
        decide(w, stick(s, &e.result, S3S_E_CHECKSUM, q, ""));
        bad = true;
        break;
      }
    if (bad) continue;
    // the state of the partition left open: known already unless the capacity cut ended the feed inside its piece
    w.q = q;
    w.carry = fresh(algo);
    if (do_sum && q < s->nparts) {
      const int32_t i = q - s->cur;
      const int64_t seed = i == 0 ? s->carry : fresh(algo);
      const int64_t* po = h_off + w.piece0 + (size_t)wi;
      if (i >= w.n || w.consumed <= po[i]) w.carry = seed;
      else if (w.consumed == po[i + 1]) w.carry = h_sums[w.piece0 + (size_t)i];
      else {
        const int32_t t = n_second++;
        w.second = t;
        h_off2[2 * t] = po[i];
        h_off2[2 * t + 1] = w.consumed;
        h_seg2[2 * t] = 0;
        h_seg2[2 * t + 1] = worst_segs(w.consumed - po[i]);
        h_seed2[t] = seed;
        h_pw2[t] = t;
        TaskTail& tt = h_tail2[t];
        memset(&tt, 0, sizeof tt);
        tt.first_pp = 2 * t;
        tt.n_parts = 1;
        tt.first_part = t;
        tt.n_segs = h_seg2[2 * t + 1];
        tt.data = e.d_comp;
        tt.data_len = e.comp_len;
      }
    }
    if (w.k > 0) any_decode = true;
  }

  // ---- phase 3: one decode launch over the frames of all windows in front of their cuts; one wait ---------------------------
  if (any_decode || n_second > 0) {
    if (any_decode) {
      for (int32_t wi = 0; wi < m; wi++) h_rng[wi].skip = W[(size_t)wi].decided ? 1 : 0;
      HIP_TRY(ctx, hipMemcpyAsync(da + a_rng, hs + a_rng, sizeof(LzRange) * M, hipMemcpyHostToDevice, ctx->stream));
      launch_frames_rebase_cut(d_rng, d_win, m, total_frames, ctx->stream);
      if (codec == S3S_CODEC_LZ4)
        launch_lz4_decompress(nullptr, dev<Frame>(ctx, B_FRAMES), (int32_t)total_frames, dev<int64_t>(ctx, B_ITEM_OFF), nullptr, d_dec_status,
                              ctx->lz4_decode_variant, ctx->stream);
      else
        launch_snappy_decompress(nullptr, dev<Frame>(ctx, B_FRAMES), (int32_t)total_frames, dev<int64_t>(ctx, B_ITEM_OFF), nullptr, d_dec_status,
                                 ctx->lz4_decode_variant, ctx->stream, cf);
      HIP_TRY(ctx, hipGetLastError());
    }
    if (n_second > 0) {  // the pieces the cuts left open, summed up to the cut: one launch for all of them
      int32_t seg0 = 0;
      for (int32_t t = 0; t < n_second; t++) {
        h_tail2[t].first_seg = seg0;
        seg0 += h_tail2[t].n_segs;
      }
      HIP_TRY(ctx, hipMemcpyAsync(da + a_off2, hs + a_off2, a_total - a_off2, hipMemcpyHostToDevice, ctx->stream));
      launch_checksum_batch(algo, reinterpret_cast<const TaskTail*>(da + a_tail2), n_second, seg0, n_second,
                            reinterpret_cast<const int64_t*>(da + a_off2), reinterpret_cast<const int32_t*>(da + a_seg2), ctx->buf[B_TABLES].p,
                            dev<uint32_t>(ctx, B_PARTIAL), d_sums + P, ctx->stream);
      launch_checksum_seed_batch(algo, reinterpret_cast<const int64_t*>(da + a_off2), reinterpret_cast<const int32_t*>(da + a_pw2), n_second,
                                 ctx->buf[B_TABLES].p, reinterpret_cast<const int64_t*>(da + a_seed2), d_sums + P, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(h_sums2, d_sums + P, 8 * (size_t)n_second, hipMemcpyDeviceToHost, ctx->stream));
    }
    record(ctx, 3);
    HIP_TRY(ctx, hipMemcpyAsync(&h_st[m], d_dec_status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->profile) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[3]) == hipSuccess) ctx->stage_ms[S3S_STAGE_TOTAL] = ms;
      if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->stage_ms[S3S_STAGE_CHECKSUM] = ms;
      if (total_frames > 0 && hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]) == hipSuccess) ctx->stage_ms[S3S_STAGE_DISCOVER] = ms;
      if (total_frames > 0 && hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->stage_ms[S3S_STAGE_CODEC] = ms;
    }
    if (any_decode && h_st[m] != 0) {
      // some frame of the batch is corrupt, or an LZ4 frame is above 32 MiB: nothing was committed, so the single feed answers
      // for every undecided entry (and runs the ring decoder where that is what the frame needs)
      std::vector<int32_t> todo;
      for (const BatchWin& w : W)
        if (!w.decided) todo.push_back(w.e);
      for (int32_t i : todo) single(E[i]);
      return verdict.finish(first_error());
    }
  }

  // ---- commit -------------------------------------------------------------------------------------------------------------
  for (BatchWin& w : W) {
    if (w.decided) continue;
    s3s_dstream_feed_entry& e = E[w.e];
    s3s_dstream* s = e.stream;
    s->pos += w.consumed;
    s->cur = w.q;
    s->carry = w.second >= 0 ? h_sums2[w.second] : w.carry;
    e.result.consumed = w.consumed;
    e.result.out_len = w.out_len;
    e.result.need_comp = w.consumed == 0 ? w.need_comp : 0;
    e.result.at_end = at_end(s);
    e.status = S3S_OK;
  }
  return verdict.finish(first_error());
}

int s3s_dstream_feed_batch(s3s_ctx* ctx, s3s_dstream_feed_entry* E, int32_t n_entries) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  if (n_entries < 0 || (n_entries > 0 && !E)) return fail(ctx, S3S_E_INVALID, "null entry array or negative count");
  BatchVerdict<s3s_dstream_feed_entry> verdict(E, n_entries);
  if (n_entries == 0) return verdict.finish(S3S_OK);
  // the windows and the destinations of ALL entries are staged in the context's workspace: the sum of comp_len + dst_capacity
  // is the caller's memory bound.  An entry the single feed refuses by its arguments is staged as empty and keeps them
  auto al = [](int64_t x) { return (x + 255) & ~int64_t(255); };
  std::vector<s3s_dstream_feed_entry> D(E, E + n_entries);
  std::vector<int64_t> so((size_t)n_entries), dso((size_t)n_entries);
  int64_t src_total = 0, dst_total = 0;
  for (int32_t i = 0; i < n_entries; i++) {
    const s3s_dstream_feed_entry& e = E[i];
    const bool ok = e.comp_len >= 0 && e.dst_capacity >= 0 && (e.comp_len == 0 || e.d_comp) && (e.dst_capacity == 0 || e.d_dst);
    so[(size_t)i] = src_total;
    dso[(size_t)i] = dst_total;
    if (ok) {
      src_total += al(e.comp_len + 64);
      dst_total += al(e.dst_capacity + 64);
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, B_SRC, (size_t)src_total + 64))) return rc;
  if ((rc = ensure(ctx, B_DST, (size_t)dst_total + 64))) return rc;
  for (int32_t i = 0; i < n_entries; i++) {
    const s3s_dstream_feed_entry& e = E[i];
    const bool ok = e.comp_len >= 0 && e.dst_capacity >= 0 && (e.comp_len == 0 || e.d_comp) && (e.dst_capacity == 0 || e.d_dst);
    if (!ok) {  // the device form's single feed answers S3S_E_INVALID from the same arguments (a null pointer stays null)
      D[(size_t)i].d_comp = e.d_comp ? dev<uint8_t>(ctx, B_SRC) : nullptr;
      D[(size_t)i].d_dst = e.d_dst ? dev<uint8_t>(ctx, B_DST) : nullptr;
      continue;
    }
    D[(size_t)i].d_comp = dev<uint8_t>(ctx, B_SRC) + so[(size_t)i];
    D[(size_t)i].d_dst = dev<uint8_t>(ctx, B_DST) + dso[(size_t)i];
    if (e.comp_len > 0 && e.stream && e.stream->err == S3S_OK)
      HIP_TRY(ctx, hipMemcpyAsync(dev<uint8_t>(ctx, B_SRC) + so[(size_t)i], e.d_comp, (size_t)e.comp_len, hipMemcpyHostToDevice, ctx->stream));
  }
  rc = s3s_dstream_feed_batch_device(ctx, D.data(), n_entries);
  for (int32_t i = 0; i < n_entries; i++) {
    E[i].result = D[(size_t)i].result;
    E[i].status = D[(size_t)i].status;
  }
  for (int32_t i = 0; i < n_entries; i++)
    if (E[i].status == S3S_OK && E[i].result.out_len > 0)
      HIP_TRY(ctx, hipMemcpyAsync(E[i].d_dst, D[(size_t)i].d_dst, (size_t)E[i].result.out_len, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return verdict.finish(rc);
}

}  // extern "C"
