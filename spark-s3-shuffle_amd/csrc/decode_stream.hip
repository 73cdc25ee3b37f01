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
//
// The host's RULES - the pieces of a window, the plain side, whether a kernel's words can be true, the verdicts, the open
// partition's carry, the commit - are decode_stream_core.h (namespace s3s_ds; no HIP, tested on the CPU).  This file holds
// what needs the context: staging, launches, waits, the sticky state and the error texts.  s3s_dstream_feed_device is the
// list of a feed's phases; s3s_dstream_feed_batch_device runs the same rules per window around launches made once per call,
// the decrypt pass of encrypted windows included (aes_ctr_stream_batch.hip).
#include <algorithm>
#include <atomic>
#include <new>

#define S3S_AES_DEVICE
#include "aes_ctr_core.h"
#include "decode_stream_core.h"
#include "s3s_ctx.h"
#include "zstd_decode_stream.h"

using namespace s3s;
namespace ds = s3s_ds;

static_assert(ds::kCodecNone == S3S_CODEC_NONE && ds::kCodecLz4 == S3S_CODEC_LZ4 && ds::kCodecSnappy == S3S_CODEC_SNAPPY &&
              ds::kCodecZstd == S3S_CODEC_ZSTD && ds::kCodecLzf == S3S_CODEC_LZF && ds::kSumNone == S3S_CHECKSUM_NONE &&
              ds::kSumAdler32 == S3S_CHECKSUM_ADLER32 && ds::kOk == S3S_OK && ds::kBadFrame == S3S_E_BAD_FRAME &&
              ds::kChecksum == S3S_E_CHECKSUM && ds::kUnsupported == S3S_E_UNSUPPORTED && ds::kIv == s3s_aes::kBlock,
              "decode_stream_core.h restates these");

struct s3s_dstream {
  s3s_ctx* ctx;
  int codec, algo;
  int32_t nparts;
  std::vector<int64_t> off, ref;  // part_offsets[nparts + 1], ref_checksums[nparts] (copies)
  ds::Pos at;                     // pos: bytes of the range consumed; partitions [0, cur) are verified, partition cur is open;
                                  // carry: checksum state of partition cur over [off[cur], pos)
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

inline ds::Range range_of(const s3s_dstream* s) {
  return {s->off.data(), s->ref.data(), s->enc ? s->poff.data() : nullptr, s->nparts, s->algo};
}

inline bool at_end(const s3s_dstream* s) { return ds::at_end(range_of(s), s->at); }

inline size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

// ---- the answers both feeds give, each text once -----------------------------------------------------------------------------
int stick(s3s_dstream* s, s3s_dstream_result* r, int code, int32_t bad_partition, const char* what) {
  s->err = code;
  s->bad_partition = bad_partition;
  r->consumed = r->out_len = 0;
  r->bad_partition = bad_partition;
  if (code == S3S_E_CHECKSUM) return fail(s->ctx, code, "Invalid checksum detected for partition %d of the range", bad_partition);
  return fail(s->ctx, code, "Stream is corrupted (%s, range offset %lld)", what, (long long)s->at.pos);
}

int too_large(s3s_ctx* ctx) { return fail(ctx, S3S_E_UNSUPPORTED, "codec block larger than the decoder takes"); }

// ds::refusal's verdict carried out: a wrong checksum and corruption stick, a refusal does not
int refuse(s3s_dstream* s, s3s_dstream_result* r, ds::Refusal v, const char* what) {
  if (v.code != S3S_E_UNSUPPORTED) return stick(s, r, v.code, v.bad, what);
  if (s->codec == S3S_CODEC_ZSTD)
    return fail(s->ctx, S3S_E_UNSUPPORTED, "Zstandard frame outside the streaming contract (content checksum, dictionary id, window above "
                                           "1 << %d, or a skippable frame above 32 MiB)", s->wlog);
  return too_large(s->ctx);
}

int bad_stop(s3s_ctx* ctx, const char* unit) { return fail(ctx, S3S_E_HIP, "%s discovery returned an impossible stop offset", unit); }
int too_many(s3s_ctx* ctx, const char* unit) { return fail(ctx, S3S_E_UNSUPPORTED, "too many %ss in one feed", unit); }
int bad_cut(s3s_ctx* ctx, const char* unit) { return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible %s index", unit); }
// the first unit does not fit dst: nothing is taken, the stream stays usable
int no_room(s3s_ctx* ctx, s3s_dstream_result* r, int64_t cap, int64_t need, const char* unit) {
  r->need_dst = need;
  return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld decoded bytes of the next %s", (long long)cap, (long long)need, unit);
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
  s->at.carry = ds::fresh(checksum_algo);
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

// ---- the single feed, phase by phase --------------------------------------------------------------------------------------------
// What the phases hand on: the staging pointers and the window's numbers
struct Feed {
  s3s_dstream* s;
  s3s_ctx* ctx;
  s3s_dstream_result* r;
  const uint8_t* d_comp;
  uint8_t* d_dst;
  int64_t cap;
  ds::Range R;
  int64_t L = 0;  // stored bytes this feed looks at
  int32_t n = 0;  // pieces of partitions in [pos, pos + L)
  size_t n1 = 1;
  // pinned staging (feed_layout)
  int64_t *h_off = nullptr, *h_off2 = nullptr, *h_seed = nullptr, *h_q = nullptr, *h_c = nullptr;
  int32_t *h_seg = nullptr, *h_seg2 = nullptr;
  int64_t* h_sums = nullptr;  // [n] = the second launch's sum
  int64_t* h_misc = nullptr;  // [0] n_frames, [1] status, [2..5] stop, need / k, consumed, out_len, need; Zstandard: [6..9] open, frame unit, window, out start, [10] resumed bytes
  uint8_t* h_iv = nullptr;
  ds::Plain pl;
  // device
  int64_t* d_off = nullptr;
  const uint8_t* P = nullptr;       // the plain bytes of the window
  const int64_t* d_poff = nullptr;  // ... and their pieces
  int32_t* d_status = nullptr;
  int64_t* d_result = nullptr;
  // discovery's answer (consumed and need_comp are plain offsets until feed_verdict maps them back)
  int64_t n_frames = 0, k = 0, consumed = 0, out_len = 0, need_comp = 0;
  int64_t z_open_after = 0, z_fu = -1, z_window = 0, z_start = 0;  // Zstandard: the frame open behind the last unit taken
  ZStreamRun zrun = {};
  // the verdict
  int32_t q = 0;  // the partition left open
  ds::Carry carry = {ds::Carry::kSeed, 0, 0, 0};

  int32_t status() const { return *reinterpret_cast<const int32_t*>(&h_misc[1]); }
  int corrupt(const char* what) { return refuse(s, r, ds::refusal(R, s->at, L, n, h_sums, S3S_E_BAD_FRAME), what); }
  int refused(const char* what) { return refuse(s, r, ds::refusal(R, s->at, L, n, h_sums, status()), what); }
};

// the sticky state and the arguments
int feed_check(s3s_dstream* s, const uint8_t* d_comp, int64_t comp_len, uint8_t* d_dst, int64_t dst_capacity, s3s_dstream_result* r) {
  s3s_ctx* ctx = s->ctx;
  ctx->err[0] = 0;
  memset(r, 0, sizeof *r);
  r->bad_partition = -1;
  if (s->err != S3S_OK) {
    r->bad_partition = s->bad_partition;
    return fail(ctx, s->err, "the stream failed in an earlier feed (%s)", s->err == S3S_E_CHECKSUM ? "Invalid checksum detected" : "Stream is corrupted");
  }
  const int64_t left = s->off[(size_t)s->nparts] - s->at.pos;
  if (comp_len < 0 || dst_capacity < 0 || (comp_len > 0 && !d_comp) || (dst_capacity > 0 && !d_dst))
    return fail(ctx, S3S_E_INVALID, "null/invalid argument");
  if (comp_len > left) return fail(ctx, S3S_E_INVALID, "the window reaches %lld bytes past the end of the range", (long long)(comp_len - left));
  if (s->enc && (s->epoch != ctx->enc_epoch || !enc_on(ctx)))  // bound to the key setting it was opened under: it can only be closed
    return fail(ctx, S3S_E_INVALID, "s3s_set_io_encryption was called on the context after the stream was opened");
  if (!s->enc && enc_on(ctx)) return fail(ctx, S3S_E_UNSUPPORTED, "IO encryption was switched on after the stream was opened");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& v : ctx->stage_ms) v = 0;
  return S3S_OK;
}

// nothing to look at: the position may still pass empty partitions
int feed_empty(Feed& f) {
  s3s_dstream* s = f.s;
  const int32_t bad = ds::pass_empty(f.R, s->at);
  if (bad >= 0) return stick(s, f.r, S3S_E_CHECKSUM, bad, "");
  f.r->at_end = at_end(s);
  if (f.R.total() > s->at.pos) f.r->need_comp = ds::min_unit(f.R, s->at, s->codec, s->zopen);
  return S3S_OK;
}

// the staging area, the window's pieces and its plain side, the device buffers
int feed_layout(Feed& f) {
  s3s_dstream* s = f.s;
  s3s_ctx* ctx = f.ctx;
  const bool enc = s->enc;
  const int32_t n = f.n = ds::piece_count(f.R, s->at, f.L);
  // pinned staging: [piece offsets n + 1][second-launch offsets 2][seg_start n + 1][second seg_start 2][seeds n + 1][sums n + 1][misc 8]
  const size_t n1 = f.n1 = (size_t)n + 1;
  const size_t o_off2 = al16(8 * n1), o_seg = al16(o_off2 + 16), o_seg2 = al16(o_seg + 4 * n1), o_seed = al16(o_seg2 + 8),
               o_sums = al16(o_seed + 8 * n1), o_misc = al16(o_sums + 8 * n1),
               // encrypted: [plain piece offsets n + 1][first cipher byte of every piece n + 1][the IVs that start in the window n + 1]
               o_q = al16(o_misc + 128), o_c = al16(o_q + 8 * n1), o_iv = al16(o_c + 8 * n1), stage_total = enc ? o_iv + 16 * n1 : o_misc + 128;
  int rc;
  if ((rc = ensure_stage(ctx, stage_total))) return rc;
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  f.h_off = reinterpret_cast<int64_t*>(hs);
  f.h_off2 = reinterpret_cast<int64_t*>(hs + o_off2);
  f.h_seg = reinterpret_cast<int32_t*>(hs + o_seg);
  f.h_seg2 = reinterpret_cast<int32_t*>(hs + o_seg2);
  f.h_seed = reinterpret_cast<int64_t*>(hs + o_seed);
  f.h_sums = reinterpret_cast<int64_t*>(hs + o_sums);
  f.h_misc = reinterpret_cast<int64_t*>(hs + o_misc);
  f.h_q = reinterpret_cast<int64_t*>(hs + o_q);
  f.h_c = reinterpret_cast<int64_t*>(hs + o_c);
  f.h_iv = hs + o_iv;
  if (ds::fill_pieces(f.R, s->at, f.L, n, kChecksumSegBytes, f.h_off, f.h_seg, f.h_seed) > ds::kMaxCount)
    return fail(ctx, S3S_E_UNSUPPORTED, "window too large for one feed");
  f.pl = ds::plain_side(f.R, s->at, f.L, n, f.h_off, f.h_q, f.h_c);
  // device: B_OFFSETS [piece offsets n + 1][2], B_REF_SUMS [seeds n + 1], B_SUMS [n + 1], B_STATUS [status][pad][result 9 x int64]
  if ((rc = ensure(ctx, B_OFFSETS, 8 * (n1 + 2)))) return rc;
  if ((rc = ensure(ctx, B_REF_SUMS, 8 * n1))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * n1))) return rc;
  if ((rc = ensure(ctx, B_STATUS, 128))) return rc;
  f.P = f.d_comp;
  if (enc) {  // device: B_CRYPT [the window decrypted], B_CRYPT_OFF [plain piece offsets n + 1][IVs n + 1]
    if ((rc = ensure(ctx, B_CRYPT, (size_t)f.pl.PL + 64))) return rc;
    if ((rc = ensure(ctx, B_CRYPT_OFF, 24 * n1))) return rc;
    f.P = dev<uint8_t>(ctx, B_CRYPT);
  }
  f.d_off = dev<int64_t>(ctx, B_OFFSETS);
  f.d_poff = enc ? dev<int64_t>(ctx, B_CRYPT_OFF) : f.d_off;
  f.d_status = dev<int32_t>(ctx, B_STATUS);
  f.d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + 16);
  return S3S_OK;
}

// queued in front of discovery: the decrypt pass and the checksums of every piece; their words arrive with the first wait
int feed_queue(Feed& f) {
  s3s_dstream* s = f.s;
  s3s_ctx* ctx = f.ctx;
  const int32_t n = f.n, m = f.pl.m;
  int rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, 128, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_off, f.h_off, 8 * f.n1, hipMemcpyHostToDevice, ctx->stream));
  if (s->enc && m > 0 && f.h_off[m] > 0) {
    uint8_t* d_iv = dev<uint8_t>(ctx, B_CRYPT_OFF) + 8 * f.n1;
    const AesWindowIv iv0 = {{s3s_aes::load_be32(s->iv), s3s_aes::load_be32(s->iv + 4), s3s_aes::load_be32(s->iv + 8), s3s_aes::load_be32(s->iv + 12)}};
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_CRYPT_OFF].p, f.h_q, 8 * ((size_t)m + 1), hipMemcpyHostToDevice, ctx->stream));
    launch_aes_ctr_window(ctx->enc_keys, ctx->enc_rounds, iv0, f.d_comp, dev<uint8_t>(ctx, B_CRYPT), f.d_off, f.d_poff, d_iv, m, f.pl.front, f.h_off[m], ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(f.h_iv, d_iv, 16 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (f.R.sums() && n > 0) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_REF_SUMS].p, f.h_seed, 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_checksum(ctx, s->algo, f.d_comp, f.d_off, n, f.h_seg, dev<int64_t>(ctx, B_SUMS), f.L))) return rc;
    launch_checksum_seed(s->algo, f.d_off, n, ctx->buf[B_TABLES].p, dev<int64_t>(ctx, B_REF_SUMS), dev<int64_t>(ctx, B_SUMS), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(f.h_sums, ctx->buf[B_SUMS].p, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  }
  return S3S_OK;
}

// the first wait: discovery's status word, the units in front of the stop (d_count), the stop offset and what the unit there needs
int discovery_answer(Feed& f, const int64_t* d_count, const char* what, const char* unit, int64_t* stop) {
  s3s_ctx* ctx = f.ctx;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[0], d_count, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[1], f.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[2], f.d_result, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (f.status() != 0) return f.refused(what);
  f.n_frames = f.h_misc[0];
  *stop = f.h_misc[2];
  f.need_comp = f.h_misc[3];
  if (!ds::stop_valid(*stop, f.need_comp, f.pl.PL)) return bad_stop(ctx, unit);
  if (f.n_frames > ds::kMaxCount) return too_many(ctx, unit);
  f.k = 0;
  f.consumed = *stop;
  f.out_len = 0;
  return S3S_OK;
}

// the second wait: the cut's status word and `words` result words
int cut_answer(Feed& f, int words, int64_t stop, const char* what, const char* unit, const char* unit_of_dst) {
  s3s_ctx* ctx = f.ctx;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[1], f.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[2], f.d_result, (size_t)words * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (f.status() != 0) return f.refused(what);
  f.k = f.h_misc[2];
  f.consumed = f.h_misc[3];
  f.out_len = f.h_misc[4];
  if (!ds::cut_valid(f.k, f.consumed, f.out_len, f.n_frames, stop, f.cap)) return bad_cut(ctx, unit);
  if (ds::nothing_fits(f.pl, f.consumed)) return no_room(ctx, f.r, f.cap, f.h_misc[5], unit_of_dst);
  return S3S_OK;
}

int ensure_frame_tables(s3s_ctx* ctx, size_t record_bytes, int64_t n_frames) {
  int rc;
  if ((rc = ensure(ctx, B_FRAMES, record_bytes * (size_t)(n_frames + 1)))) return rc;
  if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * (size_t)(n_frames + 1)))) return rc;
  return ensure(ctx, B_FRAME_OUT, sizeof(int64_t) * (size_t)(n_frames + 1));
}

// Zstandard: the unit walk (counts, scan, units), the size pass over every block of the window - a compressed block's decoded
// size is not in its header - the scan of the sizes and the cut: as for the other codecs, with one pass more
int feed_discover_zstd(Feed& f) {
  s3s_dstream* s = f.s;
  s3s_ctx* ctx = f.ctx;
  const int32_t pn = f.pl.m;
  const int resumed = s->zopen ? 1 : 0;
  int rc;
  const size_t cnt_bytes = al16(sizeof(uint32_t) * f.n1);
  if ((rc = ensure(ctx, B_PART_NFRAMES, cnt_bytes + sizeof(int64_t) * (f.n1 + 1)))) return rc;
  uint32_t* d_cnt = dev<uint32_t>(ctx, B_PART_NFRAMES);
  int64_t* d_zbase = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_PART_NFRAMES) + cnt_bytes);
  const int64_t wmax = (int64_t)1 << s->wlog;
  launch_zstd_walk(f.P, f.d_poff, pn, resumed, f.pl.plast_pend, wmax, false, nullptr, d_cnt, nullptr, nullptr, f.d_status, f.d_result, ctx->stream);
  launch_scan_u32(d_cnt, pn, d_zbase, ctx->stream);
  int64_t stop;
  if ((rc = discovery_answer(f, d_zbase + pn, "frame or block header", "unit", &stop))) return rc;
  f.z_open_after = resumed;
  if (f.n_frames == 0) return S3S_OK;
  if ((rc = ensure_frame_tables(ctx, sizeof(s3s_zstd::ZUnit), f.n_frames))) return rc;
  launch_zstd_walk(f.P, f.d_poff, pn, resumed, f.pl.plast_pend, wmax, true, d_zbase, nullptr, ctx->buf[B_FRAMES].p,
                   dev<uint32_t>(ctx, B_ITEM_SIZE), f.d_status, f.d_result, ctx->stream);
  ZStreamRun& zrun = f.zrun;
  zrun.comp = f.P;
  zrun.units = dev<s3s_zstd::ZUnit>(ctx, B_FRAMES);
  zrun.dsize = dev<uint32_t>(ctx, B_ITEM_SIZE);
  zrun.unit_out = dev<int64_t>(ctx, B_FRAME_OUT);
  zrun.unit_base = d_zbase;
  zrun.k = f.n_frames;
  zrun.execute = 0;
  zrun.resumed = resumed;
  zrun.st_in = static_cast<const s3s_zstd::ZStreamState*>(s->zmem);
  zrun.st_out = nullptr;
  zrun.dst = f.d_dst;
  zrun.staging = nullptr;
  zrun.hist_len = s->zhist_len;
  zrun.lit = nullptr;
  zrun.lit_stride = 0;
  zrun.status = f.d_status;
  zrun.result = f.d_result + 8;
  launch_zstd_stream(zrun, pn, ctx->stream);  // the size pass: no stores but the sizes, the saved state is only read
  launch_scan_u32(dev<uint32_t>(ctx, B_ITEM_SIZE), f.n_frames, dev<int64_t>(ctx, B_FRAME_OUT), ctx->stream);
  launch_zstd_units_cut(f.P, ctx->buf[B_FRAMES].p, dev<uint32_t>(ctx, B_ITEM_SIZE), dev<int64_t>(ctx, B_FRAME_OUT), f.n_frames, f.cap, stop,
                        resumed, f.d_result, ctx->stream);
  if ((rc = cut_answer(f, 8, stop, "block", "unit", "block"))) return rc;
  f.z_open_after = f.h_misc[6];
  f.z_fu = f.h_misc[7];
  f.z_window = f.h_misc[8];
  f.z_start = f.h_misc[9];
  if (!ds::open_frame_valid(f.z_open_after, f.z_fu, f.z_window, f.z_start, wmax, f.out_len))
    return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible open frame");
  return S3S_OK;
}

// LZ4 / Snappy / LZF: discover (LZ4) or count (Snappy, LZF), emit the frame records, cut
int feed_discover_frames(Feed& f) {
  s3s_ctx* ctx = f.ctx;
  const int codec = f.s->codec;
  const int32_t pn = f.pl.m;
  const int64_t PL = f.pl.PL;
  const int cf = codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy;
  int64_t *d_true_entry = nullptr, *d_base = nullptr;
  const int64_t* d_count;
  int rc;
  if (codec == S3S_CODEC_LZ4) {
    const int32_t n_tiles = lz4_tile_count(PL);
    const size_t tile_i64 = sizeof(int64_t) * (size_t)(n_tiles + 1);
    if ((rc = ensure(ctx, B_PART_NFRAMES, 4 * tile_i64 + sizeof(int32_t) * (size_t)(n_tiles + 1)))) return rc;
    int64_t* d_spec_entry = dev<int64_t>(ctx, B_PART_NFRAMES);
    int64_t* d_spec_exit = d_spec_entry + (n_tiles + 1);
    d_true_entry = d_spec_exit + (n_tiles + 1);
    d_base = d_true_entry + (n_tiles + 1);
    int32_t* d_spec_count = reinterpret_cast<int32_t*>(d_base + (n_tiles + 1));
    launch_lz4_discover_stream(f.P, PL, f.pl.pleft, n_tiles, d_spec_entry, d_spec_exit, d_spec_count, d_true_entry, d_base, f.d_status,
                               f.d_result, ctx->stream);
    d_count = d_base + n_tiles;
  } else {
    const size_t cnt_bytes = al16(sizeof(uint32_t) * f.n1);
    if ((rc = ensure(ctx, B_PART_NFRAMES, cnt_bytes + sizeof(int64_t) * (f.n1 + 1)))) return rc;
    uint32_t* d_cnt = dev<uint32_t>(ctx, B_PART_NFRAMES);
    d_base = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_PART_NFRAMES) + cnt_bytes);
    launch_snappy_count_frames_stream(f.P, f.d_poff, pn, f.pl.first_mid, f.pl.plast_pend, d_cnt, f.d_status, f.d_result, ctx->stream, cf);
    launch_scan_u32(d_cnt, pn, d_base, ctx->stream);
    d_count = d_base + pn;
  }
  int64_t stop;
  if ((rc = discovery_answer(f, d_count, codec == S3S_CODEC_LZ4 ? "frame chain" : "chunk chain", "frame", &stop))) return rc;
  if (f.n_frames == 0) return S3S_OK;
  if ((rc = ensure_frame_tables(ctx, sizeof(Frame), f.n_frames))) return rc;
  if (codec == S3S_CODEC_LZ4) {  // the one-shot emit, with the stop offset as the end of the bytes: the chain ends exactly there
    launch_lz4_emit_frames(f.P, stop, lz4_tile_count(stop), d_true_entry, d_base, dev<Frame>(ctx, B_FRAMES), dev<uint32_t>(ctx, B_ITEM_SIZE),
                           f.n_frames, dev<int64_t>(ctx, B_FRAME_OUT), f.d_status, ctx->stream);
  } else {
    launch_snappy_emit_frames_stream(f.P, f.d_poff, pn, f.pl.first_mid, f.pl.plast_pend, d_base, dev<Frame>(ctx, B_FRAMES),
                                     dev<uint32_t>(ctx, B_ITEM_SIZE), f.d_status, ctx->stream, cf);
    launch_scan_u32(dev<uint32_t>(ctx, B_ITEM_SIZE), f.n_frames, dev<int64_t>(ctx, B_FRAME_OUT), ctx->stream);
  }
  launch_frames_cut(codec, dev<Frame>(ctx, B_FRAMES), dev<uint32_t>(ctx, B_ITEM_SIZE), dev<int64_t>(ctx, B_FRAME_OUT), f.n_frames, f.cap, stop,
                    f.d_result, ctx->stream);
  return cut_answer(f, 4, stop, "frame header", "frame", "unit");
}

// discovery: the whole units of the window, then the cut at dst_capacity
int feed_discover(Feed& f) {
  f.consumed = f.out_len = f.pl.PL;
  if (f.s->codec == S3S_CODEC_NONE || f.pl.PL == 0) {  // (no plain byte: the window holds IVs, whole or cut, and nothing else)
    HIP_TRY(f.ctx, hipStreamSynchronize(f.ctx->stream));
    return S3S_OK;
  }
  return f.s->codec == S3S_CODEC_ZSTD ? feed_discover_zstd(f) : feed_discover_frames(f);
}

// back to the stored side; the verdict of every partition whose last byte this feed consumes, before anything is decoded; the
// state of the partition left open
int feed_verdict(Feed& f) {
  const ds::Stored st = ds::back_to_stored(f.pl, f.consumed, f.need_comp);
  if (st.into_short_part) return f.corrupt("partition shorter than its IV");
  f.consumed = st.consumed;
  f.need_comp = st.need_comp;
  const ds::Verdict v = ds::verdict(f.R, f.s->at, f.consumed, f.h_sums);
  if (v.bad >= 0) return stick(f.s, f.r, S3S_E_CHECKSUM, v.bad, "");
  f.q = v.cur;
  f.carry = ds::open_carry(f.R, f.s->at, f.n, f.h_off, f.h_sums, f.q, f.consumed);
  if (f.carry.kind == ds::Carry::kSecond) {
    f.h_off2[0] = f.carry.a;
    f.h_off2[1] = f.carry.b;
    f.h_seg2[0] = 0;
    f.h_seg2[1] = worst_segs(f.carry.b - f.carry.a);
    f.h_seed[f.n] = f.carry.value;
  }
  return S3S_OK;
}

// Zstandard: the frame that was open decodes behind its saved history in a staging area, so that every offset it may use is
// there; a frame that starts in this feed and stays open gets its memory now: a failure consumes nothing
int zstd_launch(Feed& f, ZNew& z_new) {
  s3s_dstream* s = f.s;
  s3s_ctx* ctx = f.ctx;
  const int32_t pn = f.pl.m;
  int rc;
  if (f.z_open_after && f.z_fu >= 0) {
    const size_t bytes = kZStateBytes + (size_t)(f.z_window > 0 ? f.z_window : 1);
    if (hipMalloc(&z_new.p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      z_new.p = nullptr;
      f.r->consumed = f.r->out_len = 0;
      return fail(ctx, S3S_E_NOMEM, "hipMalloc(%zu) for the open frame's history failed", bytes);
    }
  }
  int64_t max_piece = 0;
  for (int32_t i = 0; i < pn; i++) max_piece = std::max(max_piece, f.h_off[i + 1] - f.h_off[i]);
  const int64_t by_size = 8 * max_piece + 256;
  const int64_t lit_stride = ((std::min<int64_t>(by_size, s3s_zstd::kMaxBlock) + 64) + 15) & ~int64_t(15);
  if ((rc = ensure(ctx, B_ZBLOCK_LIT, (size_t)lit_stride * (size_t)pn + 64))) return rc;
  if (s->zopen) {
    if ((rc = ensure(ctx, B_ZSCRATCH, (size_t)(s->zhist_len + f.out_len) + 256))) return rc;
    if (s->zhist_len > 0)
      HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_ZSCRATCH].p, static_cast<uint8_t*>(s->zmem) + kZStateBytes, (size_t)s->zhist_len,
                                  hipMemcpyDeviceToDevice, ctx->stream));
  }
  ZStreamRun& zrun = f.zrun;
  zrun.k = f.k;
  zrun.execute = 1;
  zrun.st_out = !f.z_open_after ? nullptr : static_cast<s3s_zstd::ZStreamState*>(f.z_fu >= 0 ? z_new.p : s->zmem);
  zrun.staging = s->zopen ? dev<uint8_t>(ctx, B_ZSCRATCH) : nullptr;
  zrun.lit = dev<uint8_t>(ctx, B_ZBLOCK_LIT);
  zrun.lit_stride = lit_stride;
  launch_zstd_stream(zrun, pn, ctx->stream);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[10], f.d_result + 8, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  return S3S_OK;
}

// Zstandard, behind the decode's verdict: the resumed frame's bytes to dst, the open frame's last bytes to the stream
int zstd_keep(Feed& f, ZNew& z_new) {
  s3s_dstream* s = f.s;
  s3s_ctx* ctx = f.ctx;
  const int64_t out_len = f.out_len, resumed_out = s->zopen ? f.h_misc[10] : 0;
  if (resumed_out < 0 || resumed_out > out_len || (f.z_open_after && f.z_fu < 0 && resumed_out != out_len))
    return fail(ctx, S3S_E_HIP, "the resumed frame reported an impossible size");
  const uint8_t* staging = dev<uint8_t>(ctx, B_ZSCRATCH);
  if (resumed_out > 0)
    HIP_TRY(ctx, hipMemcpyAsync(f.d_dst, staging + s->zhist_len, (size_t)resumed_out, hipMemcpyDeviceToDevice, ctx->stream));
  if (!f.z_open_after) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    zfree(s);
  } else if (f.z_fu < 0) {  // still the same frame
    const int64_t produced = s->zproduced + out_len, nh = std::min(s->zwindow, produced), end = s->zhist_len + out_len;
    if (nh > 0)
      HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(s->zmem) + kZStateBytes, staging + (end - nh), (size_t)nh, hipMemcpyDeviceToDevice,
                                  ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    s->zproduced = produced;
    s->zhist_len = nh;
  } else {  // a frame that started in this feed
    const int64_t produced = out_len - f.z_start, nh = std::min(f.z_window, produced);
    if (nh > 0)
      HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(z_new.p) + kZStateBytes, f.d_dst + (out_len - nh), (size_t)nh, hipMemcpyDeviceToDevice,
                                  ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    zfree(s);
    s->zmem = z_new.p;
    z_new.p = nullptr;
    s->zheld = (int64_t)(kZStateBytes + (size_t)(f.z_window > 0 ? f.z_window : 1));
    g_zheld += s->zheld;
    s->zopen = true;
    s->zwindow = f.z_window;
    s->zproduced = produced;
    s->zhist_len = nh;
  }
  return S3S_OK;
}

// decode the cut frame table with the one-shot path's decoders; behind them the second checksum launch, when the cut asks for it
int feed_decode(Feed& f) {
  s3s_dstream* s = f.s;
  s3s_ctx* ctx = f.ctx;
  const int codec = s->codec;
  const int32_t n = f.n, k = (int32_t)f.k;
  const bool second = f.carry.kind == ds::Carry::kSecond;
  int rc;
  if (codec == S3S_CODEC_NONE) {
    HIP_TRY(ctx, hipMemcpyAsync(f.d_dst, f.P, (size_t)f.out_len, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return S3S_OK;
  }
  if (f.k == 0 && !second) return S3S_OK;
  ZNew z_new;
  if (f.k > 0 && codec == S3S_CODEC_ZSTD) {
    if ((rc = zstd_launch(f, z_new))) return rc;
  } else if (f.k > 0) {
    if (codec == S3S_CODEC_LZ4)
      launch_lz4_decompress(f.P, dev<Frame>(ctx, B_FRAMES), k, dev<int64_t>(ctx, B_FRAME_OUT), f.d_dst, f.d_status, ctx->lz4_decode_variant,
                            ctx->stream);
    else
      launch_snappy_decompress(f.P, dev<Frame>(ctx, B_FRAMES), k, dev<int64_t>(ctx, B_FRAME_OUT), f.d_dst, f.d_status, ctx->lz4_decode_variant,
                               ctx->stream, codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (second) {
    HIP_TRY(ctx, hipMemcpyAsync(f.d_off + f.n1, f.h_off2, 16, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dev<int64_t>(ctx, B_REF_SUMS) + n, &f.h_seed[n], 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_checksum(ctx, s->algo, f.d_comp, f.d_off + f.n1, 1, f.h_seg2, dev<int64_t>(ctx, B_SUMS) + n, f.L))) return rc;
    launch_checksum_seed(s->algo, f.d_off + f.n1, 1, ctx->buf[B_TABLES].p, dev<int64_t>(ctx, B_REF_SUMS) + n, dev<int64_t>(ctx, B_SUMS) + n,
                         ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&f.h_sums[n], dev<int64_t>(ctx, B_SUMS) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[1], f.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  int32_t st = f.status();
  if (st == S3S_E_UNSUPPORTED && codec == S3S_CODEC_LZ4 && ctx->lz4_decode_variant != 3) {  // a frame above 32 MiB: the ring decoder, as in the one-shot call
    HIP_TRY(ctx, hipMemsetAsync(f.d_status, 0, 16, ctx->stream));
    launch_lz4_decompress(f.P, dev<Frame>(ctx, B_FRAMES), k, dev<int64_t>(ctx, B_FRAME_OUT), f.d_dst, f.d_status, 3, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&f.h_misc[1], f.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    st = f.status();
  }
  if (st == S3S_E_UNSUPPORTED) return too_large(ctx);
  if (st != 0) return f.corrupt("frame payload");  // (the capacity cut may have left a partition's end, which the window holds, unconsumed)
  if (second) f.carry.value = f.h_sums[n];
  if (f.k > 0 && codec == S3S_CODEC_ZSTD) return zstd_keep(f, z_new);
  return S3S_OK;
}

void feed_commit(Feed& f) {
  s3s_dstream* s = f.s;
  const ds::Commit c = ds::commit(f.R, s->at, f.pl.front, f.q, f.consumed, f.carry.value, f.need_comp);
  if (c.iv_piece >= 0) memcpy(s->iv, f.h_iv + 16 * (size_t)c.iv_piece, sizeof s->iv);  // the open partition's IV: it started in this window
  f.r->consumed = f.consumed;
  f.r->out_len = f.out_len;
  f.r->need_comp = c.need_comp;
  f.r->at_end = c.at_end;
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

int64_t s3s_dstream_position(const s3s_dstream* s) { return s ? s->at.pos : (int64_t)S3S_E_INVALID; }

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
  int rc;
  if ((rc = feed_check(s, d_comp, comp_len, d_dst, dst_capacity, r))) return rc;
  Feed f = {s, s->ctx, r, d_comp, d_dst, dst_capacity, range_of(s)};
  f.L = ds::window_len(f.R, s->at, s->codec, comp_len, dst_capacity);
  if (comp_len > 0 && f.L == 0) {
    r->need_dst = 1;
    return fail(s->ctx, S3S_E_CAPACITY, "dst_capacity 0 < 1");
  }
  if (f.L == 0) return feed_empty(f);
  if ((rc = feed_layout(f))) return rc;    // staging, pieces, the plain side
  if ((rc = feed_queue(f))) return rc;     // decrypt and checksums, in front of discovery
  if ((rc = feed_discover(f))) return rc;  // the whole units of the window and the cut at dst_capacity: one or two waits
  if ((rc = feed_verdict(f))) return rc;   // the partitions this feed closes; the open partition's carry
  if ((rc = feed_decode(f))) return rc;    // one more wait; nothing of the stream has moved so far
  feed_commit(f);
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
// The path of s3s_dstream_feed_device for LZ4 / Snappy / LZF streams, plain or encrypted, with every kernel launched once per
// CALL (decode_stream_batch.hip) and the same three host waits whatever n is: checksums + discovery, frame tables + cut, decode.
// Under IO encryption a window has the two sides of the single feed: the STORED side - the entry's d_comp, what the checksums
// run over and what consumed, need_comp and the position count - and the PLAIN side, a slice of the crypt workspace that one
// launch of the window pass (aes_ctr_stream_batch.hip) fills for all windows in front of discovery.  Discovery, the cut and the
// decoders get the plain side through the same descriptors and do not know of the layer; ds::plain_side, ds::back_to_stored
// and ds::commit map between the two, per window, exactly as feed_layout, feed_verdict and feed_commit do.
// Every verdict is made on the host by the single feed's rules (decode_stream_core.h) from the same device words, and NO
// stream's state is committed before the decode's verdict is known: when the batch's one decode status word comes back
// non-zero, the undecided entries go through the single feed one by one, which says whose it was - nothing was committed, so
// its answers are the single feed's.
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
  ds::Plain pl;           // its plain side (without the layer: the stored side); q / c point into the arena
  int32_t aes_tiles = 0;  // encrypted: tiles of the decrypt launch it owns
  size_t plain_at = 0;    //            its plain buffer in B_CRYPT
};

// One arena, host (pinned) and device, uploaded in one copy:
//   [offsets P + m][seeds P][seg_start P + m][piece -> window P][tile -> window T]
//   [encrypted: plain offsets P + m | AesWindow m | decrypt tile -> window TA][tails m][windows: LzRange m][StreamWin m]
//   [second checksum launch: offsets 2 m | seeds m | seg_start 2 m | piece -> task m | tails m]
// and behind it on the host the downloads: [status words m + 1][result words kWinWords x m][encrypted: gathered IVs 16 x P]
// [sums P][second sums m], and what only the host reads: [encrypted: first cipher byte of every plain piece P + m].
// The plain offsets of a window stand where its stored ones do (at its first piece + its index; m + 1 of its n + 1 slots are
// used), so the piece -> window map serves both tables.  Without the layer the encrypted parts are empty
struct BatchArena {
  size_t off = 0, seed, seg, pw, tw, q, aw, atw, tail, rng, win, off2, seed2, seg2, pw2, tail2, total;
  size_t st, res, iv, sum, sum2, c, stage_total;
  uint8_t *hs = nullptr, *da = nullptr;
  void lay_out(size_t P, size_t M, size_t T, size_t TA, bool enc) {
    const size_t PM = P + M, e = enc ? 1 : 0;
    seed = al16(off + 8 * PM), seg = al16(seed + 8 * (P + 1)), pw = al16(seg + 4 * PM), tw = al16(pw + 4 * (P + 1));
    q = al16(tw + 4 * (T + 1)), aw = al16(q + e * 8 * PM), atw = al16(aw + e * sizeof(AesWindow) * M);
    tail = al16(atw + e * 4 * (TA + 1)), rng = al16(tail + sizeof(TaskTail) * M), win = al16(rng + sizeof(LzRange) * M);
    off2 = al16(win + sizeof(StreamWin) * M), seed2 = al16(off2 + 16 * M), seg2 = al16(seed2 + 8 * M), pw2 = al16(seg2 + 8 * M);
    tail2 = al16(pw2 + 4 * M), total = al16(tail2 + sizeof(TaskTail) * M);
    st = al16(total), res = al16(st + 4 * (M + 1)), iv = res + 8 * kWinWords * M, sum = al16(iv + e * 16 * P), sum2 = al16(sum + 8 * (P + 1));
    c = al16(sum2 + 8 * M), stage_total = al16(c + e * 8 * PM);
  }
  template <class X> X* h(size_t o) const { return reinterpret_cast<X*>(hs + o); }
  template <class X> const X* d(size_t o) const { return reinterpret_cast<const X*>(da + o); }
};

struct Batch {
  s3s_ctx* ctx;
  s3s_dstream_feed_entry* E;
  int32_t n_entries;
  int codec = 0, algo = 0, cf = 0;
  std::vector<BatchWin> W;
  int32_t m = 0;             // windows
  size_t P = 0, SG = 0;      // pieces and checksum segment slots of all windows
  int64_t T = 0;             // LZ4: tiles of all windows
  bool enc = false;          // the windows are those of encrypted streams: they have a plain side of their own
  int64_t TA = 0;            // encrypted: tiles of the decrypt launch
  size_t crypt_bytes = 0;    //            the plain buffers of all windows
  size_t iv_bytes = 0;       //            the gathered IVs (16 x P), behind the result words on both sides
  std::vector<int64_t> tmp;  //            batch_windows' offsets of one window
  BatchArena A;
  std::vector<size_t> ws_off;  // discovery workspace per window
  size_t st_bytes = 0, res_bytes = 0;
  int32_t* d_status = nullptr;
  int64_t *d_result = nullptr, *d_sums = nullptr;
  int64_t total_frames = 0;
  int32_t n_second = 0;
  bool any_decode = false;

  s3s_dstream_feed_entry& entry(const BatchWin& w) const { return E[w.e]; }
  int64_t* off_of(size_t wi) const { return A.h<int64_t>(A.off) + W[wi].piece0 + wi; }  // the window's n + 1 piece offsets
  int64_t* sums_of(const BatchWin& w) const { return A.h<int64_t>(A.sum) + w.piece0; }
  int64_t* q_of(size_t wi) const { return A.h<int64_t>(A.q) + W[wi].piece0 + wi; }          // encrypted: its plain piece offsets
  int64_t* c_of(size_t wi) const { return A.h<int64_t>(A.c) + W[wi].piece0 + wi; }          //            ... first cipher bytes
  const uint8_t* ivs_of(const BatchWin& w) const { return A.h<uint8_t>(A.iv) + 16 * w.piece0; }  //        ... gathered IVs
  const int64_t* words_of(size_t wi) const { return A.h<int64_t>(A.res) + (size_t)kWinWords * wi; }  // (status and result words come down in one copy)
  int32_t status_of(size_t wi) const { return A.h<int32_t>(A.st)[wi]; }

  void single(s3s_dstream_feed_entry& e) { e.status = s3s_dstream_feed_device(e.stream, e.d_comp, e.comp_len, e.d_dst, e.dst_capacity, &e.result); }
  int first_error() {
    for (int32_t i = 0; i < n_entries; i++)
      if (E[i].status != S3S_OK) {
        char msg[sizeof ctx->err];
        snprintf(msg, sizeof msg, "%s", ctx->err);
        return fail(ctx, E[i].status, "entry %d of the batch failed%s%.400s", i, msg[0] ? ": " : "", msg);
      }
    return S3S_OK;
  }
  void decide(BatchWin& w, int status) {
    E[w.e].status = status;
    w.decided = true;
  }
  void refused(BatchWin& w, int32_t st, const char* what) {  // the single feed's answer to a kernel's status word
    s3s_dstream_feed_entry& e = E[w.e];
    decide(w, refuse(e.stream, &e.result, ds::refusal(range_of(e.stream), e.stream->at, e.comp_len, w.n, sums_of(w), st), what));
  }
};

// call-level refusals: nothing has been touched.  *batched: the batched path takes these streams (which of them the context's
// key setting lets run is an entry's matter: batch_windows)
int batch_check(Batch& b, bool* batched) {
  s3s_ctx* ctx = b.ctx;
  *batched = b.n_entries > 1;
  std::vector<const s3s_dstream*> seen;
  seen.reserve((size_t)b.n_entries);
  for (int32_t i = 0; i < b.n_entries; i++) {
    const s3s_dstream* s = b.E[i].stream;
    if (!s) return fail(ctx, S3S_E_INVALID, "entry %d: null stream", i);
    if (s->ctx != ctx) return fail(ctx, S3S_E_INVALID, "entry %d: the stream was opened on another context", i);
    if (s->codec != b.E[0].stream->codec || s->algo != b.E[0].stream->algo)
      return fail(ctx, S3S_E_INVALID, "entry %d: the streams of a batch must share codec and checksum algorithm", i);
    if (s->wlog != 0 || s->codec == S3S_CODEC_NONE) *batched = false;
    seen.push_back(s);
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(ctx, S3S_E_INVALID, "the same stream twice in one batch");
  return S3S_OK;
}

// entries the single feed answers without device work keep its answer: a sticky error, an argument it refuses, an empty
// window, a stream that the context's key setting leaves no feed (an encrypted one bound to an earlier setting, a plain one
// under the layer).  The others are the windows of the batch: all plain, or all encrypted under the current key
void batch_windows(Batch& b) {
  s3s_ctx* ctx = b.ctx;
  b.enc = enc_on(ctx);
  b.W.reserve((size_t)b.n_entries);
  for (int32_t i = 0; i < b.n_entries; i++) {
    s3s_dstream_feed_entry& e = b.E[i];
    const s3s_dstream* s = e.stream;
    const int64_t left = s->off[(size_t)s->nparts] - s->at.pos;
    const bool no_feed = s->enc ? (s->epoch != ctx->enc_epoch || !b.enc) : b.enc;  // feed_check's two refusals
    if (s->err != S3S_OK || e.comp_len <= 0 || e.dst_capacity < 0 || !e.d_comp || (e.dst_capacity > 0 && !e.d_dst) || e.comp_len > left || no_feed) {
      b.single(e);
      continue;
    }
    const ds::Range R = range_of(s);
    BatchWin w;
    w.e = i;
    w.n = ds::piece_count(R, s->at, e.comp_len);
    w.piece0 = b.P;
    w.seg0 = b.SG;
    b.P += (size_t)w.n;
    b.SG += (size_t)ds::window_segs(R, s->at, e.comp_len, w.n, kChecksumSegBytes);
    int64_t PL = e.comp_len;
    if (b.enc) {  // what the plain side needs of the workspace; batch_layout builds it again, in the arena
      const size_t n1 = (size_t)w.n + 1;
      b.tmp.assign(3 * n1, 0);
      for (int32_t p = 0; p < w.n; p++) ds::piece(R, s->at, e.comp_len, p, b.tmp[(size_t)p], b.tmp[(size_t)p + 1]);
      const ds::Plain pl = ds::plain_side(R, s->at, e.comp_len, w.n, b.tmp.data(), b.tmp.data() + n1, b.tmp.data() + 2 * n1);
      PL = pl.PL;
      w.aes_tiles = aes_ctr_window_tiles(pl.m, pl.front, b.tmp[(size_t)pl.m]);
      w.plain_at = b.crypt_bytes;
      b.TA += w.aes_tiles;
      b.crypt_bytes += ((size_t)PL + 64 + 255) & ~size_t(255);  // PL + 64 bytes as the single feed's, every buffer aligned as B_CRYPT is
    }
    if (b.codec == S3S_CODEC_LZ4) b.T += lz4_tile_count(PL);
    b.W.push_back(w);
  }
  b.m = (int32_t)b.W.size();
}

// the arena and the workspace, sized and filled: every window's pieces, its checksum task, its LzRange and StreamWin
int batch_layout(Batch& b) {
  s3s_ctx* ctx = b.ctx;
  BatchArena& A = b.A;
  const size_t M = (size_t)b.m, P = b.P, SG = b.SG;
  const int codec = b.codec;
  A.lay_out(P, M, (size_t)b.T, (size_t)b.TA, b.enc);
  int rc;
  if ((rc = ensure_stage(ctx, A.stage_total))) return rc;
  if ((rc = ensure(ctx, B_PLAN, A.total))) return rc;
  b.st_bytes = al16(4 * (M + 1)), b.res_bytes = 8 * kWinWords * M, b.iv_bytes = b.enc ? 16 * P : 0;
  if ((rc = ensure(ctx, B_STATUS, b.st_bytes + b.res_bytes + b.iv_bytes + 16))) return rc;  // [status words][result words][gathered IVs]
  if (b.enc && (rc = ensure(ctx, B_CRYPT, b.crypt_bytes + 64))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * (P + M + 1)))) return rc;
  if ((rc = ensure(ctx, B_PARTIAL, 16 * (SG > 0 ? SG : 1)))) return rc;
  // discovery workspace per window: LZ4 4 x (tiles + 1) int64 + (tiles + 1) int32; Snappy / LZF (n + 1) int32 + (n + 2) int64
  b.ws_off.resize(M + 1);
  size_t ws = 0;
  for (size_t i = 0; i < M; i++) {
    b.ws_off[i] = ws;
    // (the tiles of the stored window bound those of its plain side: a slot too many, never one too few)
    const size_t c1 = codec == S3S_CODEC_LZ4 ? (size_t)lz4_tile_count(b.entry(b.W[i]).comp_len) + 1 : (size_t)b.W[i].n + 2;
    ws += al16(4 * 8 * c1 + 4 * c1);
  }
  b.ws_off[M] = ws;
  if ((rc = ensure(ctx, B_PART_NFRAMES, ws + 16))) return rc;
  A.hs = static_cast<uint8_t*>(ctx->h_stage);
  A.da = dev<uint8_t>(ctx, B_PLAN);
  b.d_status = dev<int32_t>(ctx, B_STATUS);
  b.d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + b.st_bytes);
  b.d_sums = dev<int64_t>(ctx, B_SUMS);

  memset(A.hs + A.tail, 0, A.off2 - A.tail);
  int32_t tile0 = 0, aes_tile0 = 0;
  for (int32_t wi = 0; wi < b.m; wi++) {
    BatchWin& w = b.W[(size_t)wi];
    const s3s_dstream_feed_entry& e = b.entry(w);
    const s3s_dstream* s = e.stream;
    const ds::Range R = range_of(s);
    const int64_t L = e.comp_len;
    const size_t o0 = w.piece0 + (size_t)wi;  // the window's first offset
    const int64_t segs = ds::fill_pieces(R, s->at, L, w.n, kChecksumSegBytes, b.off_of((size_t)wi), A.h<int32_t>(A.seg) + o0, A.h<int64_t>(A.seed) + w.piece0);
    for (int32_t p = 0; p < w.n; p++) A.h<int32_t>(A.pw)[w.piece0 + (size_t)p] = wi;
    TaskTail& t = A.h<TaskTail>(A.tail)[wi];
    t.first_pp = (int32_t)o0;
    t.n_parts = w.n;
    t.first_part = (int32_t)w.piece0;
    t.first_seg = (int32_t)w.seg0;
    t.n_segs = (int32_t)segs;
    t.data = e.d_comp;
    t.data_len = L;
    // the plain side: what discovery, the cut and the decoders see.  Without the layer it is the stored side
    ds::Plain& pl = w.pl = ds::plain_side(R, s->at, L, w.n, b.off_of((size_t)wi), b.enc ? b.q_of((size_t)wi) : nullptr, b.enc ? b.c_of((size_t)wi) : nullptr);
    const uint8_t* comp = e.d_comp;
    if (b.enc) {
      uint8_t* plain = dev<uint8_t>(ctx, B_CRYPT) + w.plain_at;
      comp = plain;
      AesWindow& a = A.h<AesWindow>(A.aw)[wi];
      a.in = e.d_comp;
      a.out = plain;
      a.E = A.d<int64_t>(A.off) + o0;
      a.Q = A.d<int64_t>(A.q) + o0;
      a.iv_out = reinterpret_cast<uint8_t*>(b.d_result) + b.res_bytes + 16 * w.piece0;
      a.m = pl.m;
      a.tile0 = aes_tile0;
      a.front = pl.front;
      a.L = b.off_of((size_t)wi)[pl.m];
      a.iv = {{s3s_aes::load_be32(s->iv), s3s_aes::load_be32(s->iv + 4), s3s_aes::load_be32(s->iv + 8), s3s_aes::load_be32(s->iv + 12)}};
      for (int32_t t2 = 0; t2 < w.aes_tiles; t2++) A.h<int32_t>(A.atw)[aes_tile0 + t2] = wi;
      aes_tile0 += w.aes_tiles;
    }
    LzRange& r = A.h<LzRange>(A.rng)[wi];
    uint8_t* ws_i = dev<uint8_t>(ctx, B_PART_NFRAMES) + b.ws_off[(size_t)wi];
    const int32_t nt = codec == S3S_CODEC_LZ4 ? lz4_tile_count(pl.PL) : 0;
    const size_t c1 = codec == S3S_CODEC_LZ4 ? (size_t)nt + 1 : (size_t)w.n + 2;
    r.comp = comp;
    r.comp_len = pl.PL;
    r.n_tiles = nt;
    r.tile0 = tile0;
    r.spec_entry = reinterpret_cast<int64_t*>(ws_i);
    r.spec_exit = r.spec_entry + c1;
    r.true_entry = r.spec_exit + c1;
    r.frame_base = r.true_entry + c1;
    r.spec_count = reinterpret_cast<int32_t*>(r.frame_base + c1);
    r.status = b.d_status + wi;
    r.result = b.d_result + (size_t)kWinWords * (size_t)wi;
    r.dst_base = (int64_t)reinterpret_cast<uintptr_t>(e.d_dst);
    r.dst_capacity = e.dst_capacity;
    for (int32_t t2 = 0; t2 < nt; t2++) A.h<int32_t>(A.tw)[tile0 + t2] = wi;
    tile0 += nt;
    StreamWin& x = A.h<StreamWin>(A.win)[wi];
    x.range_left = pl.pleft;
    x.last_pend = pl.plast_pend;
    x.first_piece = (int32_t)w.piece0;
    x.n_pieces = pl.m;
    x.first_mid = pl.first_mid ? 1 : 0;
  }
  return S3S_OK;
}

// phase 1: the checksums of every piece, seeded, and stream-mode discovery of every window; one wait
int batch_discover(Batch& b) {
  s3s_ctx* ctx = b.ctx;
  const BatchArena& A = b.A;
  const LzRange* d_rng = A.d<LzRange>(A.rng);
  const StreamWin* d_win = A.d<StreamWin>(A.win);
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, b.st_bytes + b.res_bytes, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(A.da, A.hs, A.off2, hipMemcpyHostToDevice, ctx->stream));
  record(ctx, 0);
  if (b.enc) {  // in front of discovery: every window's plain side and its IVs, one launch
    launch_aes_ctr_window_batch(ctx->enc_keys, ctx->enc_rounds, A.d<AesWindow>(A.aw), A.d<int32_t>(A.atw), (int32_t)b.TA, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
  }
  const int64_t* d_poff = A.d<int64_t>(b.enc ? A.q : A.off);  // the pieces discovery walks
  if (b.algo != S3S_CHECKSUM_NONE) {
    launch_checksum_batch(b.algo, A.d<TaskTail>(A.tail), b.m, (int32_t)b.SG, (int32_t)b.P, A.d<int64_t>(A.off), A.d<int32_t>(A.seg),
                          ctx->buf[B_TABLES].p, dev<uint32_t>(ctx, B_PARTIAL), b.d_sums, ctx->stream);
    launch_checksum_seed_batch(b.algo, A.d<int64_t>(A.off), A.d<int32_t>(A.pw), (int32_t)b.P, ctx->buf[B_TABLES].p, A.d<int64_t>(A.seed), b.d_sums,
                               ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(A.h<int64_t>(A.sum), b.d_sums, 8 * b.P, hipMemcpyDeviceToHost, ctx->stream));
  }
  record(ctx, 1);
  if (b.codec == S3S_CODEC_LZ4) {
    launch_lz4_speculate_batch(d_rng, A.d<int32_t>(A.tw), (int32_t)b.T, ctx->stream);
    launch_lz4_resolve_stream_batch(d_rng, d_win, b.m, ctx->stream);
  } else {
    launch_snappy_count_stream_batch(d_rng, d_win, b.m, d_poff, A.d<int32_t>(A.pw), (int32_t)b.P, b.cf, ctx->stream);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(A.h<int32_t>(A.st), b.d_status, b.st_bytes + b.res_bytes + b.iv_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // the single feed's verdicts, per window, from the same words
  for (int32_t wi = 0; wi < b.m; wi++) {
    BatchWin& w = b.W[(size_t)wi];
    s3s_dstream_feed_entry& e = b.entry(w);
    memset(&e.result, 0, sizeof e.result);
    e.result.bad_partition = -1;
    w.first_frame = b.total_frames;
    if (w.pl.PL == 0) continue;  // no plain byte (IVs, whole or cut, and nothing else): nothing was discovered, as in feed_discover
    if (b.status_of((size_t)wi) != 0) {
      b.refused(w, b.status_of((size_t)wi), b.codec == S3S_CODEC_LZ4 ? "frame chain" : "chunk chain");
      continue;
    }
    const int64_t* res = b.words_of((size_t)wi);
    w.stop = res[0];
    w.need_comp = res[1];
    w.n_frames = res[2];
    if (!ds::stop_valid(w.stop, w.need_comp, w.pl.PL) || w.n_frames < 0) {
      b.decide(w, bad_stop(ctx, "frame"));
      w.n_frames = 0;
      continue;
    }
    if (w.n_frames > ds::kMaxCount || b.total_frames + w.n_frames > ds::kMaxCount) {
      b.decide(w, too_many(ctx, "frame"));
      w.n_frames = 0;
      continue;
    }
    w.k = 0;
    w.consumed = w.stop;
    w.out_len = 0;
    b.total_frames += w.n_frames;
  }
  return S3S_OK;
}

// phase 2: the frame records of every window, the scan of its decoded sizes, its cut at its own dst_capacity; one wait
int batch_cut(Batch& b) {
  s3s_ctx* ctx = b.ctx;
  const BatchArena& A = b.A;
  const LzRange* d_rng = A.d<LzRange>(A.rng);
  const StreamWin* d_win = A.d<StreamWin>(A.win);
  const size_t nf1 = (size_t)b.total_frames + (size_t)b.m + 1;
  int rc;
  if ((rc = ensure(ctx, B_FRAMES, sizeof(Frame) * nf1))) return rc;
  if ((rc = ensure(ctx, B_ITEM_SIZE, 4 * nf1))) return rc;
  if ((rc = ensure(ctx, B_FRAME_OUT, 8 * nf1))) return rc;
  if ((rc = ensure(ctx, B_ITEM_OFF, 8 * nf1))) return rc;
  for (int32_t wi = 0; wi < b.m; wi++) {
    const BatchWin& w = b.W[(size_t)wi];
    LzRange& r = A.h<LzRange>(A.rng)[wi];
    const int64_t f0 = w.first_frame;
    r.n_frames = w.decided ? 0 : w.n_frames;
    r.skip = w.decided ? 1 : 0;
    if (b.codec == S3S_CODEC_LZ4 && !w.decided) r.comp_len = w.stop;  // the one-shot emit, with the stop offset as the end of the bytes
    r.frames = dev<Frame>(ctx, B_FRAMES) + f0;
    r.frame_orig = dev<uint32_t>(ctx, B_ITEM_SIZE) + f0 + wi;
    r.frame_out = dev<int64_t>(ctx, B_FRAME_OUT) + f0 + wi;
    r.out_abs = dev<int64_t>(ctx, B_ITEM_OFF) + f0;
    A.h<StreamWin>(A.win)[wi].stop = w.stop;
    A.h<StreamWin>(A.win)[wi].first_frame = f0;
  }
  HIP_TRY(ctx, hipMemcpyAsync(A.da + A.rng, A.hs + A.rng, A.off2 - A.rng, hipMemcpyHostToDevice, ctx->stream));
  if (b.codec == S3S_CODEC_LZ4) launch_lz4_emit_batch(d_rng, A.d<int32_t>(A.tw), (int32_t)b.T, ctx->stream);
  else launch_snappy_emit_stream_batch(d_rng, d_win, b.m, A.d<int64_t>(b.enc ? A.q : A.off), A.d<int32_t>(A.pw), (int32_t)b.P, b.cf, ctx->stream);
  launch_frames_cut_batch(b.codec, d_rng, d_win, b.m, ctx->stream);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(A.h<int32_t>(A.st), b.d_status, b.st_bytes + b.res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  record(ctx, 2);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return S3S_OK;
}

// every undecided window: the cut's words, the partitions its feed closes, the carry of the one it leaves open (the single
// feed's feed_verdict); a cut that ended inside a piece becomes a task of the second checksum launch
void batch_verdicts(Batch& b) {
  s3s_ctx* ctx = b.ctx;
  const BatchArena& A = b.A;
  for (int32_t wi = 0; wi < b.m; wi++) {
    BatchWin& w = b.W[(size_t)wi];
    if (w.decided) continue;
    s3s_dstream_feed_entry& e = b.entry(w);
    s3s_dstream* s = e.stream;
    const ds::Range R = range_of(s);
    if (w.n_frames > 0) {
      if (b.status_of((size_t)wi) != 0) {
        b.refused(w, b.status_of((size_t)wi), "frame header");
        continue;
      }
      const int64_t* res = b.words_of((size_t)wi);
      w.k = res[4];
      w.consumed = res[5];
      w.out_len = res[6];
      if (!ds::cut_valid(w.k, w.consumed, w.out_len, w.n_frames, w.stop, e.dst_capacity)) {
        b.decide(w, bad_cut(ctx, "frame"));
        continue;
      }
      if (ds::nothing_fits(w.pl, w.consumed)) {
        b.decide(w, no_room(ctx, &e.result, e.dst_capacity, res[7], "unit"));
        continue;
      }
    }
    const ds::Stored st = ds::back_to_stored(w.pl, w.consumed, w.need_comp);  // consumed and need_comp were plain offsets so far
    if (st.into_short_part) {
      b.refused(w, S3S_E_BAD_FRAME, "partition shorter than its IV");
      continue;
    }
    w.consumed = st.consumed;
    w.need_comp = st.need_comp;
    const ds::Verdict v = ds::verdict(R, s->at, w.consumed, b.sums_of(w));
    if (v.bad >= 0) {
      b.decide(w, stick(s, &e.result, S3S_E_CHECKSUM, v.bad, ""));
      continue;
    }
    w.q = v.cur;
    const ds::Carry c = ds::open_carry(R, s->at, w.n, b.off_of((size_t)wi), b.sums_of(w), w.q, w.consumed);
    w.carry = c.value;
    if (c.kind == ds::Carry::kSecond) {
      const int32_t t = w.second = b.n_second++;
      A.h<int64_t>(A.off2)[2 * t] = c.a;
      A.h<int64_t>(A.off2)[2 * t + 1] = c.b;
      A.h<int32_t>(A.seg2)[2 * t] = 0;
      A.h<int32_t>(A.seg2)[2 * t + 1] = worst_segs(c.b - c.a);
      A.h<int64_t>(A.seed2)[t] = c.value;
      A.h<int32_t>(A.pw2)[t] = t;
      TaskTail& tt = A.h<TaskTail>(A.tail2)[t];
      memset(&tt, 0, sizeof tt);
      tt.first_pp = 2 * t;
      tt.n_parts = 1;
      tt.first_part = t;
      tt.n_segs = worst_segs(c.b - c.a);
      tt.data = e.d_comp;
      tt.data_len = e.comp_len;
    }
    if (w.k > 0) b.any_decode = true;
  }
}

// phase 3: one decode launch over the frames of all windows in front of their cuts, the second checksum launch; one wait.
// *dec_status: the batch's one decode status word
int batch_decode(Batch& b, int32_t* dec_status) {
  s3s_ctx* ctx = b.ctx;
  const BatchArena& A = b.A;
  const int32_t m = b.m, n_second = b.n_second;
  int32_t* d_dec_status = b.d_status + m;
  if (b.any_decode) {
    for (int32_t wi = 0; wi < m; wi++) A.h<LzRange>(A.rng)[wi].skip = b.W[(size_t)wi].decided ? 1 : 0;
    HIP_TRY(ctx, hipMemcpyAsync(A.da + A.rng, A.hs + A.rng, sizeof(LzRange) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    launch_frames_rebase_cut(A.d<LzRange>(A.rng), A.d<StreamWin>(A.win), m, b.total_frames, ctx->stream);
    if (b.codec == S3S_CODEC_LZ4)
      launch_lz4_decompress(nullptr, dev<Frame>(ctx, B_FRAMES), (int32_t)b.total_frames, dev<int64_t>(ctx, B_ITEM_OFF), nullptr, d_dec_status,
                            ctx->lz4_decode_variant, ctx->stream);
    else
      launch_snappy_decompress(nullptr, dev<Frame>(ctx, B_FRAMES), (int32_t)b.total_frames, dev<int64_t>(ctx, B_ITEM_OFF), nullptr, d_dec_status,
                               ctx->lz4_decode_variant, ctx->stream, b.cf);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (n_second > 0) {  // the pieces the cuts left open, summed up to the cut: one launch for all of them
    int32_t seg0 = 0;
    for (int32_t t = 0; t < n_second; t++) {
      A.h<TaskTail>(A.tail2)[t].first_seg = seg0;
      seg0 += A.h<TaskTail>(A.tail2)[t].n_segs;
    }
    HIP_TRY(ctx, hipMemcpyAsync(A.da + A.off2, A.hs + A.off2, A.total - A.off2, hipMemcpyHostToDevice, ctx->stream));
    launch_checksum_batch(b.algo, A.d<TaskTail>(A.tail2), n_second, seg0, n_second, A.d<int64_t>(A.off2), A.d<int32_t>(A.seg2), ctx->buf[B_TABLES].p,
                          dev<uint32_t>(ctx, B_PARTIAL), b.d_sums + b.P, ctx->stream);
    launch_checksum_seed_batch(b.algo, A.d<int64_t>(A.off2), A.d<int32_t>(A.pw2), n_second, ctx->buf[B_TABLES].p, A.d<int64_t>(A.seed2),
                               b.d_sums + b.P, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(A.h<int64_t>(A.sum2), b.d_sums + b.P, 8 * (size_t)n_second, hipMemcpyDeviceToHost, ctx->stream));
  }
  record(ctx, 3);
  HIP_TRY(ctx, hipMemcpyAsync(&A.h<int32_t>(A.st)[m], d_dec_status, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->profile) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[3]) == hipSuccess) ctx->stage_ms[S3S_STAGE_TOTAL] = ms;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->stage_ms[S3S_STAGE_CHECKSUM] = ms;
    if (b.total_frames > 0 && hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]) == hipSuccess) ctx->stage_ms[S3S_STAGE_DISCOVER] = ms;
    if (b.total_frames > 0 && hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->stage_ms[S3S_STAGE_CODEC] = ms;
  }
  *dec_status = b.any_decode ? b.status_of((size_t)m) : 0;
  return S3S_OK;
}

void batch_commit(Batch& b) {
  for (BatchWin& w : b.W) {
    if (w.decided) continue;
    s3s_dstream_feed_entry& e = b.entry(w);
    const int64_t carry = w.second >= 0 ? b.A.h<int64_t>(b.A.sum2)[w.second] : w.carry;
    const ds::Commit c = ds::commit(range_of(e.stream), e.stream->at, w.pl.front, w.q, w.consumed, carry, w.need_comp);
    if (c.iv_piece >= 0) memcpy(e.stream->iv, b.ivs_of(w) + 16 * (size_t)c.iv_piece, sizeof e.stream->iv);  // the open partition's IV: it started in this window
    e.result.consumed = w.consumed;
    e.result.out_len = w.out_len;
    e.result.need_comp = c.need_comp;
    e.result.at_end = c.at_end;
    e.status = S3S_OK;
  }
}

}  // namespace

extern "C" {

int s3s_dstream_feed_batch_device(s3s_ctx* ctx, s3s_dstream_feed_entry* E, int32_t n_entries) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  if (n_entries < 0 || (n_entries > 0 && !E)) return fail(ctx, S3S_E_INVALID, "null entry array or negative count");
  ctx->dstream_batch_entries = 0;  // S3S_OPT_DSTREAM_BATCH_ENTRIES: set where the batched path has answered
  BatchVerdict<s3s_dstream_feed_entry> verdict(E, n_entries);
  if (n_entries == 0) return verdict.finish(S3S_OK);
  Batch b = {ctx, E, n_entries};
  bool batched;
  int rc;
  if ((rc = batch_check(b, &batched))) return rc;
  if (!batched) {  // nothing to batch: one by one, in order
    for (int32_t i = 0; i < n_entries; i++) b.single(E[i]);
    return verdict.finish(b.first_error());
  }
  b.codec = E[0].stream->codec;
  b.algo = E[0].stream->algo;
  b.cf = b.codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy;
  batch_windows(b);
  if (b.m == 0) return verdict.finish(b.first_error());
  if (b.P > (size_t)ds::kMaxCount || b.SG > (size_t)ds::kMaxCount || b.T > ds::kMaxCount || b.TA > ds::kMaxCount)
    return fail(ctx, S3S_E_UNSUPPORTED, "batch too large for one call");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& v : ctx->stage_ms) v = 0;
  if ((rc = batch_layout(b))) return rc;
  // the host copies of IVs the arena holds - the carried ones in the descriptors, the gathered ones - go with the call, as a
  // stream's own copy goes with the stream; before a single feed lays the staging area out anew
  struct WipeIvs {
    Batch& b;
    bool done = false;
    void now() {
      if (b.enc && !done) {
        wipe(b.A.hs + b.A.aw, b.A.atw - b.A.aw);
        wipe(b.A.hs + b.A.iv, b.iv_bytes);
      }
      done = true;
    }
    ~WipeIvs() { now(); }
  } wipe_ivs{b};
  if ((rc = batch_discover(b))) return rc;                      // wait 1: decrypt + checksums + discovery
  if (b.total_frames > 0 && (rc = batch_cut(b))) return rc;     // wait 2: frame tables + cut
  batch_verdicts(b);
  if (b.any_decode || b.n_second > 0) {
    int32_t dec_status;
    if ((rc = batch_decode(b, &dec_status))) return rc;         // wait 3: decode + the second checksum launch
    if (dec_status != 0) {
      // some frame of the batch is corrupt, or an LZ4 frame is above 32 MiB: nothing was committed, so the single feed answers
      // for every undecided entry (and runs the ring decoder where that is what the frame needs)
      std::vector<int32_t> todo;
      for (const BatchWin& w : b.W)
        if (!w.decided) todo.push_back(w.e);
      ctx->dstream_batch_entries = b.m - (int32_t)todo.size();  // what the batch decided itself
      wipe_ivs.now();
      for (int32_t i : todo) b.single(E[i]);
      return verdict.finish(b.first_error());
    }
  }
  batch_commit(b);
  ctx->dstream_batch_entries = b.m;
  return verdict.finish(b.first_error());
}

int s3s_dstream_feed_batch(s3s_ctx* ctx, s3s_dstream_feed_entry* E, int32_t n_entries) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  ctx->dstream_batch_entries = 0;
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

