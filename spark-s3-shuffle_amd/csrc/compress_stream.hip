// compress_stream.hip — the streaming map side of the C-ABI: a map output compressed window by window, in bounded memory.
//
// The reference never holds a map output: S3ShuffleMapOutputWriter.scala:43-49 puts a BufferedOutputStream of
// dispatcher.bufferSize in front of the object, :136-202 writes partition after partition through a codec stream and learns
// each partition's length as it closes.  An s3s_cstream does the same with the one-shot path's kernels: LZ4Block frames,
// Snappy chunks and LZF chunks are independent blocks cut at multiples of the block size from the partition's start, so a
// stream that takes only whole blocks needs no device memory between feeds and writes the bytes of the one-shot call.
//
// Both feeds are the same phases: checks, plan, device work, take.  The rules of the first, second and last are HIP-free
// functions of compress_stream_batch_core.h (over compress_stream_core.h) that the sanitized model programs call too; this file
// holds what needs the context: the codec's functors (CsCodec), the buffers, the copies, the launches and the error texts.
//
// A feed plans its window as a batch of ONE on the host, launches the unchanged codec kernels into slots, scans the item sizes
// (launch_scan_items), cuts the plan at the caller's capacity on the device (cstream_cut_kernel), gathers the items in front of
// the cut (gather_items_cut_kernel, compress_stream_kernels.hip, reads the cut from device memory) and runs the checksums over
// the pieces of partitions in the output, seeded with the open partition's carried state.  ONE host wait per feed, at its end.
// (A workspace buffer that has to grow waits once more, as everywhere: ensure().)
//
// Under IO encryption (s3s_cstream_open_encrypted) a kItemIv record goes in front of the items of every unit that
// starts its partition, launch_seed_iv_items gives it its 16 bytes before the scan, and one more kernel (aes_ctr_cstream.hip)
// encrypts d_dst[0, out_len) in place behind the cut gather and in front of the checksums; S3S_CODEC_NONE is cut on the host
// (none_cut_encrypted) and written by the same kernel from the source.  The feed's IVs are one upload; still one wait.
// The batched feed of streams under IO encryption carries the call's IVs, one pass descriptor per window and the
// pass's tile -> window map in its ONE upload and encrypts the outputs of all windows in ONE launch (aes_ctr_cstream_batch.hip).
#include <algorithm>
#include <new>
#include <optional>
#include <vector>

#include "compress_stream_batch_core.h"
#include "compress_stream_core.h"
#include "s3s_ctx.h"

using namespace s3s;

struct s3s_cstream {
  s3s_ctx* ctx;
  int codec, algo;
  int64_t bs;  // the block size in force at open (0: S3S_CODEC_NONE)
  int lz4_variant, snappy_variant;
  s3s_cs::State st;
  int64_t carry;  // checksum state of the open partition over the image bytes written so far
  // s3s_cstream_open_encrypted: the key setting the stream is bound to (s3s_ctx::enc_epoch) and the open partition's IV while
  // it has image bytes (host state; wiped when the partition closes and at close)
  bool enc = false;
  uint64_t epoch = 0;
  uint8_t iv[16] = {};
};

namespace {

using Entry = s3s_cstream_feed_entry;  // a window with its answer; the single feed makes one of its arguments

inline int64_t fresh(int algo) { return algo == S3S_CHECKSUM_ADLER32 ? 1 : 0;  }  // getValue() of a new Adler32 / CRC32 / CRC32C

inline int64_t need_src_unit(const s3s_cstream* s) { return s->codec == S3S_CODEC_NONE ? 1 : s->bs; }

inline size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

inline bool with_sums(const s3s_cstream* s) { return s->algo != S3S_CHECKSUM_NONE; }

inline uint8_t* carried_iv(s3s_cstream* s) { return s->enc ? s->iv : nullptr; }

// ---- the error texts that more than one path answers with ------------------------------------------------------------------------
int fail_need_dst(s3s_ctx* ctx, const Entry& e) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
  return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld image bytes of the next unit", (long long)e.dst_capacity, (long long)e.result.need_dst);
}
int fail_iv_count(s3s_ctx* ctx, int64_t want) {
  return fail(ctx, S3S_E_INVALID, "the entries of the batch have %lld pieces (n_ends + 1 each), s3s_set_stream_ivs gave %lld IVs", (long long)want,
              (long long)ctx->iv_cur_n);
}
int fail_entries(s3s_ctx* ctx) { return fail(ctx, S3S_E_INVALID, "null entry array or negative count"); }

inline bool null_with_length(const Entry& e) {
  return (e.src_len > 0 && !e.d_src) || (e.dst_capacity > 0 && !e.d_dst) ||
         (e.n_ends > 0 && (!e.part_ends || !e.out_lengths || (with_sums(e.stream) && !e.out_checksums)));
}
inline bool refused(const Entry& e) { return s3s_cs::window_refused(e.src_len, e.part_ends, e.n_ends, e.dst_capacity, null_with_length(e)); }

// ---- what the codec of a stream makes of a unit (s3s_ctx.h): the functors of the HIP-free core, and the codec launch -------------
struct CsCodec {
  const s3s_cstream* s0;  // the stream, or the first of a batch: its codec, block size and variants are the call's
  int codec;
  int64_t bs;
  bool enc;
  int level;
  CsCodec(const s3s_cstream* s, bool encrypted)
      : s0(s), codec(s->codec), bs(s->bs), enc(encrypted), level(s->codec == S3S_CODEC_LZ4 ? lz4_level(s->bs) : 0) {}

  int64_t items_of(const s3s_cs::Unit& u) const { return codec == S3S_CODEC_SNAPPY ? u.first + snappy_chunk_items(u.len) : 1; }
  int64_t slots_of(const s3s_cs::Unit& u) const { return codec == S3S_CODEC_SNAPPY ? snappy_chunk_slots(u.len) : u.len > 0; }
  s3s_cs::Count count(const Entry& e) const {
    return s3s_cs::count_window(codec, bs, e.stream->st.open_bytes, e.src_len, e.part_ends, e.n_ends, enc,
                                [&](const s3s_cs::Unit& u) { return items_of(u); }, [&](const s3s_cs::Unit& u) { return slots_of(u); });
  }
  // checksum segments of every piece, from an upper bound of its image bytes (a stream header and an end frame on top of what
  // the one-shot call allows a partition of the piece's source bytes, and its IV); < 0: "window too large for one feed"
  int64_t segs(const Entry& e, int32_t* seg_start) const {
    return s3s_cs::piece_segs(e.src_len, e.part_ends, e.n_ends, seg_start, [&](int64_t bytes) {
      return worst_segs(max_partition_size(codec, bs, bytes) + kLz4FrameHeader + kSnappyStreamHeader + (enc ? 16 : 0));
    });
  }
  // The plan records of a window at its places in the call's arrays, sources seen from the call's base pointer (delta).
  // false: they do not match the count the window was reserved with
  bool plan(s3s_cs::CutEntry* c, const Entry& e, int64_t delta, Item* items, s3s_cs::Mark* marks, int32_t* part_first) const {
    return s3s_cs::plan_entry_records(
        c, codec, bs, e.stream->st.open_bytes, e.src_len, e.part_ends, e.n_ends, marks, part_first, enc, [&](const s3s_cs::Unit& u) { return items_of(u); },
        [&](const s3s_cs::Unit& u, int32_t at) { items[at] = Item{0, 0, kItemIv, -1, u.piece}; },  // the hole the encrypt pass fills
        [&](const s3s_cs::Unit& u, int32_t at, int32_t& slot) {
          if (codec == S3S_CODEC_SNAPPY && u.first) items[at++] = Item{0, 0, kItemSnappyHeader, -1, u.piece};
          if (u.len > 0) plan_codec_block(items, at, slot, codec, level, delta + u.src_off, u.len, u.piece, false);
          else if (codec == S3S_CODEC_LZ4) items[at] = Item{0, 0, kItemLz4End | (level << 8), -1, u.piece};  // (plan_units: LZ4 alone has a unit without bytes)
        });
  }
  int64_t slot_stride() const { return compress_slot_stride(codec, bs); }
  int launch(s3s_ctx* ctx, const uint8_t* base, const Item* d_items, int32_t n_items) const {
    if (codec == S3S_CODEC_LZ4) {
      ctx->lz4_variant_used = s0->lz4_variant;
      launch_lz4_compress(base, d_items, n_items, dev<uint32_t>(ctx, B_ITEM_CHECK), dev<uint8_t>(ctx, B_SLOTS), (int32_t)slot_stride(),
                          dev<uint32_t>(ctx, B_ITEM_SIZE), dev<uint32_t>(ctx, B_WORK), (s0->lz4_variant == 11 ? 8 : 10) * ctx->cu_count,
                          s0->lz4_variant, ctx->stream, nullptr, bs >= kLz4U32From);
    } else if (codec == S3S_CODEC_LZF) {
      launch_lzf_compress(base, d_items, n_items, dev<uint8_t>(ctx, B_SLOTS), slot_stride(), dev<uint32_t>(ctx, B_ITEM_SIZE), ctx->stream);
    } else {
      launch_snappy_compress(base, d_items, n_items, dev<uint8_t>(ctx, B_SLOTS), slot_stride(), dev<uint32_t>(ctx, B_ITEM_SIZE), s0->snappy_variant,
                             ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return S3S_OK;
  }
};

// the arrays of a call's s3s_cs::Arena in the pinned staging area
struct CsStage {
  uint8_t* hs;
  Item* items;
  s3s_cs::Mark* marks;
  int32_t *pf, *seg, *pw, *status;
  int64_t *seed, *res, *piece, *len, *sums;
  uint8_t* ivs;
  template <typename T>
  T* at(size_t off) const { return reinterpret_cast<T*>(hs + off); }
  CsStage(s3s_ctx* ctx, const s3s_cs::Arena& A)
      : hs(static_cast<uint8_t*>(ctx->h_stage)), items(at<Item>(A.items)), marks(at<s3s_cs::Mark>(A.marks)), pf(at<int32_t>(A.pf)),
        seg(at<int32_t>(A.seg)), pw(at<int32_t>(A.pw)), status(at<int32_t>(A.status)), seed(at<int64_t>(A.seed)), res(at<int64_t>(A.res)),
        piece(at<int64_t>(A.piece)), len(at<int64_t>(A.len)), sums(at<int64_t>(A.sums)), ivs(hs + A.ivs) {}
};

s3s_cs::Arena lay_out(const s3s_cs::Totals& tot, bool enc, int64_t tiles) {
  s3s_cs::Arena A;
  if (enc) A.lay_out_encrypted(tot, sizeof(Item), sizeof(TaskTail), sizeof(s3s_cs::PassWindow), tiles);
  else A.lay_out(tot, sizeof(Item), sizeof(TaskTail));
  return A;
}

// Window wi of a call into the staging arrays: plan records, seeds, and under IO encryption its
// IVs (slice: the window's own of the call's; entry 0 is the stream's while the open partition already has image bytes)
bool stage_window(const CsCodec& k, const CsStage& h, s3s_cs::CutEntry* c, int32_t wi, const Entry& e, int64_t delta,
                  const uint8_t* slice) {
  const s3s_cstream* s = e.stream;
  if (!k.plan(c, e, delta, h.items, h.marks, h.pf)) return false;
  s3s_cs::seed_pieces(*c, wi, s->carry, fresh(s->algo), h.seed, h.pw);
  if (k.enc) s3s_cs::window_ivs(*c, slice, 0, s->iv, h.ivs);
  return true;
}

// behind the download: the words of a window's cut, checked
bool words_ok(const CsStage& h, int32_t wi, const s3s_cs::CutEntry& c, const Entry& e, s3s_cs::Cut* cut) {
  return s3s_cs::cut_from_words(h.res + (size_t)s3s_cs::kCutWords * (size_t)wi, h.status[wi], c.n_items, e.src_len, e.dst_capacity, e.n_ends, cut);
}
// ... and taken: the stream moves, the entry has its answer
int take(s3s_ctx* ctx, const CsStage& h, const s3s_cs::CutEntry& c, const s3s_cs::Cut& cut, Entry& e) {
  s3s_cstream* s = e.stream;
  if (!s3s_cs::take_window(&s->st, &s->carry, carried_iv(s), cut, e.part_ends, h.piece + c.first_pp, h.len + c.first_len,
                           with_sums(s) ? h.sums + c.first_piece : nullptr, h.ivs + 16 * (size_t)c.first_piece, e.out_lengths, e.out_checksums, &e.result))
    return fail_need_dst(ctx, e);
  return S3S_OK;
}

int open_stream(s3s_ctx* ctx, int codec, int checksum_algo, bool encrypted, s3s_cstream** out) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  if (!out) return fail(ctx, S3S_E_INVALID, "null/invalid argument");
  *out = nullptr;
  if (codec != S3S_CODEC_NONE && codec != S3S_CODEC_LZ4 && codec != S3S_CODEC_SNAPPY && codec != S3S_CODEC_ZSTD && codec != S3S_CODEC_LZF)
    return fail(ctx, S3S_E_INVALID, "unknown codec %d", codec);
  if (checksum_algo != S3S_CHECKSUM_NONE && checksum_algo != S3S_CHECKSUM_ADLER32 && checksum_algo != S3S_CHECKSUM_CRC32 &&
      checksum_algo != S3S_CHECKSUM_CRC32C)
    return fail(ctx, S3S_E_INVALID, "unknown checksum algorithm %d", checksum_algo);
  if (codec == S3S_CODEC_ZSTD)  // the frame header carries the content size of a partition whose end a stream has not seen
    return fail(ctx, S3S_E_UNSUPPORTED, "Zstandard map outputs are not streamed: the frame header holds the partition's size (use s3s_compress_map_output*)");
  if (codec == S3S_CODEC_LZF && !ctx->lzf_compress)
    return fail(ctx, S3S_E_UNSUPPORTED, "lzf compression stays on the JVM codec (S3S_OPT_LZF_COMPRESS is 0)");
  if (encrypted && !enc_on(ctx)) return fail(ctx, S3S_E_INVALID, "s3s_cstream_open_encrypted on a context without IO encryption");
  if (!encrypted && enc_on(ctx))  // the caller has to know the IV unit and set IVs: s3s_cstream_open_encrypted is the opt-in
    return fail(ctx, S3S_E_UNSUPPORTED, "map outputs under IO encryption are streamed by s3s_cstream_open_encrypted");
  if (codec == S3S_CODEC_SNAPPY && !snappy_compress_available())
    return fail(ctx, S3S_E_UNSUPPORTED, "snappy compression is not available in this build");
  s3s_cstream* s = new (std::nothrow) s3s_cstream();
  if (!s) return fail(ctx, S3S_E_NOMEM, "out of host memory");
  s->ctx = ctx;
  s->codec = codec;
  s->algo = checksum_algo;
  s->bs = effective_block(ctx, codec);
  s->lz4_variant = ctx->lz4_variant == 9 ? 11 : ctx->lz4_variant;  // auto: no timing rounds in a stream, as in a batched call
  s->snappy_variant = ctx->snappy_variant;
  s->carry = fresh(checksum_algo);
  s->enc = encrypted;
  s->epoch = ctx->enc_epoch;
  *out = s;
  return S3S_OK;
}

// ---- the single feed, phase by phase ----------------------------------------------------------------------------------------
// checks: the arguments, the key setting the stream is bound to, one IV per piece - before anything is launched
int feed_checks(const Entry& e) {
  const s3s_cstream* s = e.stream;
  s3s_ctx* ctx = s->ctx;
  if (refused(e))
    return fail(ctx, S3S_E_INVALID, "%s",
                e.src_len < 0 || e.n_ends < 0 || e.dst_capacity < 0 ? "negative size"
                : null_with_length(e)                                ? "null pointer with a non-zero length"
                                                                     : "part_ends must be ascending offsets inside the window");
  if (s->enc && (s->epoch != ctx->enc_epoch || !enc_on(ctx)))  // bound to the key setting it was opened under: it can only be closed
    return fail(ctx, S3S_E_INVALID, "s3s_set_io_encryption was called after the stream was opened: the stream can only be closed");
  if (!s->enc && enc_on(ctx)) return fail(ctx, S3S_E_UNSUPPORTED, "IO encryption was switched on after the stream was opened");
  return s->enc ? enc_check_ivs(ctx, e.n_ends + 1) : S3S_OK;  // the partitions that end in the window, and the one it leaves open
}

// device work, first step: the buffers of every feed, the status and result words zeroed, the feed's IVs (staged at h_ivs) up
int feed_begin(const Entry& e, const uint8_t* h_ivs) {
  s3s_ctx* ctx = e.stream->ctx;
  const size_t n_pieces = (size_t)e.n_ends + 1;
  int rc;
  if ((rc = ensure(ctx, B_INDEX, 8 * (n_pieces + 1)))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * (n_pieces + 1)))) return rc;
  if ((rc = ensure(ctx, B_REF_SUMS, 8 * (n_pieces + 1)))) return rc;
  if ((rc = ensure(ctx, B_STATUS, 128))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, 128, ctx->stream));
  if (e.stream->enc) {
    if ((rc = ensure(ctx, B_IVS, 16 * n_pieces))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_IVS].p, h_ivs, 16 * n_pieces, hipMemcpyHostToDevice, ctx->stream));
  }
  return S3S_OK;
}

// device work, last step: the checksums over the pieces as the cut left them (offsets in B_INDEX), the open partition's state
// as the first piece's seed; the status word; the feed's ONE wait
int feed_sums_and_wait(const Entry& e, const int32_t* h_seg, const int64_t* h_seed, int64_t* h_sums, int32_t* h_status) {
  const s3s_cstream* s = e.stream;
  s3s_ctx* ctx = s->ctx;
  const int32_t n_pieces = e.n_ends + 1;
  int64_t* d_piece = dev<int64_t>(ctx, B_INDEX);
  int rc;
  if (with_sums(s)) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_REF_SUMS].p, h_seed, 8 * (size_t)n_pieces, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_checksum(ctx, s->algo, e.d_dst, d_piece, n_pieces, h_seg, dev<int64_t>(ctx, B_SUMS), e.dst_capacity))) return rc;
    launch_checksum_seed(s->algo, d_piece, n_pieces, ctx->buf[B_TABLES].p, dev<int64_t>(ctx, B_REF_SUMS), dev<int64_t>(ctx, B_SUMS), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_sums, ctx->buf[B_SUMS].p, 8 * (size_t)n_pieces, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipMemcpyAsync(h_status, ctx->buf[B_STATUS].p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return S3S_OK;
}

// spark.shuffle.compress=false: the partition bytes are the image, the cut is known on the host.  Under IO encryption:
// IV | window bytes XOR key stream, in one pass from the source
int feed_none(Entry& e) {
  s3s_cstream* s = e.stream;
  s3s_ctx* ctx = s->ctx;
  const bool enc = s->enc;
  const int32_t n_ends = e.n_ends, n_pieces = n_ends + 1;
  const int64_t front = s->st.open_img;  // stored bytes of the open partition that earlier feeds wrote
  const s3s_cs::Cut c = enc ? s3s_cs::none_cut_encrypted(front, e.src_len, e.part_ends, n_ends, e.dst_capacity, nullptr)
                            : s3s_cs::none_cut(e.src_len, e.part_ends, n_ends, e.dst_capacity);
  if (c.need_dst) {
    e.result.need_dst = c.need_dst;
    return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld", (long long)e.dst_capacity, (long long)c.need_dst);
  }
  if (c.out_len == 0) {  // nothing to write: no device work
    s3s_cs::answer_on_host(&s->st, &s->carry, carried_iv(s), fresh(s->algo), c, e.out_lengths, e.out_checksums, &e.result);
    return S3S_OK;
  }
  // pinned staging: [seg_start n_pieces + 1][piece offsets n_pieces + 1][seeds n_pieces] | down: [sums n_pieces][status]
  //                 encrypted, up: [IVs n_pieces][plain piece offsets n_pieces + 1]
  const size_t np1 = (size_t)n_pieces + 1;
  const size_t o_up = al16(4 * np1), o_seed = al16(o_up + 8 * np1), o_sums = al16(o_seed + 8 * np1), o_status = al16(o_sums + 8 * np1),
               o_ivs = o_status + 16, o_plain = al16(o_ivs + 16 * (size_t)n_pieces);
  int rc;
  if ((rc = ensure_stage(ctx, enc ? o_plain + 8 * np1 : o_ivs))) return rc;
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  int32_t* h_seg = reinterpret_cast<int32_t*>(hs);
  int64_t* h_up = reinterpret_cast<int64_t*>(hs + o_up);
  int64_t* h_seed = reinterpret_cast<int64_t*>(hs + o_seed);
  int64_t* h_plain = reinterpret_cast<int64_t*>(hs + o_plain);
  uint8_t* h_ivs = hs + o_ivs;
  s3s_cs::CutEntry pieces = {};  // (the pieces of a plan of one window without items)
  pieces.n_pieces = n_pieces;
  pieces.open_img = front;
  if (CsCodec(s, enc).segs(e, h_seg) < 0) return fail(ctx, S3S_E_UNSUPPORTED, "window too large for one feed");
  s3s_cs::seed_pieces(pieces, 0, s->carry, fresh(s->algo), h_seed, nullptr);
  if (enc) s3s_cs::window_ivs(pieces, ctx->iv_cur, 0, s->iv, h_ivs);
  if ((rc = feed_begin(e, h_ivs))) return rc;
  int64_t* d_piece = dev<int64_t>(ctx, B_INDEX);
  if (enc) {
    s3s_cs::none_cut_encrypted(front, e.src_len, e.part_ends, n_ends, e.dst_capacity, h_up);
    h_plain[0] = 0;
    for (int32_t j = 0; j < n_ends; j++) h_plain[j + 1] = e.part_ends[j];
    h_plain[n_pieces] = e.src_len;
    if ((rc = ensure(ctx, B_CRYPT_OFF, 8 * np1))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_piece, h_up, 8 * np1, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_CRYPT_OFF].p, h_plain, 8 * np1, hipMemcpyHostToDevice, ctx->stream));
    launch_aes_ctr_cstream(kCsFromPlain, ctx->enc_keys, ctx->enc_rounds, e.d_src, e.d_dst, d_piece, dev<int64_t>(ctx, B_CRYPT_OFF),
                           dev<uint8_t>(ctx, B_IVS), nullptr, n_pieces, front, c.out_len, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    h_up[0] = 0;
    for (int32_t j = 0; j < n_ends; j++) h_up[j + 1] = e.part_ends[j] < c.out_len ? e.part_ends[j] : c.out_len;
    h_up[n_pieces] = c.out_len;
    HIP_TRY(ctx, hipMemcpyAsync(e.d_dst, e.d_src, (size_t)c.out_len, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_piece, h_up, 8 * np1, hipMemcpyHostToDevice, ctx->stream));
  }
  int64_t* h_sums = reinterpret_cast<int64_t*>(hs + o_sums);
  if ((rc = feed_sums_and_wait(e, h_seg, h_seed, h_sums, reinterpret_cast<int32_t*>(hs + o_status)))) return rc;
  s3s_cs::take_window(&s->st, &s->carry, carried_iv(s), c, e.part_ends, h_up, nullptr, with_sums(s) ? h_sums : nullptr, h_ivs, e.out_lengths,
                      e.out_checksums, &e.result);  // (need_dst was answered in front of the device work)
  return S3S_OK;
}

// A codec's window: the plan is a batch of ONE on the host (the records, places and staging layout of the batched feed with
// every first_* = 0); the device work keeps the single kernels and its own copies into the context's buffers
int feed_codec(Entry& e) {
  s3s_cstream* s = e.stream;
  s3s_ctx* ctx = s->ctx;
  const bool enc = s->enc;
  const CsCodec k(s, enc);
  const int32_t n_pieces = e.n_ends + 1;
  int rc;
  // ---- plan ----------------------------------------------------------------------------------------------------------------
  const s3s_cs::Count n = k.count(e);
  if (n.items > s3s_cs::kBatchMax) return fail(ctx, S3S_E_UNSUPPORTED, "too many codec blocks in one window");
  if (n.items == 0) {  // nothing to write: no device work
    s3s_cs::answer_on_host(&s->st, &s->carry, carried_iv(s), fresh(s->algo), s3s_cs::cut_nothing(e.n_ends, need_src_unit(s)), e.out_lengths,
                           e.out_checksums, &e.result);
    return S3S_OK;
  }
  s3s_cs::Totals tot;  // (the segments are sized straight into the staging area, below: the single kernels do not read n_segs)
  s3s_cs::CutEntry c = s3s_cs::reserve(&tot, n.items, n.slots, e.n_ends, 0, e.dst_capacity, s->st.open_img);
  const s3s_cs::Arena A = lay_out(tot, enc, 0);
  if ((rc = ensure_stage(ctx, A.total))) return rc;
  const CsStage h(ctx, A);
  if (k.segs(e, h.seg) < 0) return fail(ctx, S3S_E_UNSUPPORTED, "window too large for one feed");
  if (!stage_window(k, h, &c, 0, e, 0, ctx->iv_cur)) return fail(ctx, S3S_E_HIP, "the window's plan does not match its count");

  // ---- device work ---------------------------------------------------------------------------------------------------------
  if ((rc = feed_begin(e, h.ivs))) return rc;
  const size_t np1 = (size_t)n_pieces + 1, n_items = (size_t)c.n_items;
  if ((rc = ensure(ctx, B_ITEMS, sizeof(Item) * n_items + 16))) return rc;
  if ((rc = ensure(ctx, B_PLAN, sizeof(s3s_cs::Mark) * n_items + 16))) return rc;
  if ((rc = ensure(ctx, B_PART_FIRST, 4 * np1))) return rc;
  if ((rc = ensure(ctx, B_SLOTS, (size_t)k.slot_stride() * (size_t)(c.n_slots > 0 ? c.n_slots : 1)))) return rc;
  if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * (n_items + 1)))) return rc;
  if ((rc = ensure(ctx, B_ITEM_OFF, sizeof(int64_t) * (n_items + 1)))) return rc;
  if ((rc = ensure(ctx, B_ITEM_CHECK, sizeof(uint32_t) * (n_items + 1)))) return rc;
  if ((rc = ensure(ctx, B_WORK, 64))) return rc;
  if ((rc = ensure(ctx, B_OFFSETS, 8 * np1))) return rc;
  if ((rc = ensure(ctx, B_FRAME_OUT, 8 * np1))) return rc;
  const Item* d_items = dev<Item>(ctx, B_ITEMS);
  int64_t* d_piece = dev<int64_t>(ctx, B_INDEX);
  int32_t* d_status = dev<int32_t>(ctx, B_STATUS);
  int64_t* d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + 16);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_ITEMS].p, h.items, sizeof(Item) * n_items, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_PLAN].p, h.marks, sizeof(s3s_cs::Mark) * n_items, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_PART_FIRST].p, h.pf, 4 * np1, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = k.launch(ctx, e.d_src, d_items, c.n_items))) return rc;
  if (enc) launch_seed_iv_items(d_items, c.n_items, dev<uint32_t>(ctx, B_ITEM_SIZE), ctx->stream);
  // (the scan's own index - the unclamped piece offsets - goes to a buffer nobody reads: the cut kernel writes the clamped ones)
  launch_scan_items(d_items, dev<uint32_t>(ctx, B_ITEM_SIZE), c.n_items, dev<int64_t>(ctx, B_ITEM_OFF), dev<int32_t>(ctx, B_PART_FIRST), n_pieces,
                    dev<int64_t>(ctx, B_OFFSETS), ctx->stream);
  launch_cstream_cut(ctx->buf[B_PLAN].p, dev<int64_t>(ctx, B_ITEM_OFF), c.n_items, dev<int32_t>(ctx, B_PART_FIRST), n_pieces, e.dst_capacity,
                     c.first_last, c.ends0, c.open_img, d_result, d_piece, dev<int64_t>(ctx, B_FRAME_OUT), ctx->stream);
  launch_gather_items_cut(e.d_src, d_items, c.n_items, d_result, dev<uint8_t>(ctx, B_SLOTS), k.slot_stride(), dev<uint32_t>(ctx, B_ITEM_SIZE),
                          dev<int64_t>(ctx, B_ITEM_OFF), e.d_dst, e.dst_capacity, d_status, ctx->stream);
  if (enc) {  // IVs into the holes, key stream over the rest of d_dst[0, out_len): out_len is the cut kernel's, the grid a host bound
    const int64_t bound = s3s_cs::feed_bound_encrypted(k.codec, k.bs, e.src_len, e.n_ends);
    launch_aes_ctr_cstream(kCsInPlace, ctx->enc_keys, ctx->enc_rounds, nullptr, e.d_dst, d_piece, nullptr, dev<uint8_t>(ctx, B_IVS), d_result, n_pieces,
                           c.open_img, bound < e.dst_capacity ? bound : e.dst_capacity, ctx->stream);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(h.res, d_result, 8 * s3s_cs::kCutWords, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(h.piece, d_piece, 8 * np1, hipMemcpyDeviceToHost, ctx->stream));
  if (e.n_ends > 0) HIP_TRY(ctx, hipMemcpyAsync(h.len, ctx->buf[B_FRAME_OUT].p, 8 * (size_t)e.n_ends, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = feed_sums_and_wait(e, h.seg, h.seed, h.sums, h.status))) return rc;

  // ---- take: the words checked, then the stream moves -----------------------------------------------------------------------
  s3s_cs::Cut cut;
  if (!words_ok(h, 0, c, e, &cut)) return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible result");
  return take(ctx, h, c, cut, e);
}

}  // namespace

extern "C" {

int s3s_cstream_open(s3s_ctx* ctx, int codec, int checksum_algo, s3s_cstream** out) { return open_stream(ctx, codec, checksum_algo, false, out); }

int s3s_cstream_open_encrypted(s3s_ctx* ctx, int codec, int checksum_algo, s3s_cstream** out) {
  return open_stream(ctx, codec, checksum_algo, true, out);
}

int64_t s3s_cstream_position(const s3s_cstream* s) { return s ? s->st.pos : (int64_t)S3S_E_INVALID; }

int64_t s3s_cstream_written(const s3s_cstream* s) { return s ? s->st.written : (int64_t)S3S_E_INVALID; }

int64_t s3s_cstream_feed_bound(const s3s_cstream* s, int64_t src_len, int32_t n_ends) {
  if (!s || src_len < 0 || n_ends < 0) return S3S_E_INVALID;
  return s->enc ? s3s_cs::feed_bound_encrypted(s->codec, s->bs, src_len, n_ends) : s3s_cs::feed_bound(s->codec, s->bs, src_len, n_ends);
}

int s3s_cstream_close(s3s_cstream* s) {
  if (!s) return S3S_E_INVALID;
  const int rc = s->st.open_bytes == 0 ? S3S_OK : S3S_E_INVALID;  // otherwise the image ends inside a codec stream
  wipe(s->iv, sizeof s->iv);
  delete s;
  return rc;
}

int s3s_cstream_feed_device(s3s_cstream* s, const uint8_t* d_src, int64_t src_len, const int64_t* part_ends, int32_t n_ends,
                            uint8_t* d_dst, int64_t dst_capacity, int64_t* out_lengths, int64_t* out_checksums,
                            s3s_cstream_result* r) {
  if (!s || !r) return S3S_E_INVALID;
  s3s_ctx* ctx = s->ctx;
  ctx->err[0] = 0;
  memset(r, 0, sizeof *r);
  std::optional<IvScope> iv_scope;  // an encrypted stream's feed is a compress call: it consumes the IVs of s3s_set_stream_ivs either way
  if (s->enc) iv_scope.emplace(ctx);
  Entry e = {s, d_src, src_len, part_ends, n_ends, S3S_OK, d_dst, dst_capacity, out_lengths, out_checksums, {}};
  if (int rc = feed_checks(e)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!with_sums(s)) e.out_checksums = nullptr;
  const int rc = s->codec == S3S_CODEC_NONE ? feed_none(e) : feed_codec(e);
  *r = e.result;
  return rc;
}

int s3s_cstream_feed(s3s_cstream* s, const uint8_t* src, int64_t src_len, const int64_t* part_ends, int32_t n_ends, uint8_t* dst,
                     int64_t dst_capacity, int64_t* out_lengths, int64_t* out_checksums, s3s_cstream_result* r) {
  if (!s || !r) return S3S_E_INVALID;
  s3s_ctx* ctx = s->ctx;
  ctx->err[0] = 0;
  if (src_len < 0 || (src_len > 0 && !src) || dst_capacity < 0 || (dst_capacity > 0 && !dst)) {
    memset(r, 0, sizeof *r);
    return fail(ctx, S3S_E_INVALID, "null/invalid host buffer");
  }
  std::optional<IvScope> iv_scope;  // (the device form's scope nests in this one)
  if (s->enc) iv_scope.emplace(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  // both device buffers are the context's workspace, sized by the window and by dst_capacity: the caller's two bounds
  if ((rc = ensure(ctx, B_SRC, (size_t)src_len + 64))) return rc;
  if ((rc = ensure(ctx, B_DST, (size_t)dst_capacity + 64))) return rc;
  if (src_len > 0) HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_SRC].p, src, (size_t)src_len, hipMemcpyHostToDevice, ctx->stream));
  rc = s3s_cstream_feed_device(s, dev<uint8_t>(ctx, B_SRC), src_len, part_ends, n_ends, dev<uint8_t>(ctx, B_DST), dst_capacity,
                               out_lengths, out_checksums, r);
  if (rc != S3S_OK) return rc;
  if (r->out_len > 0) HIP_TRY(ctx, hipMemcpy(dst, ctx->buf[B_DST].p, (size_t)r->out_len, hipMemcpyDeviceToHost));
  return S3S_OK;
}

}  // extern "C"

// ---- the batched feed: one window of each of several streams per call ------------------------------------------
// The windows of all batched entries become ONE plan (compress_stream_batch_core.h lays the call's arrays out): one upload, one
// launch of the codec kernels over the blocks of all windows, one scan, one cut, one gather, one checksum pass, one download,
// ONE host wait.  No stream's state changes before the download has been checked.
namespace {

struct CsWin {
  int32_t e;  // its entry
  s3s_cs::CutEntry c;
  int64_t tiles = 0;  // under IO encryption: its tiles of the encrypt pass
};

struct CsBatch {
  s3s_ctx* ctx;
  Entry* E;
  int32_t n;
  std::vector<CsWin> W;
  std::vector<int32_t> host;  // entries the single feed answers without device work, in order
  bool enc = false;           // the batched path runs under IO encryption: every window is a keyed stream's
  int64_t tiles = 0;          // ... the grid of the encrypt pass
  // keyed streams on a keyed context: the call's IVs (the IvScope's) and where every entry's slice of them starts (n + 1)
  const uint8_t* call_ivs = nullptr;
  std::vector<int64_t> iv_at;

  const uint8_t* slice(int32_t i) const { return call_ivs + 16 * (size_t)iv_at[(size_t)i]; }
  void single(int32_t i) {
    Entry& e = E[i];
    if (call_ivs) {  // the entry's slice of the call's IVs
      ctx->iv_cur = slice(i);
      ctx->iv_cur_n = iv_at[(size_t)i + 1] - iv_at[(size_t)i];
    }
    e.status = s3s_cstream_feed_device(e.stream, e.d_src, e.src_len, e.part_ends, e.n_ends, e.d_dst, e.dst_capacity, e.out_lengths,
                                       e.out_checksums, &e.result);
  }
  int first_error() {
    for (int32_t i = 0; i < n; i++)
      if (E[i].status != S3S_OK) {
        char msg[sizeof ctx->err];
        snprintf(msg, sizeof msg, "%s", ctx->err);
        return fail(ctx, E[i].status, "entry %d of the batch failed%s%.400s", i, msg[0] ? ": " : "", msg);
      }
    return S3S_OK;
  }
};

// call-level refusals: nothing has been touched.  *batched: these streams go through the batched path - plain streams with
// the layer off, or, with the layer on, the streams of s3s_cstream_open_encrypted under the context's current key setting
// (a stream bound to an earlier one and a plain stream keep the single feed's refusal: cs_batch_windows sends them to b.host)
int cs_batch_check(CsBatch& b, bool* batched, bool* any_enc) {
  s3s_ctx* ctx = b.ctx;
  *batched = b.n > 1;
  *any_enc = false;
  std::vector<const s3s_cstream*> seen;
  seen.reserve((size_t)b.n);
  for (int32_t i = 0; i < b.n; i++) {
    const s3s_cstream* s = b.E[i].stream;
    if (!s) return fail(ctx, S3S_E_INVALID, "entry %d: null stream", i);
    if (s->ctx != ctx) return fail(ctx, S3S_E_INVALID, "entry %d: the stream was opened on another context", i);
    const s3s_cstream* s0 = b.E[0].stream;
    if (s->codec != s0->codec || s->algo != s0->algo)
      return fail(ctx, S3S_E_INVALID, "entry %d: the streams of a batch must share codec and checksum algorithm", i);
    if (s->enc) *any_enc = true;
    if ((s->enc && !enc_on(ctx)) || s->codec == S3S_CODEC_NONE || s->bs != s0->bs || s->lz4_variant != s0->lz4_variant || s->snappy_variant != s0->snappy_variant)
      *batched = false;
    seen.push_back(s);
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(ctx, S3S_E_INVALID, "the same stream twice in one batch");
  return S3S_OK;
}

// Which entries are windows of the batch: those whose single feed would launch something.  An entry the single feed refuses
// (by its arguments; under IO encryption a plain stream's S3S_E_UNSUPPORTED and a stale key setting's S3S_E_INVALID) and one
// whose window launches nothing or is too large for a feed keep that feed's answer (b.host).  false: the call does not fit one
// plan (an index would leave int32): it goes one by one
bool cs_batch_windows(CsBatch& b, const CsCodec& k, s3s_cs::Totals* tot) {
  for (int32_t i = 0; i < b.n; i++) {
    const Entry& e = b.E[i];
    const s3s_cstream* s = e.stream;
    const bool no = (b.enc && (!s->enc || s->epoch != b.ctx->enc_epoch)) || refused(e);
    const s3s_cs::Count n = no ? s3s_cs::Count() : k.count(e);
    const int64_t segs = !no && n.items > 0 && with_sums(s) ? k.segs(e, nullptr) : 0;  // (sized only where checksums run)
    if (s3s_cs::route_entry(no, n, segs) != s3s_cs::kRouteWindow) {
      b.host.push_back(i);
      continue;
    }
    if (!s3s_cs::fits_call(*tot, n.items, n.slots, e.n_ends, segs)) return false;
    CsWin w;
    w.e = i;
    w.c = s3s_cs::reserve(tot, n.items, n.slots, e.n_ends, segs, e.dst_capacity, s->st.open_img);
    if (b.enc) {
      w.tiles = s3s_cs::pass_tiles(e.dst_capacity, s3s_cs::feed_bound_encrypted(k.codec, k.bs, e.src_len, e.n_ends), s->st.open_img);
      if (b.tiles + w.tiles > s3s_cs::kBatchMax) return false;
      b.tiles += w.tiles;
    }
    b.W.push_back(w);
  }
  return true;
}

int cs_batch_run(CsBatch& b, const CsCodec& k, const s3s_cs::Totals& tot) {
  s3s_ctx* ctx = b.ctx;
  const int algo = k.s0->algo;
  const bool do_sum = with_sums(k.s0), enc = b.enc;
  const int32_t m = tot.m, N = (int32_t)tot.items;
  const size_t PP = (size_t)tot.pp(), P = (size_t)tot.pieces;
  const s3s_cs::Arena A = lay_out(tot, enc, b.tiles);
  const int64_t slot_stride = k.slot_stride();
  int rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = ensure_stage(ctx, A.total))) return rc;
  if ((rc = ensure(ctx, B_PLAN, A.total))) return rc;
  if ((rc = ensure(ctx, B_SLOTS, (size_t)slot_stride * (size_t)(tot.slots > 0 ? tot.slots : 1)))) return rc;  // a slot for every block of EVERY window
  if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * ((size_t)N + 1)))) return rc;
  if ((rc = ensure(ctx, B_ITEM_OFF, sizeof(int64_t) * ((size_t)N + (size_t)m + 1)))) return rc;
  if ((rc = ensure(ctx, B_ITEM_CHECK, sizeof(uint32_t) * ((size_t)N + 1)))) return rc;
  if ((rc = ensure(ctx, B_WORK, 64))) return rc;
  if ((rc = ensure(ctx, B_OFFSETS, 8 * PP))) return rc;
  if (do_sum && (rc = ensure(ctx, B_PARTIAL, 16 * (size_t)(tot.segs > 0 ? tot.segs : 1)))) return rc;
  const CsStage h(ctx, A);
  uint8_t* hs = h.hs;
  uint8_t* da = dev<uint8_t>(ctx, B_PLAN);
  TaskTail* h_tails = h.at<TaskTail>(A.tails);
  s3s_cs::CutEntry* h_cuts = h.at<s3s_cs::CutEntry>(A.cuts);
  s3s_cs::PassWindow* h_wins = h.at<s3s_cs::PassWindow>(A.wins);  // under IO encryption: the pass descriptors and the tile -> window map
  int32_t* h_tile_win = h.at<int32_t>(A.tile_win);
  int32_t tile0 = 0;

  const uint8_t* base = b.E[b.W[0].e].d_src;  // the one source pointer of the codec launch: every item is an offset from it
  memset(hs + A.seg, 0, A.seed - A.seg);
  for (int32_t wi = 0; wi < m; wi++) {
    CsWin& w = b.W[(size_t)wi];
    const Entry& e = b.E[w.e];
    const int64_t delta = s3s_cs::item_src_off((int64_t)reinterpret_cast<intptr_t>(e.d_src), (int64_t)reinterpret_cast<intptr_t>(base), 0);
    if (!stage_window(k, h, &w.c, wi, e, delta, enc ? b.slice(w.e) : nullptr))
      return fail(ctx, S3S_E_HIP, "the plan of entry %d does not match its count", w.e);
    if (do_sum) k.segs(e, h.seg + w.c.first_pp);
    h_cuts[wi] = w.c;
    TaskTail& t = h_tails[wi];
    t.first_item = w.c.first_item;
    t.n_items = w.c.n_items;
    t.first_pp = w.c.first_pp;
    t.n_parts = w.c.n_pieces;
    t.first_part = w.c.first_piece;
    t.first_seg = w.c.first_seg;
    t.n_segs = w.c.n_segs;
    t.pad = 0;
    t.data = e.d_dst;
    t.data_len = e.dst_capacity;
    t.dst = e.d_dst;
    t.dst_capacity = e.dst_capacity;
  }
  if (enc)  // (behind the loop: the plan has filled every CutEntry)
    for (int32_t wi = 0; wi < m; wi++) {
      h_wins[wi] = s3s_cs::pass_window(h_cuts, wi, b.E[b.W[(size_t)wi].e].d_dst, reinterpret_cast<const int64_t*>(da + A.piece), da + A.ivs,
                                       reinterpret_cast<const int64_t*>(da + A.res), tile0);
      tile0 = s3s_cs::map_tiles(h_tile_win, tile0, b.W[(size_t)wi].tiles, wi);
    }

  const TaskTail* d_tails = reinterpret_cast<const TaskTail*>(da + A.tails);
  const Item* d_items = reinterpret_cast<const Item*>(da + A.items);
  const int32_t* d_pf = reinterpret_cast<const int32_t*>(da + A.pf);
  int32_t* d_status = reinterpret_cast<int32_t*>(da + A.status);
  int64_t* d_result = reinterpret_cast<int64_t*>(da + A.res);
  int64_t* d_piece = reinterpret_cast<int64_t*>(da + A.piece);
  int64_t* d_len = reinterpret_cast<int64_t*>(da + A.len);
  int64_t* d_sums = reinterpret_cast<int64_t*>(da + A.sums);
  HIP_TRY(ctx, hipMemcpyAsync(da, hs, A.up, hipMemcpyHostToDevice, ctx->stream));  // the call's one upload
  HIP_TRY(ctx, hipMemsetAsync(da + A.up, 0, A.total - A.up, ctx->stream));
  if ((rc = k.launch(ctx, base, d_items, N))) return rc;
  if (enc) launch_seed_iv_items(d_items, N, dev<uint32_t>(ctx, B_ITEM_SIZE), ctx->stream);  // once, over the items of the whole call
  // (the scan's own index - the unclamped piece offsets - goes to a buffer nobody reads: the cut kernel writes the clamped ones)
  launch_scan_items_batch(d_tails, m, dev<uint32_t>(ctx, B_ITEM_SIZE), dev<int64_t>(ctx, B_ITEM_OFF), d_pf, dev<int64_t>(ctx, B_OFFSETS),
                          ctx->stream);
  launch_cstream_cut_batch(da + A.cuts, m, da + A.marks, dev<int64_t>(ctx, B_ITEM_OFF), d_pf, d_result, d_piece, d_len, ctx->stream);
  launch_gather_items_cut_batch(d_tails, m, N, base, d_items, d_result, dev<uint8_t>(ctx, B_SLOTS), slot_stride, dev<uint32_t>(ctx, B_ITEM_SIZE),
                                dev<int64_t>(ctx, B_ITEM_OFF), d_status, ctx->stream);
  if (enc)  // IVs into the holes, key stream over the rest of every d_dst[0, out_len): ONE launch, the grid a sum of host bounds
    launch_aes_ctr_cstream_batch(ctx->enc_keys, ctx->enc_rounds, da + A.wins, reinterpret_cast<const int32_t*>(da + A.tile_win), tile0, ctx->stream);
  if (do_sum) {  // over the pieces as the cuts left them (the stored bytes); a stream's carried state seeds its window's first piece
    launch_checksum_batch(algo, d_tails, m, (int32_t)tot.segs, (int32_t)P, d_piece, reinterpret_cast<const int32_t*>(da + A.seg),
                          ctx->buf[B_TABLES].p, dev<uint32_t>(ctx, B_PARTIAL), d_sums, ctx->stream);
    launch_checksum_seed_batch(algo, d_piece, reinterpret_cast<const int32_t*>(da + A.pw), (int32_t)P, ctx->buf[B_TABLES].p,
                               reinterpret_cast<const int64_t*>(da + A.seed), d_sums, ctx->stream);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(hs + A.up, da + A.up, A.total - A.up, hipMemcpyDeviceToHost, ctx->stream));  // the call's one download
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                                                          // ... and its one wait

  // every window's words are checked before any stream moves
  std::vector<s3s_cs::Cut> cuts((size_t)m);
  for (int32_t wi = 0; wi < m; wi++)
    if (!words_ok(h, wi, b.W[(size_t)wi].c, b.E[b.W[(size_t)wi].e], &cuts[(size_t)wi]))
      return fail(ctx, S3S_E_HIP, "the capacity cut of entry %d returned an impossible result", b.W[(size_t)wi].e);
  for (int32_t wi = 0; wi < m; wi++) {
    Entry& e = b.E[b.W[(size_t)wi].e];
    memset(&e.result, 0, sizeof e.result);
    e.status = take(ctx, h, b.W[(size_t)wi].c, cuts[(size_t)wi], e);
  }
  return S3S_OK;
}

}  // namespace

extern "C" {

int s3s_cstream_feed_batch_device(s3s_ctx* ctx, s3s_cstream_feed_entry* E, int32_t n) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  ctx->cstream_batch_entries = 0;  // S3S_OPT_CSTREAM_BATCH_ENTRIES: set where the batched path has answered
  ctx->cstream_batch_enc_entries = 0;  // S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES: the same under IO encryption (key 18 then stays 0)
  std::optional<IvScope> iv_scope;  // under IO encryption the call is a compress call: it consumes the IVs of s3s_set_stream_ivs either way
  if (enc_on(ctx)) iv_scope.emplace(ctx);
  if (n < 0 || (n > 0 && !E)) return fail_entries(ctx);
  BatchVerdict<s3s_cstream_feed_entry> verdict(E, n);
  if (n == 0) return verdict.finish(S3S_OK);
  CsBatch b = {ctx, E, n, {}, {}};
  bool batched, any_enc;
  int rc;
  if ((rc = cs_batch_check(b, &batched, &any_enc))) return rc;
  if (enc_on(ctx) && any_enc) {  // ONE array of IVs for the call, sliced in entry order: any other count before anything runs
    b.iv_at.resize((size_t)n + 1);  // (with the layer off every encrypted stream is stale: the single feed's refusal)
    const int64_t want = s3s_cs::slice_ivs(n, [&](int32_t i) { return E[i].n_ends; }, b.iv_at.data());
    if (ctx->iv_cur_n != want) return fail_iv_count(ctx, want);
    b.call_ivs = ctx->iv_cur;
  }
  if (enc_on(ctx) && !any_enc) batched = false;  // only plain streams on a keyed context: each one's S3S_E_UNSUPPORTED
  b.enc = batched && enc_on(ctx);
  const CsCodec k(E[0].stream, b.enc);
  s3s_cs::Totals tot;
  if (batched && !cs_batch_windows(b, k, &tot)) {  // the call does not fit one plan: nothing of the attempt stays
    batched = false;
    b.W.clear();
    b.host.clear();
    b.enc = false;
    b.tiles = 0;
  }
  if (!batched) {  // nothing to batch: one by one, in order
    for (int32_t i = 0; i < n; i++) b.single(i);
    return verdict.finish(b.first_error());
  }
  if (tot.m > 0 && (rc = cs_batch_run(b, k, tot))) return rc;
  for (int32_t i : b.host) b.single(i);  // (no device work: an argument the single feed refuses, a window that launches nothing)
  (b.enc ? ctx->cstream_batch_enc_entries : ctx->cstream_batch_entries) = tot.m;
  return verdict.finish(b.first_error());
}

int s3s_cstream_feed_batch(s3s_ctx* ctx, s3s_cstream_feed_entry* E, int32_t n) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  ctx->cstream_batch_entries = 0;
  ctx->cstream_batch_enc_entries = 0;
  if (n < 0 || (n > 0 && !E)) return fail_entries(ctx);
  BatchVerdict<s3s_cstream_feed_entry> verdict(E, n);
  if (n == 0) return verdict.finish(S3S_OK);
  // the windows and the destinations of ALL entries are staged in the context's workspace: the sum of src_len + dst_capacity
  // is the caller's memory bound.  An entry the single feed refuses by its buffers is staged as empty and keeps them
  auto al = [](int64_t x) { return (x + 255) & ~int64_t(255); };
  auto staged = [](const s3s_cstream_feed_entry& e) {
    return e.src_len >= 0 && e.dst_capacity >= 0 && (e.src_len == 0 || e.d_src) && (e.dst_capacity == 0 || e.d_dst);
  };
  std::vector<s3s_cstream_feed_entry> D(E, E + n);
  std::vector<int64_t> so((size_t)n), dso((size_t)n);
  int64_t src_total = 0, dst_total = 0;
  for (int32_t i = 0; i < n; i++) {
    so[(size_t)i] = src_total;
    dso[(size_t)i] = dst_total;
    if (staged(E[i])) {
      src_total += al(E[i].src_len + 64);
      dst_total += al(E[i].dst_capacity + 64);
    }
  }
  std::optional<IvScope> iv_scope;  // (the device form's scope nests in this one)
  if (enc_on(ctx)) iv_scope.emplace(ctx);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, B_SRC, (size_t)src_total + 64))) return rc;
  if ((rc = ensure(ctx, B_DST, (size_t)dst_total + 64))) return rc;
  for (int32_t i = 0; i < n; i++) {
    const s3s_cstream_feed_entry& e = E[i];
    if (!staged(e)) {  // the device form's single feed answers S3S_E_INVALID from the same arguments (a null pointer stays null)
      D[(size_t)i].d_src = e.d_src ? dev<uint8_t>(ctx, B_SRC) : nullptr;
      D[(size_t)i].d_dst = e.d_dst ? dev<uint8_t>(ctx, B_DST) : nullptr;
      continue;
    }
    D[(size_t)i].d_src = e.src_len > 0 ? dev<uint8_t>(ctx, B_SRC) + so[(size_t)i] : nullptr;
    D[(size_t)i].d_dst = e.dst_capacity > 0 ? dev<uint8_t>(ctx, B_DST) + dso[(size_t)i] : nullptr;
    if (e.src_len > 0) HIP_TRY(ctx, hipMemcpyAsync(dev<uint8_t>(ctx, B_SRC) + so[(size_t)i], e.d_src, (size_t)e.src_len, hipMemcpyHostToDevice, ctx->stream));
  }
  rc = s3s_cstream_feed_batch_device(ctx, D.data(), n);
  for (int32_t i = 0; i < n; i++) {
    E[i].result = D[(size_t)i].result;
    E[i].status = D[(size_t)i].status;
  }
  for (int32_t i = 0; i < n; i++)
    if (E[i].status == S3S_OK && E[i].result.out_len > 0)
      HIP_TRY(ctx, hipMemcpyAsync(E[i].d_dst, D[(size_t)i].d_dst, (size_t)E[i].result.out_len, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return verdict.finish(rc);
}

}  // extern "C"
