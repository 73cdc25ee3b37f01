// compress_stream.hip — the streaming map side of the C-ABI: a map output compressed window by window, in bounded memory.
//
// The reference never holds a map output: S3ShuffleMapOutputWriter.scala:43-49 puts a BufferedOutputStream of
// dispatcher.bufferSize in front of the object, :136-202 writes partition after partition through a codec stream and learns
// each partition's length as it closes.  An s3s_cstream does the same with the one-shot path's kernels: LZ4Block frames,
// Snappy chunks and LZF chunks are independent blocks cut at multiples of the block size from the partition's start, so a
// stream that takes only whole blocks needs no device memory between feeds and writes the bytes of the one-shot call.
//
// A feed plans the units of its window on the host (compress_stream_core.h), launches the unchanged codec kernels into slots,
// scans the item sizes (launch_scan_items), cuts the plan at the caller's capacity on the device (cstream_cut_kernel), gathers
// the items in front of the cut (gather_items_cut_kernel, compress_stream_kernels.hip, reads the cut from device memory) and runs the checksums over the
// pieces of partitions in the output, seeded with the open partition's carried state.  ONE host wait per feed, at its end.
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

inline int64_t fresh(int algo) { return algo == S3S_CHECKSUM_ADLER32 ? 1 : 0;  }  // getValue() of a new Adler32 / CRC32 / CRC32C

inline int64_t need_src_unit(const s3s_cstream* s) { return s->codec == S3S_CODEC_NONE ? 1 : s->bs; }

inline size_t al16(size_t x) { return (x + 15) & ~size_t(15); }

// the feed that wrote nothing: every end it passes closes a partition with what the stream already holds
void finish_on_host(s3s_cstream* s, const s3s_cs::Cut& c, const int64_t* ends, int64_t* out_lengths, int64_t* out_checksums) {
  s3s_cs::commit_nothing(&s->st, &s->carry, fresh(s->algo), c.parts_closed, out_lengths, out_checksums);
  if (s->enc) s3s_cs::commit_nothing_iv(s->iv, c.parts_closed);
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
  const bool enc = s->enc;
  const int codec = s->codec;
  const bool do_sum = s->algo != S3S_CHECKSUM_NONE;
  if (src_len < 0 || n_ends < 0 || dst_capacity < 0) return fail(ctx, S3S_E_INVALID, "negative size");
  if ((src_len > 0 && !d_src) || (dst_capacity > 0 && !d_dst) || (n_ends > 0 && (!part_ends || !out_lengths || (do_sum && !out_checksums))))
    return fail(ctx, S3S_E_INVALID, "null pointer with a non-zero length");
  if (!s3s_cs::ends_valid(src_len, part_ends, n_ends))
    return fail(ctx, S3S_E_INVALID, "part_ends must be ascending offsets inside the window");
  if (enc && (s->epoch != ctx->enc_epoch || !enc_on(ctx)))  // bound to the key setting it was opened under: it can only be closed
    return fail(ctx, S3S_E_INVALID, "s3s_set_io_encryption was called after the stream was opened: the stream can only be closed");
  if (!enc && enc_on(ctx)) return fail(ctx, S3S_E_UNSUPPORTED, "IO encryption was switched on after the stream was opened");
  const int32_t n_pieces = n_ends + 1;  // the partitions that end in the window, and the one it leaves open
  if (enc)  // one IV per piece, before anything is launched
    if (int iv_rc = enc_check_ivs(ctx, n_pieces)) return iv_rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!do_sum) out_checksums = nullptr;
  const int64_t bs = s->bs;
  const int64_t front = s->st.open_img;  // stored bytes of the open partition that earlier feeds wrote
  int rc;

  // ---- plan: count, then build ----------------------------------------------------------------------------------------------
  s3s_cs::Cut c;
  int64_t n_items64 = 0, n_slots64 = 0;
  s3s_cs::Plan plan;
  if (codec == S3S_CODEC_NONE) {
    c = enc ? s3s_cs::none_cut_encrypted(front, src_len, part_ends, n_ends, dst_capacity, nullptr)
            : s3s_cs::none_cut(src_len, part_ends, n_ends, dst_capacity);
    if (c.need_dst) {
      r->need_dst = c.need_dst;
      return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld", (long long)dst_capacity, (long long)c.need_dst);
    }
  } else {
    plan = s3s_cs::plan_units(codec, bs, s->st.open_bytes, src_len, part_ends, n_ends, [&](const s3s_cs::Unit& u) {
      if (codec == S3S_CODEC_SNAPPY) {
        n_items64 += s3s_cs::iv_records(u, enc) + u.first + snappy_chunk_items(u.len);
        n_slots64 += snappy_chunk_slots(u.len);
      } else {
        n_items64 += s3s_cs::iv_records(u, enc) + 1;
        n_slots64 += u.len > 0;
      }
    });
    if (n_items64 > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "too many codec blocks in one window");
    if (plan.n_units == 0) {
      c.parts_closed = n_ends;
      if (n_ends == 0) c.need_src = need_src_unit(s);
    }
  }
  const int32_t n_items = (int32_t)n_items64, n_slots = (int32_t)n_slots64;
  if (codec == S3S_CODEC_NONE ? c.out_len == 0 : n_items == 0) {  // nothing to write: no device work
    finish_on_host(s, c, part_ends, out_lengths, out_checksums);
    r->need_src = c.need_src;
    r->parts_closed = c.parts_closed;
    return S3S_OK;
  }

  // pinned staging: [items][marks][part_first n_pieces + 1][seg_start n_pieces + 1][piece offsets n_pieces + 1 (NONE: up)]
  //                 [seeds n_pieces] | down: [result][piece offsets n_pieces + 1][lengths n_ends][sums n_pieces][status]
  //                 encrypted, up: [IVs n_pieces][plain piece offsets n_pieces + 1 (NONE)]
  const size_t np1 = (size_t)n_pieces + 1;
  const size_t o_marks = al16(sizeof(Item) * (size_t)n_items), o_pf = al16(o_marks + sizeof(s3s_cs::Mark) * (size_t)n_items),
               o_seg = al16(o_pf + 4 * np1), o_up = al16(o_seg + 4 * np1), o_seed = al16(o_up + 8 * np1),
               o_res = al16(o_seed + 8 * np1), o_piece = al16(o_res + 8 * s3s_cs::kCutWords), o_len = al16(o_piece + 8 * np1),
               o_sums = al16(o_len + 8 * np1), o_status = al16(o_sums + 8 * np1), o_ivs = o_status + 16,
               o_plain = al16(o_ivs + 16 * (size_t)n_pieces), stage_total = enc ? o_plain + 8 * np1 : o_status + 16;
  if ((rc = ensure_stage(ctx, stage_total))) return rc;
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  Item* h_items = reinterpret_cast<Item*>(hs);
  s3s_cs::Mark* h_marks = reinterpret_cast<s3s_cs::Mark*>(hs + o_marks);
  int32_t* h_pf = reinterpret_cast<int32_t*>(hs + o_pf);
  int32_t* h_seg = reinterpret_cast<int32_t*>(hs + o_seg);
  int64_t* h_up = reinterpret_cast<int64_t*>(hs + o_up);
  int64_t* h_seed = reinterpret_cast<int64_t*>(hs + o_seed);
  int64_t* h_res = reinterpret_cast<int64_t*>(hs + o_res);
  int64_t* h_piece = reinterpret_cast<int64_t*>(hs + o_piece);
  int64_t* h_len = reinterpret_cast<int64_t*>(hs + o_len);
  int64_t* h_sums = reinterpret_cast<int64_t*>(hs + o_sums);
  int32_t* h_status = reinterpret_cast<int32_t*>(hs + o_status);
  uint8_t* h_ivs = hs + o_ivs;

  // checksum segments of every piece, from an upper bound of its image bytes (a stream header and an end frame on top of
  // what the one-shot call allows a partition of the piece's source bytes)
  int64_t segs = 0;
  for (int32_t j = 0; j < n_pieces; j++) {
    const int64_t a = j == 0 ? 0 : part_ends[j - 1], b = j < n_ends ? part_ends[j] : src_len;
    h_seg[j] = (int32_t)segs;
    segs += worst_segs(max_partition_size(codec, bs, b - a) + kLz4FrameHeader + kSnappyStreamHeader + (enc ? 16 : 0));
    h_seed[j] = j == 0 ? s->carry : fresh(s->algo);
    if (segs > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "window too large for one feed");
  }
  h_seg[n_pieces] = (int32_t)segs;

  if ((rc = ensure(ctx, B_INDEX, 8 * np1))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * np1))) return rc;
  if ((rc = ensure(ctx, B_REF_SUMS, 8 * np1))) return rc;
  if ((rc = ensure(ctx, B_STATUS, 128))) return rc;
  int64_t* d_piece = dev<int64_t>(ctx, B_INDEX);
  int32_t* d_status = dev<int32_t>(ctx, B_STATUS);
  int64_t* d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + 16);
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, 128, ctx->stream));
  if (enc) {  // the feed's IVs, one upload; entry 0 is the stream's own while the open partition already has image bytes
    if ((rc = ensure(ctx, B_IVS, 16 * (size_t)n_pieces))) return rc;
    memcpy(h_ivs, ctx->iv_cur, 16 * (size_t)n_pieces);
    if (front > 0) memcpy(h_ivs, s->iv, 16);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_IVS].p, h_ivs, 16 * (size_t)n_pieces, hipMemcpyHostToDevice, ctx->stream));
  }

  if (codec == S3S_CODEC_NONE && enc) {
    // spark.shuffle.compress=false under IO encryption: IV | window bytes XOR key stream, in one pass from the source
    int64_t* h_plain = reinterpret_cast<int64_t*>(hs + o_plain);
    s3s_cs::none_cut_encrypted(front, src_len, part_ends, n_ends, dst_capacity, h_up);
    h_plain[0] = 0;
    for (int32_t j = 0; j < n_ends; j++) h_plain[j + 1] = part_ends[j];
    h_plain[n_pieces] = src_len;
    if ((rc = ensure(ctx, B_CRYPT_OFF, 8 * np1))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_piece, h_up, 8 * np1, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_CRYPT_OFF].p, h_plain, 8 * np1, hipMemcpyHostToDevice, ctx->stream));
    launch_aes_ctr_cstream(kCsFromPlain, ctx->enc_keys, ctx->enc_rounds, d_src, d_dst, d_piece, dev<int64_t>(ctx, B_CRYPT_OFF),
                           dev<uint8_t>(ctx, B_IVS), nullptr, n_pieces, front, c.out_len, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
  } else if (codec == S3S_CODEC_NONE) {
    // spark.shuffle.compress=false: the partition bytes are the image; the cut is known on the host
    h_up[0] = 0;
    for (int32_t j = 0; j < n_ends; j++) h_up[j + 1] = part_ends[j] < c.out_len ? part_ends[j] : c.out_len;
    h_up[n_pieces] = c.out_len;
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, d_src, (size_t)c.out_len, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_piece, h_up, 8 * np1, hipMemcpyHostToDevice, ctx->stream));
  } else {
    // items, marks and the first item of every piece, in image order.  A unit's marks learn how many ends lie behind it when
    // the next unit arrives (that one's ends_before); the last unit's is every end of the window
    const int level = codec == S3S_CODEC_LZ4 ? lz4_level(bs) : 0;
    int32_t it = 0, slot = 0, piece = 0, first_last = -1, ends0 = 0, prev0 = 0;
    bool fits = true;  // the records stay inside what the count above sized
    h_pf[0] = 0;
    s3s_cs::plan_units(codec, bs, s->st.open_bytes, src_len, part_ends, n_ends, [&](const s3s_cs::Unit& u) {
      const int64_t mine = s3s_cs::iv_records(u, enc) + (codec == S3S_CODEC_SNAPPY ? u.first + snappy_chunk_items(u.len) : 1);
      if (!fits || it + mine > n_items) {
        fits = false;
        return;
      }
      s3s_cs::mark_ends_after(h_marks, prev0, it, u.ends_before);
      if (it == 0) ends0 = u.ends_before;
      while (piece < u.piece) h_pf[++piece] = it;
      prev0 = it;
      if (s3s_cs::iv_records(u, enc)) h_items[it++] = Item{0, 0, kItemIv, -1, u.piece};  // the hole the encrypt pass fills
      if (codec == S3S_CODEC_SNAPPY) {
        if (u.first) h_items[it++] = Item{0, 0, kItemSnappyHeader, -1, u.piece};
        snappy_plan_chunk(h_items, it, slot, u.src_off, u.len, u.piece);
      } else if (codec == S3S_CODEC_LZF) {
        h_items[it++] = Item{u.src_off, u.len, kItemLzfChunk, slot++, u.piece};
      } else if (u.len > 0) {
        h_items[it++] = Item{u.src_off, u.len, lz4_chunk_kind(u.len) | (level << 8), slot++, u.piece};
      } else {
        h_items[it++] = Item{0, 0, kItemLz4End | (level << 8), -1, u.piece};
      }
      s3s_cs::mark_unit(h_marks, prev0, it, u, n_ends);
      if (first_last < 0) first_last = it - 1;
    });
    while (piece < n_pieces) h_pf[++piece] = it;
    if (!fits || it != n_items || slot != n_slots) return fail(ctx, S3S_E_HIP, "the window's plan does not match its count");

    const int64_t slot_stride = codec == S3S_CODEC_SNAPPY ? snappy_slot_stride(bs) : codec_slot_stride(codec, bs);
    if ((rc = ensure(ctx, B_ITEMS, sizeof(Item) * (size_t)n_items + 16))) return rc;
    if ((rc = ensure(ctx, B_PLAN, sizeof(s3s_cs::Mark) * (size_t)n_items + 16))) return rc;
    if ((rc = ensure(ctx, B_PART_FIRST, 4 * np1))) return rc;
    if ((rc = ensure(ctx, B_SLOTS, (size_t)slot_stride * (size_t)(n_slots > 0 ? n_slots : 1)))) return rc;
    if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * (size_t)(n_items + 1)))) return rc;
    if ((rc = ensure(ctx, B_ITEM_OFF, sizeof(int64_t) * (size_t)(n_items + 1)))) return rc;
    if ((rc = ensure(ctx, B_ITEM_CHECK, sizeof(uint32_t) * (size_t)(n_items + 1)))) return rc;
    if ((rc = ensure(ctx, B_WORK, 64))) return rc;
    if ((rc = ensure(ctx, B_OFFSETS, 8 * np1))) return rc;
    if ((rc = ensure(ctx, B_FRAME_OUT, 8 * np1))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_ITEMS].p, h_items, sizeof(Item) * (size_t)n_items, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_PLAN].p, h_marks, sizeof(s3s_cs::Mark) * (size_t)n_items, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_PART_FIRST].p, h_pf, 4 * np1, hipMemcpyHostToDevice, ctx->stream));
    if (codec == S3S_CODEC_LZ4) {
      ctx->lz4_variant_used = s->lz4_variant;
      launch_lz4_compress(d_src, dev<Item>(ctx, B_ITEMS), n_items, dev<uint32_t>(ctx, B_ITEM_CHECK), dev<uint8_t>(ctx, B_SLOTS),
                          (int32_t)slot_stride, dev<uint32_t>(ctx, B_ITEM_SIZE), dev<uint32_t>(ctx, B_WORK),
                          (s->lz4_variant == 11 ? 8 : 10) * ctx->cu_count, s->lz4_variant, ctx->stream, nullptr, bs >= kLz4U32From);
    } else if (codec == S3S_CODEC_LZF) {
      launch_lzf_compress(d_src, dev<Item>(ctx, B_ITEMS), n_items, dev<uint8_t>(ctx, B_SLOTS), slot_stride,
                          dev<uint32_t>(ctx, B_ITEM_SIZE), ctx->stream);
    } else {
      launch_snappy_compress(d_src, dev<Item>(ctx, B_ITEMS), n_items, dev<uint8_t>(ctx, B_SLOTS), slot_stride,
                             dev<uint32_t>(ctx, B_ITEM_SIZE), s->snappy_variant, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (enc) launch_seed_iv_items(dev<Item>(ctx, B_ITEMS), n_items, dev<uint32_t>(ctx, B_ITEM_SIZE), ctx->stream);
    // (the scan's own index - the unclamped piece offsets - goes to a buffer nobody reads: the cut kernel writes the clamped ones)
    launch_scan_items(dev<Item>(ctx, B_ITEMS), dev<uint32_t>(ctx, B_ITEM_SIZE), n_items, dev<int64_t>(ctx, B_ITEM_OFF),
                      dev<int32_t>(ctx, B_PART_FIRST), n_pieces, dev<int64_t>(ctx, B_OFFSETS), ctx->stream);
    launch_cstream_cut(ctx->buf[B_PLAN].p, dev<int64_t>(ctx, B_ITEM_OFF), n_items, dev<int32_t>(ctx, B_PART_FIRST), n_pieces,
                       dst_capacity, first_last, ends0, s->st.open_img, d_result, d_piece, dev<int64_t>(ctx, B_FRAME_OUT),
                       ctx->stream);
    launch_gather_items_cut(d_src, dev<Item>(ctx, B_ITEMS), n_items, d_result, dev<uint8_t>(ctx, B_SLOTS), slot_stride,
                            dev<uint32_t>(ctx, B_ITEM_SIZE), dev<int64_t>(ctx, B_ITEM_OFF), d_dst, dst_capacity, d_status, ctx->stream);
    if (enc) {  // IVs into the holes, key stream over the rest of d_dst[0, out_len): out_len is the cut kernel's, the grid a host bound
      const int64_t bound = s3s_cs::feed_bound_encrypted(codec, bs, src_len, n_ends);
      launch_aes_ctr_cstream(kCsInPlace, ctx->enc_keys, ctx->enc_rounds, nullptr, d_dst, d_piece, nullptr, dev<uint8_t>(ctx, B_IVS), d_result,
                             n_pieces, front, bound < dst_capacity ? bound : dst_capacity, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_res, d_result, 8 * s3s_cs::kCutWords, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h_piece, d_piece, 8 * np1, hipMemcpyDeviceToHost, ctx->stream));
    if (n_ends > 0) HIP_TRY(ctx, hipMemcpyAsync(h_len, ctx->buf[B_FRAME_OUT].p, 8 * (size_t)n_ends, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (do_sum) {  // over the pieces as the cut left them, the open partition's state as the first piece's seed
    HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[B_REF_SUMS].p, h_seed, 8 * (size_t)n_pieces, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = run_checksum(ctx, s->algo, d_dst, d_piece, n_pieces, h_seg, dev<int64_t>(ctx, B_SUMS), dst_capacity))) return rc;
    launch_checksum_seed(s->algo, d_piece, n_pieces, ctx->buf[B_TABLES].p, dev<int64_t>(ctx, B_REF_SUMS), dev<int64_t>(ctx, B_SUMS), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_sums, ctx->buf[B_SUMS].p, 8 * (size_t)n_pieces, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipMemcpyAsync(h_status, d_status, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the feed's one wait

  const int64_t* piece_off = h_up;
  if (codec != S3S_CODEC_NONE) {
    piece_off = h_piece;
    if (!s3s_cs::cut_from_words(h_res, *h_status, n_items, src_len, dst_capacity, n_ends, &c))
      return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible result");
    if (c.need_dst > 0) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
      r->need_dst = c.need_dst;
      return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld image bytes of the next unit", (long long)dst_capacity, (long long)c.need_dst);
    }
  }
  // (the commit step the batched feed shares: compress_stream_batch_core.h)
  s3s_cs::commit(&s->st, &s->carry, c, part_ends, piece_off, codec != S3S_CODEC_NONE ? h_len : nullptr, do_sum ? h_sums : nullptr, out_lengths,
                 out_checksums);
  if (enc) s3s_cs::commit_iv(s->iv, s->st, front, c.parts_closed, h_ivs);  // (shared with the batched feed, like commit)
  r->consumed = c.consumed;
  r->out_len = c.out_len;
  r->parts_closed = c.parts_closed;
  return S3S_OK;
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
  s3s_cstream_feed_entry* E;
  int32_t n;
  std::vector<CsWin> W;
  std::vector<int32_t> host;  // entries the single feed answers without device work, in order
  bool enc = false;           // the batched path runs under IO encryption: every window is a keyed stream's
  std::vector<int64_t> iv_at; // ... where every entry's slice of the call's IVs starts
  int64_t tiles = 0;          // ... the grid of the encrypt pass
  const uint8_t* call_ivs = nullptr;  // ... the call's IVs (the IvScope's), before any entry's slice is set in iv_cur

  void single(s3s_cstream_feed_entry& e) {
    if (enc) {  // the entry's slice of the call's IVs
      ctx->iv_cur = call_ivs + 16 * (size_t)iv_at[(size_t)(&e - E)];
      ctx->iv_cur_n = s3s_cs::iv_slice_len(e.n_ends);
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

inline int64_t unit_items(int codec, const s3s_cs::Unit& u) { return codec == S3S_CODEC_SNAPPY ? u.first + snappy_chunk_items(u.len) : 1; }
inline int64_t unit_slots(int codec, const s3s_cs::Unit& u) { return codec == S3S_CODEC_SNAPPY ? snappy_chunk_slots(u.len) : u.len > 0; }

// worst-case checksum segments of a window's pieces, as the single feed sizes them; seg_start (or null): n_ends + 2 entries
int64_t window_segs(int codec, int64_t bs, int64_t src_len, const int64_t* ends, int32_t n_ends, int32_t* seg_start, bool enc) {
  int64_t segs = 0;
  for (int32_t j = 0; j <= n_ends; j++) {
    const int64_t a = j == 0 ? 0 : ends[j - 1], b = j < n_ends ? ends[j] : src_len;
    if (seg_start) seg_start[j] = (int32_t)segs;
    segs += worst_segs(max_partition_size(codec, bs, b - a) + kLz4FrameHeader + kSnappyStreamHeader + (enc ? 16 : 0));
    if (segs > s3s_cs::kBatchMax) return -1;
  }
  if (seg_start) seg_start[n_ends + 1] = (int32_t)segs;
  return segs;
}

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

// one by one, in order.  Encrypted streams: the call's IVs are sliced in entry order, n_ends + 1 an entry
int cs_one_by_one(CsBatch& b, bool any_enc) {
  s3s_ctx* ctx = b.ctx;
  if (any_enc && enc_on(ctx)) {  // (with the layer off every encrypted stream is stale: the single feed's refusal)
    int64_t want = 0;
    for (int32_t i = 0; i < b.n; i++) want += (int64_t)(b.E[i].n_ends > 0 ? b.E[i].n_ends : 0) + 1;
    if (ctx->iv_cur_n != want)
      return fail(ctx, S3S_E_INVALID, "the entries of the batch have %lld pieces (n_ends + 1 each), s3s_set_stream_ivs gave %lld IVs",
                  (long long)want, (long long)ctx->iv_cur_n);
    const uint8_t* ivs = ctx->iv_cur;
    for (int32_t i = 0; i < b.n; i++) {
      const int64_t mine = (int64_t)(b.E[i].n_ends > 0 ? b.E[i].n_ends : 0) + 1;
      ctx->iv_cur = ivs;
      ctx->iv_cur_n = mine;
      ivs += 16 * (size_t)mine;
      b.single(b.E[i]);
    }
    return S3S_OK;
  }
  for (int32_t i = 0; i < b.n; i++) b.single(b.E[i]);
  return S3S_OK;
}

// Which entries are windows of the batch: those whose single feed would launch something.  An entry the single feed refuses
// by its arguments, and one whose window launches nothing, keep that feed's answer (b.host).  false: the call does not fit one
// plan (an index would leave int32): it goes one by one
bool cs_batch_windows(CsBatch& b, s3s_cs::Totals* tot) {
  const s3s_cstream* s0 = b.E[0].stream;
  const int codec = s0->codec;
  const int64_t bs = s0->bs;
  const bool do_sum = s0->algo != S3S_CHECKSUM_NONE;
  const bool enc = b.enc;
  s3s_cs::IvSlicer slices;
  for (int32_t i = 0; i < b.n; i++) {
    const s3s_cstream_feed_entry& e = b.E[i];
    const s3s_cstream* s = e.stream;
    if (enc) b.iv_at.push_back(slices.take(e.n_ends));
    if (enc && (!s->enc || s->epoch != b.ctx->enc_epoch)) {  // (the single feed's S3S_E_UNSUPPORTED / S3S_E_INVALID)
      b.host.push_back(i);
      continue;
    }
    const bool null_with_length = (e.src_len > 0 && !e.d_src) || (e.dst_capacity > 0 && !e.d_dst) ||
                                  (e.n_ends > 0 && (!e.part_ends || !e.out_lengths || (do_sum && !e.out_checksums)));
    const bool refused = s3s_cs::window_refused(e.src_len, e.part_ends, e.n_ends, e.dst_capacity, null_with_length);
    int64_t n_items = 0, n_slots = 0;
    if (!refused)
      s3s_cs::plan_units(codec, bs, s->st.open_bytes, e.src_len, e.part_ends, e.n_ends, [&](const s3s_cs::Unit& u) {
        n_items += s3s_cs::iv_records(u, enc) + unit_items(codec, u);
        n_slots += unit_slots(codec, u);
      });
    if (refused || n_items == 0 || n_items > s3s_cs::kBatchMax) {  // (too many blocks: the single feed's S3S_E_UNSUPPORTED)
      b.host.push_back(i);
      continue;
    }
    const int64_t segs = do_sum ? window_segs(codec, bs, e.src_len, e.part_ends, e.n_ends, nullptr, enc) : 0;
    if (segs < 0) {  // (window too large for one feed: the single feed's answer)
      b.host.push_back(i);
      continue;
    }
    if (!s3s_cs::fits_call(*tot, n_items, n_slots, e.n_ends, segs)) return false;
    CsWin w;
    w.e = i;
    w.c = s3s_cs::reserve(tot, n_items, n_slots, e.n_ends, segs, e.dst_capacity, s->st.open_img);
    if (enc) {
      w.tiles = s3s_cs::pass_tiles(e.dst_capacity, s3s_cs::feed_bound_encrypted(codec, bs, e.src_len, e.n_ends), s->st.open_img);
      if (b.tiles + w.tiles > s3s_cs::kBatchMax) return false;
      b.tiles += w.tiles;
    }
    b.W.push_back(w);
  }
  return true;
}

int cs_batch_run(CsBatch& b, const s3s_cs::Totals& tot) {
  s3s_ctx* ctx = b.ctx;
  const s3s_cstream* s0 = b.E[0].stream;
  const int codec = s0->codec, algo = s0->algo;
  const int64_t bs = s0->bs;
  const bool do_sum = algo != S3S_CHECKSUM_NONE;
  const int32_t m = tot.m, N = (int32_t)tot.items;
  const size_t PP = (size_t)tot.pp(), P = (size_t)tot.pieces;
  const bool enc = b.enc;
  s3s_cs::Arena A;
  if (enc) A.lay_out_encrypted(tot, sizeof(Item), sizeof(TaskTail), sizeof(s3s_cs::PassWindow), b.tiles);
  else A.lay_out(tot, sizeof(Item), sizeof(TaskTail));
  const int64_t slot_stride = codec == S3S_CODEC_SNAPPY ? snappy_slot_stride(bs) : codec_slot_stride(codec, bs);
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
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  uint8_t* da = dev<uint8_t>(ctx, B_PLAN);
  Item* h_items = reinterpret_cast<Item*>(hs + A.items);
  s3s_cs::Mark* h_marks = reinterpret_cast<s3s_cs::Mark*>(hs + A.marks);
  int32_t* h_pf = reinterpret_cast<int32_t*>(hs + A.pf);
  int32_t* h_seg = reinterpret_cast<int32_t*>(hs + A.seg);
  int64_t* h_seed = reinterpret_cast<int64_t*>(hs + A.seed);
  int32_t* h_pw = reinterpret_cast<int32_t*>(hs + A.pw);
  TaskTail* h_tails = reinterpret_cast<TaskTail*>(hs + A.tails);
  s3s_cs::CutEntry* h_cuts = reinterpret_cast<s3s_cs::CutEntry*>(hs + A.cuts);
  uint8_t* h_ivs = hs + A.ivs;  // under IO encryption: the IVs, the pass descriptors and the tile -> window map
  s3s_cs::PassWindow* h_wins = reinterpret_cast<s3s_cs::PassWindow*>(hs + A.wins);
  int32_t* h_tile_win = reinterpret_cast<int32_t*>(hs + A.tile_win);
  int32_t tile0 = 0;

  const uint8_t* base = b.E[b.W[0].e].d_src;  // the one source pointer of the codec launch: every item is an offset from it
  const int level = codec == S3S_CODEC_LZ4 ? lz4_level(bs) : 0;
  memset(hs + A.seg, 0, A.seed - A.seg);
  for (int32_t wi = 0; wi < m; wi++) {
    CsWin& w = b.W[(size_t)wi];
    const s3s_cstream_feed_entry& e = b.E[w.e];
    const s3s_cstream* s = e.stream;
    const int64_t delta = s3s_cs::item_src_off((int64_t)reinterpret_cast<intptr_t>(e.d_src), (int64_t)reinterpret_cast<intptr_t>(base), 0);
    const bool ok = s3s_cs::plan_entry_records(
        &w.c, codec, bs, s->st.open_bytes, e.src_len, e.part_ends, e.n_ends, h_marks, h_pf, enc,
        [&](const s3s_cs::Unit& u) { return unit_items(codec, u); },
        [&](const s3s_cs::Unit& u, int32_t at) { h_items[at] = Item{0, 0, kItemIv, -1, u.piece}; },  // the hole the encrypt pass fills
        [&](const s3s_cs::Unit& u, int32_t at, int32_t& slot) {
          int32_t it = at;
          if (codec == S3S_CODEC_SNAPPY) {
            if (u.first) h_items[it++] = Item{0, 0, kItemSnappyHeader, -1, u.piece};
            snappy_plan_chunk(h_items, it, slot, delta + u.src_off, u.len, u.piece);
          } else if (codec == S3S_CODEC_LZF) {
            h_items[it] = Item{delta + u.src_off, u.len, kItemLzfChunk, slot++, u.piece};
          } else if (u.len > 0) {
            h_items[it] = Item{delta + u.src_off, u.len, lz4_chunk_kind(u.len) | (level << 8), slot++, u.piece};
          } else {
            h_items[it] = Item{0, 0, kItemLz4End | (level << 8), -1, u.piece};
          }
        });
    if (!ok) return fail(ctx, S3S_E_HIP, "the plan of entry %d does not match its count", w.e);
    if (do_sum) window_segs(codec, bs, e.src_len, e.part_ends, e.n_ends, h_seg + w.c.first_pp, enc);
    s3s_cs::seed_pieces(w.c, wi, s->carry, fresh(algo), h_seed, h_pw);
    h_cuts[wi] = w.c;
    if (enc) s3s_cs::window_ivs(w.c, b.call_ivs, b.iv_at[(size_t)w.e], s->iv, h_ivs);
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
  if (codec == S3S_CODEC_LZ4) {
    ctx->lz4_variant_used = s0->lz4_variant;
    launch_lz4_compress(base, d_items, N, dev<uint32_t>(ctx, B_ITEM_CHECK), dev<uint8_t>(ctx, B_SLOTS), (int32_t)slot_stride,
                        dev<uint32_t>(ctx, B_ITEM_SIZE), dev<uint32_t>(ctx, B_WORK), (s0->lz4_variant == 11 ? 8 : 10) * ctx->cu_count,
                        s0->lz4_variant, ctx->stream, nullptr, bs >= kLz4U32From);
  } else if (codec == S3S_CODEC_LZF) {
    launch_lzf_compress(base, d_items, N, dev<uint8_t>(ctx, B_SLOTS), slot_stride, dev<uint32_t>(ctx, B_ITEM_SIZE), ctx->stream);
  } else {
    launch_snappy_compress(base, d_items, N, dev<uint8_t>(ctx, B_SLOTS), slot_stride, dev<uint32_t>(ctx, B_ITEM_SIZE), s0->snappy_variant,
                           ctx->stream);
  }
  HIP_TRY(ctx, hipGetLastError());
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
  const int32_t* h_status = reinterpret_cast<const int32_t*>(hs + A.status);
  const int64_t* h_res = reinterpret_cast<const int64_t*>(hs + A.res);
  std::vector<s3s_cs::Cut> cuts((size_t)m);
  for (int32_t wi = 0; wi < m; wi++) {
    const CsWin& w = b.W[(size_t)wi];
    const s3s_cstream_feed_entry& e = b.E[w.e];
    if (!s3s_cs::cut_from_words(h_res + (size_t)s3s_cs::kCutWords * (size_t)wi, h_status[wi], w.c.n_items, e.src_len, e.dst_capacity, e.n_ends,
                                &cuts[(size_t)wi]))
      return fail(ctx, S3S_E_HIP, "the capacity cut of entry %d returned an impossible result", w.e);
  }
  for (int32_t wi = 0; wi < m; wi++) {
    const CsWin& w = b.W[(size_t)wi];
    s3s_cstream_feed_entry& e = b.E[w.e];
    s3s_cstream* s = e.stream;
    const s3s_cs::Cut& c = cuts[(size_t)wi];
    memset(&e.result, 0, sizeof e.result);
    if (c.need_dst > 0) {  // the window's first unit does not fit its dst: nothing is taken, the stream stays usable
      e.result.need_dst = c.need_dst;
      e.status = fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld image bytes of the next unit", (long long)e.dst_capacity, (long long)c.need_dst);
      continue;
    }
    s3s_cs::commit(&s->st, &s->carry, c, e.part_ends, reinterpret_cast<const int64_t*>(hs + A.piece) + w.c.first_pp,
                   reinterpret_cast<const int64_t*>(hs + A.len) + w.c.first_len,
                   do_sum ? reinterpret_cast<const int64_t*>(hs + A.sums) + w.c.first_piece : nullptr, e.out_lengths, e.out_checksums);
    if (enc) s3s_cs::commit_iv(s->iv, s->st, w.c.open_img, c.parts_closed, h_ivs + 16 * (size_t)w.c.first_piece);
    e.result.consumed = c.consumed;
    e.result.out_len = c.out_len;
    e.result.parts_closed = c.parts_closed;
    e.status = S3S_OK;
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
  if (n < 0 || (n > 0 && !E)) return fail(ctx, S3S_E_INVALID, "null entry array or negative count");
  BatchVerdict<s3s_cstream_feed_entry> verdict(E, n);
  if (n == 0) return verdict.finish(S3S_OK);
  CsBatch b = {ctx, E, n, {}, {}};
  bool batched, any_enc;
  int rc;
  if ((rc = cs_batch_check(b, &batched, &any_enc))) return rc;
  s3s_cs::Totals tot;
  if (batched && enc_on(ctx) && !any_enc) batched = false;  // only plain streams on a keyed context: each one's S3S_E_UNSUPPORTED
  if (batched && enc_on(ctx)) {  // ONE array of IVs for the call, sliced in entry order: any other count before anything runs
    int64_t want = 0;
    for (int32_t i = 0; i < n; i++) want += s3s_cs::iv_slice_len(E[i].n_ends);
    if (ctx->iv_cur_n != want)
      return fail(ctx, S3S_E_INVALID, "the entries of the batch have %lld pieces (n_ends + 1 each), s3s_set_stream_ivs gave %lld IVs",
                  (long long)want, (long long)ctx->iv_cur_n);
    b.enc = true;
    b.call_ivs = ctx->iv_cur;
    b.iv_at.reserve((size_t)n);
  }
  if (batched && !cs_batch_windows(b, &tot)) {
    batched = false;
    b.W.clear();
    b.host.clear();
    b.iv_at.clear();
    b.enc = false;
  }
  if (!batched) {  // nothing to batch: one by one, in order
    if ((rc = cs_one_by_one(b, any_enc))) return rc;
    return verdict.finish(b.first_error());
  }
  if (tot.m > 0 && (rc = cs_batch_run(b, tot))) return rc;
  for (int32_t i : b.host) b.single(E[i]);  // (no device work: an argument the single feed refuses, a window that launches nothing)
  (b.enc ? ctx->cstream_batch_enc_entries : ctx->cstream_batch_entries) = tot.m;
  return verdict.finish(b.first_error());
}

int s3s_cstream_feed_batch(s3s_ctx* ctx, s3s_cstream_feed_entry* E, int32_t n) {
  if (!ctx) return S3S_E_INVALID;
  ctx->err[0] = 0;
  ctx->cstream_batch_entries = 0;
  ctx->cstream_batch_enc_entries = 0;
  if (n < 0 || (n > 0 && !E)) return fail(ctx, S3S_E_INVALID, "null entry array or negative count");
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
