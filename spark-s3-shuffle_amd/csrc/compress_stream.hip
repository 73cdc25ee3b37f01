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
#include <new>
#include <optional>

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
  for (int32_t j = 0; j < c.parts_closed; j++) {
    out_lengths[j] = j == 0 ? s->st.open_img : 0;
    if (out_checksums) out_checksums[j] = j == 0 ? s->carry : fresh(s->algo);
  }
  if (c.parts_closed > 0) {
    s->carry = fresh(s->algo);
    s->st.open_bytes = s->st.open_img = 0;
    wipe(s->iv, sizeof s->iv);
  }
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
    c.k = h_res[s3s_cs::kCutK];
    c.consumed = h_res[s3s_cs::kCutConsumed];
    c.out_len = h_res[s3s_cs::kCutOutLen];
    c.need_dst = h_res[s3s_cs::kCutNeedDst];
    c.parts_closed = (int32_t)h_res[s3s_cs::kCutPartsClosed];
    piece_off = h_piece;
    if (*h_status != 0 || c.k < 0 || c.k > n_items || c.consumed < 0 || c.consumed > src_len || c.out_len < 0 || c.out_len > dst_capacity ||
        c.parts_closed < 0 || c.parts_closed > n_ends || c.need_dst < 0)
      return fail(ctx, S3S_E_HIP, "the capacity cut returned an impossible result");
    if (c.need_dst > 0) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
      r->need_dst = c.need_dst;
      return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld image bytes of the next unit", (long long)dst_capacity, (long long)c.need_dst);
    }
    if (c.parts_closed > 0) memcpy(out_lengths, h_len, 8 * (size_t)c.parts_closed);
  } else {
    s3s_cs::closed_lengths(s->st, c, piece_off, out_lengths);
  }
  if (do_sum) {
    if (c.parts_closed > 0) memcpy(out_checksums, h_sums, 8 * (size_t)c.parts_closed);
    s->carry = h_sums[c.parts_closed];
  }
  s3s_cs::advance(&s->st, c, part_ends, piece_off);
  if (enc) {  // the open partition's IV stays with the stream from the feed that took its first block until it closes
    if (s->st.open_img == 0) wipe(s->iv, sizeof s->iv);
    else if (c.parts_closed > 0 || front == 0) memcpy(s->iv, h_ivs + 16 * (size_t)c.parts_closed, 16);
  }
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
