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
#include <new>

#include "s3s_ctx.h"

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
};

namespace {

inline int64_t fresh(int algo) { return algo == S3S_CHECKSUM_ADLER32 ? 1 : 0; }  // getValue() of a new Adler32 / CRC32 / CRC32C

inline bool at_end(const s3s_dstream* s) { return s->pos == s->off[(size_t)s->nparts] && s->cur == s->nparts; }

// the smallest window that can hold a unit's header when the window shows nothing of it
inline int64_t min_unit(const s3s_dstream* s) {
  switch (s->codec) {
    case S3S_CODEC_LZ4: return kLz4FrameHeader;
    case S3S_CODEC_SNAPPY: return s->pos == s->off[(size_t)(s->cur < s->nparts ? s->cur : s->nparts)] ? kSnappyStreamHeader : 4;
    case S3S_CODEC_LZF: return 5;
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

}  // namespace

extern "C" {

int s3s_dstream_open(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                     int32_t nparts, s3s_dstream** out) {
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
  if (codec == S3S_CODEC_ZSTD)  // a frame is a whole partition with history across its blocks: no unit to stop at
    return fail(ctx, S3S_E_UNSUPPORTED, "Zstandard ranges cannot be streamed (use s3s_decompress_range*)");
  if (enc_on(ctx))  // the key stream would have to be sought to the middle of a partition
    return fail(ctx, S3S_E_UNSUPPORTED, "ranges under IO encryption cannot be streamed (use s3s_decompress_range*)");
  s3s_dstream* s = new (std::nothrow) s3s_dstream();
  if (!s) return fail(ctx, S3S_E_NOMEM, "out of host memory");
  s->ctx = ctx;
  s->codec = codec;
  s->algo = checksum_algo;
  s->nparts = nparts;
  s->off.assign(part_offsets, part_offsets + nparts + 1);
  if (checksum_algo != S3S_CHECKSUM_NONE && nparts > 0) s->ref.assign(ref_checksums, ref_checksums + nparts);
  s->carry = fresh(checksum_algo);
  *out = s;
  return S3S_OK;
}

int64_t s3s_dstream_position(const s3s_dstream* s) { return s ? s->pos : (int64_t)S3S_E_INVALID; }

int s3s_dstream_close(s3s_dstream* s) {
  if (!s) return S3S_E_INVALID;
  const int rc = s->err != S3S_OK ? s->err : at_end(s) ? S3S_OK : S3S_E_BAD_FRAME;
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
  if (enc_on(ctx)) return fail(ctx, S3S_E_UNSUPPORTED, "IO encryption was switched on after the stream was opened");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& v : ctx->stage_ms) v = 0;
  const bool do_sum = s->algo != S3S_CHECKSUM_NONE;
  const int codec = s->codec;

  // bytes this feed looks at: S3S_CODEC_NONE's units are bytes, so its cut is known before anything runs
  int64_t L = comp_len;
  if (codec == S3S_CODEC_NONE && dst_capacity < L) L = dst_capacity;
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
               o_sums = al(o_seed + 8 * n1), o_misc = al(o_sums + 8 * n1), stage_total = o_misc + 64;
  int rc;
  if ((rc = ensure_stage(ctx, stage_total))) return rc;
  uint8_t* hs = static_cast<uint8_t*>(ctx->h_stage);
  int64_t* h_off = reinterpret_cast<int64_t*>(hs);
  int64_t* h_off2 = reinterpret_cast<int64_t*>(hs + o_off2);
  int32_t* h_seg = reinterpret_cast<int32_t*>(hs + o_seg);
  int32_t* h_seg2 = reinterpret_cast<int32_t*>(hs + o_seg2);
  int64_t* h_seed = reinterpret_cast<int64_t*>(hs + o_seed);
  int64_t* h_sums = reinterpret_cast<int64_t*>(hs + o_sums);  // [n] = the second launch's sum
  int64_t* h_misc = reinterpret_cast<int64_t*>(hs + o_misc);  // [0] n_frames, [1] status, [2..5] stop, need / k, consumed, out_len, need
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
  // device: B_OFFSETS [piece offsets n + 1][2], B_REF_SUMS [seeds n + 1], B_SUMS [n + 1], B_STATUS [status][pad][result 4 x int64]
  if ((rc = ensure(ctx, B_OFFSETS, 8 * (n1 + 2)))) return rc;
  if ((rc = ensure(ctx, B_REF_SUMS, 8 * n1))) return rc;
  if ((rc = ensure(ctx, B_SUMS, 8 * n1))) return rc;
  if ((rc = ensure(ctx, B_STATUS, 64))) return rc;
  int64_t* d_off = dev<int64_t>(ctx, B_OFFSETS);
  int32_t* d_status = dev<int32_t>(ctx, B_STATUS);
  int64_t* d_result = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_STATUS) + 16);
  HIP_TRY(ctx, hipMemsetAsync(ctx->buf[B_STATUS].p, 0, 64, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_off, h_off, 8 * n1, hipMemcpyHostToDevice, ctx->stream));
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
    return bad >= 0 ? stick(s, r, S3S_E_CHECKSUM, bad, "") : fail(ctx, S3S_E_UNSUPPORTED, "codec block larger than the decoder takes");
  };

  // ---- discovery: the whole units of the window, then the cut at dst_capacity -----------------------------------------------
  int64_t n_frames = 0, k = 0, consumed = L, out_len = L, need_comp = 0;
  if (codec == S3S_CODEC_NONE) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else {
    const int cf = codec == S3S_CODEC_LZF ? kChunkLzf : kChunkSnappy;
    const int32_t n_tiles = codec == S3S_CODEC_LZ4 ? lz4_tile_count(L) : 0;
    int64_t *d_true_entry = nullptr, *d_base = nullptr;
    if (codec == S3S_CODEC_LZ4) {
      const size_t tile_i64 = sizeof(int64_t) * (size_t)(n_tiles + 1);
      if ((rc = ensure(ctx, B_PART_NFRAMES, 4 * tile_i64 + sizeof(int32_t) * (size_t)(n_tiles + 1)))) return rc;
      int64_t* d_spec_entry = dev<int64_t>(ctx, B_PART_NFRAMES);
      int64_t* d_spec_exit = d_spec_entry + (n_tiles + 1);
      d_true_entry = d_spec_exit + (n_tiles + 1);
      d_base = d_true_entry + (n_tiles + 1);
      int32_t* d_spec_count = reinterpret_cast<int32_t*>(d_base + (n_tiles + 1));
      launch_lz4_discover_stream(d_comp, L, left, n_tiles, d_spec_entry, d_spec_exit, d_spec_count, d_true_entry, d_base, d_status,
                                 d_result, ctx->stream);
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[0], d_base + n_tiles, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    } else {
      const size_t cnt_bytes = al(sizeof(uint32_t) * n1);
      if ((rc = ensure(ctx, B_PART_NFRAMES, cnt_bytes + sizeof(int64_t) * (n1 + 1)))) return rc;
      uint32_t* d_cnt = dev<uint32_t>(ctx, B_PART_NFRAMES);
      d_base = reinterpret_cast<int64_t*>(dev<uint8_t>(ctx, B_PART_NFRAMES) + cnt_bytes);
      launch_snappy_count_frames_stream(d_comp, d_off, n, s->pos > s->off[(size_t)s->cur], last_pend, d_cnt, d_status, d_result,
                                        ctx->stream, cf);
      launch_scan_u32(d_cnt, n, d_base, ctx->stream);
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[0], d_base + n, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
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
    if (stop < 0 || stop > L || (stop < L && need_comp <= L - stop)) return fail(ctx, S3S_E_HIP, "frame discovery returned an impossible stop offset");
    if (n_frames > 0x7fffff00ll) return fail(ctx, S3S_E_UNSUPPORTED, "too many frames in one feed");
    k = 0;
    consumed = stop;
    out_len = 0;
    if (n_frames > 0) {
      if ((rc = ensure(ctx, B_FRAMES, sizeof(Frame) * (size_t)(n_frames + 1)))) return rc;
      if ((rc = ensure(ctx, B_ITEM_SIZE, sizeof(uint32_t) * (size_t)(n_frames + 1)))) return rc;
      if ((rc = ensure(ctx, B_FRAME_OUT, sizeof(int64_t) * (size_t)(n_frames + 1)))) return rc;
      if (codec == S3S_CODEC_LZ4) {  // the one-shot emit, with the stop offset as the end of the bytes: the chain ends exactly there
        launch_lz4_emit_frames(d_comp, stop, lz4_tile_count(stop), d_true_entry, d_base, dev<Frame>(ctx, B_FRAMES),
                               dev<uint32_t>(ctx, B_ITEM_SIZE), n_frames, dev<int64_t>(ctx, B_FRAME_OUT), d_status, ctx->stream);
      } else {
        launch_snappy_emit_frames_stream(d_comp, d_off, n, s->pos > s->off[(size_t)s->cur], last_pend, d_base, dev<Frame>(ctx, B_FRAMES),
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
      if (consumed == 0) {  // the first unit does not fit dst: nothing is taken, the stream stays usable
        r->need_dst = h_misc[5];
        return fail(ctx, S3S_E_CAPACITY, "dst_capacity %lld < %lld decoded bytes of the next unit", (long long)dst_capacity, (long long)h_misc[5]);
      }
    }
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
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, d_comp, (size_t)consumed, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  } else if (k > 0 || second) {
    if (k > 0) {
      if (codec == S3S_CODEC_LZ4)
        launch_lz4_decompress(d_comp, dev<Frame>(ctx, B_FRAMES), (int32_t)k, dev<int64_t>(ctx, B_FRAME_OUT), d_dst, d_status,
                              ctx->lz4_decode_variant, ctx->stream);
      else
        launch_snappy_decompress(d_comp, dev<Frame>(ctx, B_FRAMES), (int32_t)k, dev<int64_t>(ctx, B_FRAME_OUT), d_dst, d_status,
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
      launch_lz4_decompress(d_comp, dev<Frame>(ctx, B_FRAMES), (int32_t)k, dev<int64_t>(ctx, B_FRAME_OUT), d_dst, d_status, 3, ctx->stream);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&h_misc[1], d_status, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      st = *reinterpret_cast<int32_t*>(&h_misc[1]);
    }
    if (st == S3S_E_UNSUPPORTED) return fail(ctx, S3S_E_UNSUPPORTED, "codec block larger than the decoder takes");
    if (st != 0) return corrupt("frame payload");  // (the capacity cut may have left a partition's end, which the window holds, unconsumed)
    if (second) carry = h_sums[n];
  }

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
