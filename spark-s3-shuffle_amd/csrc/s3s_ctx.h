// s3s_ctx.h — the context object behind the C-ABI and the helpers both API translation units
// (codec_api.hip: map side, decode_api.hip: reduce side) share.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "s3s_internal.h"
#include "stream_placement.h"

namespace s3s {

inline thread_local char g_create_error[512] = "";

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

enum BufId {
  B_ITEMS, B_PART_FIRST, B_SLOTS, B_ITEM_SIZE, B_ITEM_OFF, B_INDEX, B_SUMS, B_SEG_START,
  B_PARTIAL, B_STATUS, B_TABLES, B_SRC, B_DST, B_OFFSETS, B_FRAMES, B_PART_NFRAMES,
  B_FRAME_OUT, B_REF_SUMS, B_ITEM_CHECK, B_RANGES, B_TILE_RANGE,
  B_HB_IN0, B_HB_IN1, B_HB_OUT0, B_HB_OUT1,  // host-buffer batch pipeline (host_batch.hip): double-buffered device staging
  B_WORK,  // block counter of the persistent codec grid
  B_PARTIAL2,  // checksum partials of folded segment groups (ranges of more than kChecksumFoldFrom segments)
  B_ZSCRATCH, B_ZPIECES,  // zstd single pass: decoded partitions at guessed capacities, and the compaction's piece list
  B_ZENC,  // zstd map side: sequences + literals of the blocks in flight, one piece per resident workgroup
  B_TAILS,  // batched calls: one TaskTail per map task / fetched range (s3s_internal.h)
  B_IVS,        // IO encryption, map side: one IV per partition of the call
  B_CRYPT,      // IO encryption, reduce side: the fetched range decrypted, IVs dropped
  B_CRYPT_OFF,  // IO encryption: stored / plain partition offsets of the AES-CTR pass where they are not B_INDEX
  B_ZBLOCKS, B_ZBLOCK_LIT,  // zstd block path (zstd_decode_blocks.hip): control word + frame and block tables; literal buffers of its grid
  B_ZSTAGED, B_ZSTAGED_POOL,  // zstd staged path (zstd_decode_staged.hip): control word + frame and block tables; literal and sequence-record staging
  B_PLAN,  // batched map side: the call's small arrays in one arena, one upload and one download (PackedPlan, stream_placement.h)
  B_COUNT
};

}  // namespace s3s

struct s3s_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int stream_slot = -1;   // this context's slot in its device's registry (codec_api.hip), returned in s3s_destroy
  int stream_class = 1;   // S3S_OPT_STREAM_CLASS: the queue pool the slot put the stream in (stream_placement.h)
  char err[512] = "";
  int64_t lz4_block = 32768;
  int64_t snappy_block = 32768;
  int profile = 0;
  int lz4_variant = 11;  // 11 = exact windows with the input ring (default); 10 = exact windows; 1 = general batch; 9 = auto: the context times 1 and 10 on its own one-task calls (batched calls run 11)
  // auto-tuning state (S3S_OPT_LZ4_VARIANT = 9): index 0 = variant 1 (general batch), 1 = variant 10
  // (exact windows).  Shuffle data of one stage has one schema, so the faster parse for a
  // context's first map outputs stays the faster one; every 32nd large call re-measures the other.
  int auto_choice = 1;
  int auto_samples[2] = {0, 0};
  int auto_tick = 0;
  double auto_ms_per_mib[2] = {0, 0};
  int lz4_variant_used = 0;  // the parse the last LZ4 compress call ran (S3S_OPT_LZ4_VARIANT_USED)
  hipEvent_t ev_auto[2] = {nullptr, nullptr};
  int lz4_decode_variant = 4;  // 4 = batch decoder (lz4_decode_batch.hip), 3 = ring decoder on the vector ALU
  int snappy_variant = 1;
  int zstd_compress = 0;  // S3S_OPT_ZSTD_COMPRESS: the compress entry points take S3S_CODEC_ZSTD (off: S3S_E_UNSUPPORTED, as before ABI 11)
  int lzf_compress = 0;   // S3S_OPT_LZF_COMPRESS: the same switch for S3S_CODEC_LZF
  int zstd_decode_variant = 1;  // S3S_OPT_ZSTD_DECODE_VARIANT: 1 = block-independent frames one workgroup per block, 0 = one frame per wavefront only
  int zstd_decode_blocks = 0;   // S3S_OPT_ZSTD_DECODE_BLOCKS: blocks of the last Zstandard decode call whose frames completed on the block path
  int zstd_decode_staged = 0;         // S3S_OPT_ZSTD_DECODE_STAGED: 1 = frames with history decode in stages (entropy per block, copies per frame)
  int zstd_decode_staged_blocks = 0;  // S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS: blocks of the last Zstandard decode call whose frames completed on the staged path
  int dstream_batch_entries = 0;      // S3S_OPT_DSTREAM_BATCH_ENTRIES: entries of the last s3s_dstream_feed_batch* call that the batched path answered
  int cstream_batch_entries = 0;      // S3S_OPT_CSTREAM_BATCH_ENTRIES: the same for the last s3s_cstream_feed_batch* call (plain windows only)
  int cstream_batch_enc_entries = 0;  // S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES: ... the entries it answered under IO encryption
  s3s::DevBuf buf[s3s::B_COUNT];
  int cu_count = 256;  // compute units of the device (persistent grids: resident wavefronts per CU x this)
  void* h_stage = nullptr;  // pinned
  size_t h_stage_cap = 0;
  hipEvent_t ev[S3S_STAGE_COUNT + 1] = {};
  hipEvent_t ev_hash = nullptr;  // between the xxHash32 pre-pass and the LZ4 compress kernel
  // host-buffer map side: the upload of the source runs in chunks on its own stream, the codec kernels of a chunk's
  // blocks start as soon as the chunk has landed (s3s_compress_map_output sets up_host for the duration of the call)
  hipStream_t copy_stream = nullptr;
  std::vector<hipEvent_t> ev_up;
  const uint8_t* up_host = nullptr;  // host source of d_src[0, total_u), or nullptr (source already on the device)
  // host-buffer batch entry points (host_batch.hip): one DMA stream per PCIe direction next to the compute stream
  hipStream_t hb_in = nullptr, hb_out = nullptr;
  bool hb_shared = false;  // hb_in / hb_out are the device's shared copy lanes (host_batch.hip: copy arbiter), not this context's to destroy
  hipEvent_t hb_ev_in[2] = {nullptr, nullptr}, hb_ev_out[2] = {nullptr, nullptr};
  double stage_ms[S3S_STAGE_COUNT] = {};
  // Spark IO encryption (s3s_set_io_encryption): on while enc_rounds != 0.  The round keys live here on the host and travel
  // to the AES-CTR kernel as arguments; they are wiped when the layer is switched off and in s3s_destroy
  s3s::AesKeys enc_keys = {};
  int enc_rounds = 0, enc_key_bits = 0;
  uint64_t enc_epoch = 0;           // counts the s3s_set_io_encryption calls that took effect: an encrypted s3s_dstream is bound to the one it was opened under
  bool enc_suspended = false;       // reduce side: the wrapped call on the decrypted bytes runs with the layer off
  std::vector<uint8_t> ivs;         // s3s_set_stream_ivs: the IVs of the NEXT compress call (consumed by it, success or not)
  bool ivs_set = false;
  const uint8_t* iv_cur = nullptr;  // the IVs of the compress call (or task of a batch) in progress, iv_cur_n of them (-1: none given)
  int64_t iv_cur_n = -1;
  int iv_depth = 0;                 // entry points call each other: the outermost one owns the IVs
};

namespace s3s {

inline int fail(s3s_ctx* ctx, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (ctx) vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
  else vsnprintf(g_create_error, sizeof g_create_error, fmt, ap);
  va_end(ap);
  return code;
}

// Batch entry points stamp every entry S3S_STATUS_NOT_RUN on entry and create one of these: a return that is not the call's
// regular end (bad argument, HIP error between the groups, allocation failure) leaves NO entry reporting S3S_OK — an entry whose
// kernels ran may still be waiting for its download — so the caller applies the call's return code to exactly the NOT_RUN ones
// and keeps the verdict of every entry that has one (advisor r3: one task's error must not fail its neighbours).
template <typename T>
struct BatchVerdict {
  T* e;
  int32_t n;
  bool done = false;
  BatchVerdict(T* entries, int32_t count) : e(entries), n(count) {
    for (int32_t i = 0; i < n; i++) e[i].status = S3S_STATUS_NOT_RUN;
  }
  ~BatchVerdict() {
    if (done) return;
    for (int32_t i = 0; i < n; i++)
      if (e[i].status == S3S_OK) e[i].status = S3S_STATUS_NOT_RUN;
  }
  int finish(int rc) {
    done = true;
    return rc;
  }
};

inline bool enc_on(const s3s_ctx* ctx) { return ctx && ctx->enc_rounds != 0 && !ctx->enc_suspended; }

inline void wipe(void* p, size_t n) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) v[i] = 0;
}

// Every compress entry point creates one: the outermost takes the IVs that s3s_set_stream_ivs left (they are gone when it
// returns, whichever way), the nested ones see the slice their caller set in iv_cur / iv_cur_n.
struct IvScope {
  s3s_ctx* c;
  std::vector<uint8_t> own;
  explicit IvScope(s3s_ctx* ctx) : c(ctx) {
    if (c->iv_depth++ != 0) return;
    own.swap(c->ivs);
    c->iv_cur = own.data();
    c->iv_cur_n = c->ivs_set ? (int64_t)(own.size() / 16) : -1;
    c->ivs_set = false;
  }
  ~IvScope() {
    if (--c->iv_depth != 0) return;
    c->iv_cur = nullptr;
    c->iv_cur_n = -1;
  }
  IvScope(const IvScope&) = delete;
  IvScope& operator=(const IvScope&) = delete;
};

// with the layer on, a compress call needs exactly one IV per partition (a call without partitions needs none)
inline int enc_check_ivs(s3s_ctx* ctx, int64_t n_parts) {
  if (!enc_on(ctx) || ctx->iv_cur_n == n_parts || (n_parts == 0 && ctx->iv_cur_n < 0)) return S3S_OK;
  if (ctx->iv_cur_n < 0)
    return fail(ctx, S3S_E_INVALID, "IO encryption is on and no IVs were set for this call (s3s_set_stream_ivs: one per partition, %lld)",
                (long long)n_parts);
  return fail(ctx, S3S_E_INVALID, "IO encryption is on: the call has %lld partitions, s3s_set_stream_ivs gave %lld IVs",
              (long long)n_parts, (long long)ctx->iv_cur_n);
}

#define HIP_TRY(ctx, expr)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, S3S_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                      \
  } while (0)

inline int ensure(s3s_ctx* ctx, BufId id, size_t bytes) {
  DevBuf& b = ctx->buf[id];
  if (bytes <= b.cap) return S3S_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (b.p) HIP_TRY(ctx, hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  size_t want = bytes + bytes / 4 + 4096;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    want = bytes;
    e = hipMalloc(&b.p, want);
  }
  if (e != hipSuccess) return fail(ctx, S3S_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
  b.cap = want;
  return S3S_OK;
}

inline int ensure_stage(s3s_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->h_stage_cap) return S3S_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->h_stage) HIP_TRY(ctx, hipHostFree(ctx->h_stage));
  ctx->h_stage = nullptr;
  ctx->h_stage_cap = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  HIP_TRY(ctx, hipHostMalloc(&ctx->h_stage, want, hipHostMallocDefault));
  ctx->h_stage_cap = want;
  return S3S_OK;
}

template <typename T>
inline T* dev(s3s_ctx* ctx, BufId id) {
  return static_cast<T*>(ctx->buf[id].p);
}

inline int lz4_level(int64_t block_size) {
  int level = 0;
  while ((1ll << level) < block_size) level++;
  level -= 10;
  return level < 0 ? 0 : level;
}

// plan record kind of an LZ4 chunk: liblz4 picks its parse by the input's LENGTH (LZ4_64Klimit), not by the block size, so a
// partition's tail below kLz4U32From bytes is a byU16 chunk whatever the block size
inline int32_t lz4_chunk_kind(int32_t len) { return len >= kLz4U32From ? kItemLz4ChunkU32 : kItemLz4Chunk; }

inline int64_t snappy_max_len(int64_t n) { return 32 + n + n / 6; }

// ---- Snappy chunks and their plan records --------------------------------------------------------------------------
// A chunk of up to one 64 KiB fragment is ONE kItemSnappyChunk item (one wavefront, one slot).  A larger chunk is a
// kItemSnappyChunkHead item followed by one kItemSnappyFrag item per fragment: every fragment gets its own wavefront and
// slot, so a 1 MiB block is 16 independent parses instead of a chain of 16 on one wavefront.
inline int64_t snappy_chunk_items(int64_t len) { return len <= kSnappyFragment ? 1 : 1 + (len + kSnappyFragment - 1) / kSnappyFragment; }
inline int64_t snappy_chunk_slots(int64_t len) { return len <= kSnappyFragment ? 1 : (len + kSnappyFragment - 1) / kSnappyFragment; }
// items / slots of a segment of u bytes cut into chunks of bs (stream header item included)
inline void snappy_segment_counts(int64_t bs, int64_t u, int64_t* items, int64_t* slots) {
  const int64_t full = u / bs, rem = u % bs;
  *items += 1 + full * snappy_chunk_items(bs) + (rem ? snappy_chunk_items(rem) : 0);
  *slots += full * snappy_chunk_slots(bs) + (rem ? snappy_chunk_slots(rem) : 0);
}
// the items of one chunk [src_off, src_off + len) of partition `part`; `slot` counts the slots handed out
template <typename ItemT>
inline void snappy_plan_chunk(ItemT* items, int32_t& it, int32_t& slot, int64_t src_off, int32_t len, int32_t part) {
  if (len <= kSnappyFragment) {
    items[it++] = ItemT{src_off, len, kItemSnappyChunk, slot++, part};
    return;
  }
  items[it++] = ItemT{src_off, len, kItemSnappyChunkHead, -1, part};
  for (int32_t f = 0; f < len; f += kSnappyFragment) {
    const int32_t fl = len - f < kSnappyFragment ? len - f : kSnappyFragment;
    items[it++] = ItemT{src_off + f, fl, kItemSnappyFrag, slot++, part};
  }
}
// What ONE codec block [src_off, src_off + len) of partition `part` is in the plan of every compress call - the one-shot call,
// the task batch and the streaming feeds.  level: lz4_level(bs); last: the last block of its stream (Zstandard's kind bit)
template <typename ItemT>
inline void plan_codec_block(ItemT* items, int32_t& it, int32_t& slot, int codec, int level, int64_t src_off, int32_t len, int32_t part,
                             bool last) {
  if (codec == S3S_CODEC_SNAPPY) snappy_plan_chunk(items, it, slot, src_off, len, part);
  else if (codec == S3S_CODEC_ZSTD) items[it++] = ItemT{src_off, len, kItemZstdBlock | (last << 8), slot++, part};
  else if (codec == S3S_CODEC_LZF) items[it++] = ItemT{src_off, len, kItemLzfChunk, slot++, part};
  else items[it++] = ItemT{src_off, len, lz4_chunk_kind(len) | (level << 8), slot++, part};
}
// bytes between the slots of one Snappy call: a slot holds at most one fragment's output
inline int64_t snappy_slot_stride(int64_t bs) {
  const int64_t n = bs < kSnappyFragment ? bs : kSnappyFragment;
  return (int64_t)kSlotHeader + ((snappy_max_len(n) + 15) & ~int64_t(15));
}

// bytes between the slots of one call that is not Snappy's: LZ4 and Zstandard payloads never exceed the chunk (RAW fallback);
// an LZF block is written in full before the chunk is declared stored
inline int64_t codec_slot_stride(int codec, int64_t bs) {
  return (int64_t)kSlotHeader + (codec == S3S_CODEC_LZF ? (int64_t)kLzfSlotPayload : ((bs + 15) & ~int64_t(15)));
}
// ... of a compress call of any codec
inline int64_t compress_slot_stride(int codec, int64_t bs) {
  return codec == S3S_CODEC_SNAPPY ? snappy_slot_stride(bs) : codec_slot_stride(codec, bs);
}

inline int64_t effective_block(const s3s_ctx* ctx, int codec) {
  if (codec == S3S_CODEC_LZ4) return ctx ? ctx->lz4_block : 32768;
  if (codec == S3S_CODEC_SNAPPY) {
    const int64_t b = ctx ? ctx->snappy_block : 32768;
    return b < 1024 ? 1024 : b;  // snappy-java: Math.max(MIN_BLOCK_SIZE, blockSize)
  }
  if (codec == S3S_CODEC_ZSTD) return kZstdBlock;
  if (codec == S3S_CODEC_LZF) return kLzfChunk;
  return 0;
}

inline int64_t max_partition_size(int codec, int64_t bs, int64_t u) {
  if (u <= 0) return 0;
  switch (codec) {
    case S3S_CODEC_NONE:
      return u;
    case S3S_CODEC_LZ4: {
      const int64_t chunks = (u + bs - 1) / bs;
      return u + chunks * kLz4FrameHeader + kLz4FrameHeader;  // RAW fallback caps the payload
    }
    case S3S_CODEC_SNAPPY: {
      const int64_t full = u / bs, rem = u % bs;
      return kSnappyStreamHeader + full * (4 + snappy_max_len(bs)) + (rem ? 4 + snappy_max_len(rem) : 0);
    }
    case S3S_CODEC_ZSTD:  // frame header + every block Raw
      return kZstdFrameHeader + u + 3 * ((u + bs - 1) / bs);
    case S3S_CODEC_LZF:  // 7 bytes per chunk (the header of a compressed chunk; a stored one has 5)
      return u + 7 * ((u + bs - 1) / bs);
  }
  return -1;
}

inline void record(s3s_ctx* ctx, int slot) {
  if (ctx->profile) hipEventRecord(ctx->ev[slot], ctx->stream);
}

// worst-case 16 KiB checksum segments of a range that is at most `bytes` long
inline int32_t worst_segs(int64_t bytes) { return (int32_t)((bytes + kChecksumSegBytes - 1) / kChecksumSegBytes); }

inline int run_checksum(s3s_ctx* ctx, int algo, const uint8_t* d_data, const int64_t* d_offsets,
                 int32_t n, const int32_t* h_seg_start /* n+1, in pinned stage */,
                 int64_t* d_out, int64_t data_len) {
  const int32_t total = h_seg_start[n];
  int rc;
  if ((rc = ensure(ctx, B_SEG_START, sizeof(int32_t) * (size_t)(n + 1)))) return rc;
  if ((rc = ensure(ctx, B_PARTIAL, sizeof(uint32_t) * 4 * (size_t)(total > 0 ? total : 1)))) return rc;
  int32_t max_segs = 0;
  for (int32_t p = 0; p < n; p++) max_segs = h_seg_start[p + 1] - h_seg_start[p] > max_segs ? h_seg_start[p + 1] - h_seg_start[p] : max_segs;
  const int32_t groups = checksum_fold_groups(n, max_segs);
  if (groups > 0 && (rc = ensure(ctx, B_PARTIAL2, sizeof(uint32_t) * 4 * (size_t)n * (size_t)groups))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(dev<int32_t>(ctx, B_SEG_START), h_seg_start,
                              sizeof(int32_t) * (size_t)(n + 1), hipMemcpyHostToDevice, ctx->stream));
  launch_checksum_with_tables(algo, d_data, d_offsets, n, dev<int32_t>(ctx, B_SEG_START), total,
                              ctx->buf[B_TABLES].p, dev<uint32_t>(ctx, B_PARTIAL), d_out, data_len,
                              ctx->stream, max_segs, groups > 0 ? dev<uint32_t>(ctx, B_PARTIAL2) : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  return S3S_OK;
}

// Zstandard reduce side (zstd_decompress.hip): verify + decode (or only size) the frames of n_ranges device ranges
int zstd_decompress_ranges(s3s_ctx* ctx, int checksum_algo, s3s_fetch_range* R, int32_t n_ranges, bool size_only, bool* regular_end = nullptr);

}  // namespace s3s
