// s3s_internal.h — shared declarations of the MI355X shuffle-block codec library.
//
// Layout of the device workspace for one compress call (all in HBM, owned by s3s_ctx):
//   items[n_items]        16 B plan records (host-built, uploaded once per call)
//   part_first[N+1]       first item of every partition
//   slots[n_chunks]       one SLOT per codec chunk: frame header right-aligned in the first
//                         32 B, payload from +32 (16 B aligned)  -> written by the codec kernel
//   item_size[n_items]    bytes each item contributes to the .data image
//   item_off[n_items+1]   exclusive scan of item_size                 -> scan kernel
//   d_index[N+1], d_sums[N]                                           -> D2H at the end
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/s3shuffle_codec.h"

namespace s3s {

constexpr int kWave = 64;
constexpr int kMaxBlock = 32768;          // largest codec chunk the LDS-resident kernels take (Snappy; LZ4's default)
constexpr int kLz4MaxBlock = 65536;       // largest LZ4 block size S3S_OPT_LZ4_BLOCK_SIZE takes (round 4): liblz4 parses inputs below
                                          // 65 547 bytes with the SAME 8192 x u16 table (byU16) - positions just need all 16 bits - so
                                          // the window engine takes them as it is.  Larger blocks are S3S_OPT_LZ4_BLOCK_SIZE_LARGE
                                          // (ABI 10, up to kBatchMaxBlock)
constexpr int kLz4U32From = 65536 + 11;   // LZ4_64Klimit: from this chunk LENGTH on liblz4 parses with its 4096 x u32 table, a 5-byte
                                          // hash and a distance test (byU32): kItemLz4ChunkU32, lz4_compress_u32_kernel
constexpr int kBatchMaxBlock = 1 << 25;   // largest LZ4Block frame the batch decoder takes (lz4-java's MAX_BLOCK_SIZE); also the
                                          // largest Snappy chunk of both sides (spark.io.compression.snappy.blockSize, ABI 9)
constexpr int kSnappyFragment = 65536;    // snappy::RawCompress compresses its input in independent 64 KiB fragments
constexpr int kSlotHeader = 32;           // bytes reserved in front of a slot's payload
constexpr int kLz4FrameHeader = 21;       // "LZ4Block" + token + 3 x i32
constexpr int kSnappyStreamHeader = 16;
constexpr uint32_t kLz4BlockSeed = 0x9747b28cu;

// plan record kinds
enum : int32_t {
  kItemLz4Chunk = 0,     // LZ4Block data frame (header + payload, payload may be RAW)
  kItemLz4End = 1,       // 21-byte end-of-stream frame
  kItemSnappyHeader = 2, // 16-byte SnappyOutputStream header
  kItemSnappyChunk = 3,  // i32 BE length + raw snappy (a chunk of at most one fragment: <= kSnappyFragment bytes)
  // a Snappy chunk above one fragment (ABI 9): a head item, then one kItemSnappyFrag item per 64 KiB fragment, in order
  kItemSnappyChunkHead = 4,  // i32 BE length + varint32(len); len = the whole chunk.  Its size is known from len; the
                             // length VALUE is the sum of the fragments' sizes, written by the gather (assemble.hip)
  kItemSnappyFrag = 5,       // one fragment's raw snappy elements (no preamble), compressed on its own wavefront
  // an LZ4Block data frame whose chunk is kLz4U32From bytes or longer (ABI 10): the same frame, slot and item_size as
  // kItemLz4Chunk, parsed by the byU32 kernel.  A kind of its own, so that the kernels of the <= 64 KiB path pass it by
  // without a length test of their own.
  kItemLz4ChunkU32 = 6,
  // Zstandard map side (ABI 11, zstd_compress.hip): one frame per non-empty segment
  kItemZstdHeader = 7,   // the 14-byte frame header; src_off holds the segment's length (Frame_Content_Size)
  kItemZstdBlock = 8,    // one block of at most kZstdBlock bytes: 3-byte header right-aligned in the slot header, content from
                         // +32; kind bit 8 = Last_Block; item_size bit 31 = Raw_Block (content copied from the source)
  // LZF map side (S3S_OPT_LZF_COMPRESS, lzf_compress.hip): one chunk of at most kLzfChunk bytes - the 7-byte ('Z' 'V' 1 | clen |
  // ulen) or 5-byte ('Z' 'V' 0 | len) header right-aligned in the slot header, the liblzf block from +32; item_size bit 31 =
  // stored chunk (bytes copied from the source)
  kItemLzfChunk = 9,
  // Spark IO encryption (s3s_set_io_encryption, aes_ctr.hip): 16 bytes in front of the first item of every non-empty partition.
  // The gather leaves them alone; the AES-CTR pass behind it writes the partition's IV there.  No codec kernel knows the
  // kind: launch_seed_iv_items gives the records their item_size
  kItemIv = 10
};
constexpr int kLzfChunk = 65535;          // source bytes of an LZFOutputStream chunk (= s3s_lzf_enc::kChunk)
constexpr int kLzfSlotPayload = (kLzfChunk + kLzfChunk / 32 + 4 + 15) & ~15;  // the largest block the parse writes, rounded up
constexpr int kZstdBlock = 1 << 17;       // Block_Maximum_Size of the frames the map side writes (= s3s_zstd_enc::kBlock)
constexpr int kZstdFrameHeader = 14;      // magic | descriptor | window | 8-byte content size (= s3s_zstd_enc::kFrameHeader)

// bytes of snappy's varint32 preamble of a block of n bytes
__host__ __device__ constexpr int snappy_varint_len(int64_t n) {
  return n < (1 << 7) ? 1 : n < (1 << 14) ? 2 : n < (1 << 21) ? 3 : n < (1 << 28) ? 4 : 5;
}

struct Item {
  int64_t src_off;  // offset of the chunk in the uncompressed source (chunks only)
  int32_t len;      // uncompressed chunk length (chunks only)
  int32_t kind;     // low 8 bits: kind; bits 8..15: LZ4Block level nibble; bits 16..: unused
  int32_t chunk;    // slot index for chunk items, -1 otherwise
  int32_t part;     // owning partition
};

// item_size bit 31 marks an LZ4 chunk stored RAW (payload copied from the source)
constexpr uint32_t kRawFlag = 0x80000000u;

// ---- kernel launchers (each defined next to its kernel) ---------------------------------
// LZ4: compress every kItemLz4Chunk item into its slot, write the frame header, item_size.
//   d_item_check: per-item xxHash32 workspace (written by the xxh32 pre-pass)
//   variant 0: chunk staged in LDS (3 wavefronts/CU); 1: chunk read through L1/L2 (10/CU);
//   2: as 1 plus the window-speculative parse (default)
//   slot_stride: bytes between slots (kSlotHeader + the block size rounded up to 16)
//   has_u32: the items may hold kItemLz4ChunkU32 records (block size >= kLz4U32From): their hash pass and the byU32 parse
//   are two more launches over the same items
//   work_is_zero: *d_work is already zero in stream order (it travelled with the caller's upload): no memset is queued
void launch_lz4_compress(const uint8_t* d_src, const Item* d_items, int32_t n_items,
                         uint32_t* d_item_check, uint8_t* d_slots, int32_t slot_stride, uint32_t* d_item_size, uint32_t* d_work, int resident_waves,
                         int variant, hipStream_t st, hipEvent_t after_hash = nullptr, bool has_u32 = false, bool work_is_zero = false);
//   variant 11 (lz4_compress_ring.hip): the exact-window kernel with the input ring, launched by launch_lz4_compress
void launch_lz4_compress_ring_kernel(const uint8_t* d_src, const Item* d_items, int32_t n_items, uint32_t* d_item_check, uint8_t* d_slots,
                                     int32_t slot_stride, uint32_t* d_item_size, uint32_t* d_work, int grid, hipStream_t st);
// Snappy: same for kItemSnappyChunk.
bool snappy_compress_available();
//   slot_stride: bytes between slots (a raw snappy block can be larger than its chunk)
void launch_snappy_compress(const uint8_t* d_src, const Item* d_items, int32_t n_items,
                            uint8_t* d_slots, int64_t slot_stride, uint32_t* d_item_size,
                            int variant, hipStream_t st);  // variant 0: batch only, 1: exact windows first
// Zstandard: every kItemZstdBlock item into its slot (and its item_size), kItemZstdHeader items get their constant size.
//   d_scratch: grid x zstd_compress_scratch_stride() bytes (sequences and literals of the block a workgroup is working on)
int64_t zstd_compress_scratch_stride();
void launch_zstd_compress(const uint8_t* d_src, const Item* d_items, int32_t n_items, uint8_t* d_slots, int64_t slot_stride,
                          uint32_t* d_item_size, uint8_t* d_scratch, int32_t grid, hipStream_t st);
// LZF: every kItemLzfChunk item into its slot (and its item_size); one wavefront per item
void launch_lzf_compress(const uint8_t* d_src, const Item* d_items, int32_t n_items, uint8_t* d_slots, int64_t slot_stride,
                         uint32_t* d_item_size, hipStream_t st);
// ---- Spark IO encryption: AES-CTR over the stored bytes (aes_ctr.hip) ----------------------------------------------------
struct AesKeys {
  uint32_t rk[60];  // FIPS-197 round keys as big-endian words, 4 x (rounds + 1) of them in use; a kernel ARGUMENT, never in HBM
};
// rounds (10 / 12 / 14) for a key of 16 / 24 / 32 bytes, 0 (nothing written) for any other length
int aes_expand_key(const uint8_t* key, int key_bytes, AesKeys* keys);
enum { kCtrInPlace = 0, kCtrFromPlain = 1, kCtrDecrypt = 2 };
// stored partition p = d_stored_off[p] .. d_stored_off[p + 1] (n_parts + 1 DEVICE offsets; a non-empty one is IV | cipher text)
//   kCtrInPlace    d_out holds 16 free bytes + the plain bytes of every non-empty partition: writes d_ivs[16 p ..] and XORs in place
//   kCtrFromPlain  plain partition p at d_in + d_plain_off[p]  ->  IV | cipher text at d_out + d_stored_off[p]
//   kCtrDecrypt    stored bytes at d_in + d_stored_off[p]  ->  plain bytes at d_out + d_plain_off[p]; the IV is read from d_in
// stored_bound: what the host knows d_stored_off[n] - d_stored_off[0] not to exceed (sizes the grid; at most aes_ctr_max_bytes());
// stored_limit: no stored byte at or beyond this offset is touched whatever the device-side offsets say
int64_t aes_ctr_max_bytes();
void launch_aes_ctr(int mode, const AesKeys& keys, int rounds, const uint8_t* d_in, uint8_t* d_out, const int64_t* d_stored_off,
                    const int64_t* d_plain_off, const uint8_t* d_ivs, int32_t n_parts, int64_t stored_bound, int64_t stored_limit,
                    hipStream_t st);
// The window form (aes_ctr_stream.hip; the arithmetic is aes_ctr_stream_core.h): the stored window d_in[0, window_len) of a
// streamed range -> its plain bytes, IVs dropped.  d_stored_off[n_pieces + 1] are the window's pieces of partitions (window-
// relative, [0] = 0, [n_pieces] = window_len; every piece but the first starts with its partition, and an IV is whole in the
// window or its piece is empty), d_plain_off[n_pieces + 1] where their plain bytes go in d_out.  `front` stored bytes of piece
// 0's partition lie in front of the window: 0, or >= 16 and iv0 is that partition's IV (four big-endian words).  The IV of
// every piece that starts with one is copied to d_iv_out[16 piece ..].
struct AesWindowIv {
  uint32_t w[4];
};
void launch_aes_ctr_window(const AesKeys& keys, int rounds, const AesWindowIv& iv0, const uint8_t* d_in, uint8_t* d_out,
                           const int64_t* d_stored_off, const int64_t* d_plain_off, uint8_t* d_iv_out, int32_t n_pieces, int64_t front,
                           int64_t window_len, hipStream_t st);
// The window form over the windows of a batched feed, one launch: window i is d_wins[i] (what launch_aes_ctr_window takes as
// arguments, in device memory; tile0 = its first tile in the launch), tile t of the launch belongs to window d_tile_win[t].
// aes_ctr_window_tiles is the number of tiles a window owns (0 without a plain piece or a stored byte).  The carried IV of a
// window is in its descriptor (an IV is stored in the clear in the stream); the round keys are kernel arguments as everywhere.
struct AesWindow {
  const uint8_t* in;   // the stored window
  uint8_t* out;        // its plain bytes
  const int64_t* E;    // m + 1 stored piece offsets, window-relative
  const int64_t* Q;    // m + 1 plain piece offsets
  uint8_t* iv_out;     // 16 x m
  int32_t m, tile0;
  int64_t front, L;    // L = E[m]
  AesWindowIv iv;      // the carried IV (front > 0)
};
int32_t aes_ctr_window_tiles(int32_t n_pieces, int64_t front, int64_t window_len);
void launch_aes_ctr_window_batch(const AesKeys& keys, int rounds, const AesWindow* d_wins, const int32_t* d_tile_win, int32_t total_tiles,
                                 hipStream_t st);
// The map-side stream's form (aes_ctr_cstream.hip; the same arithmetic): the output d_dst[0, out_len) of one feed -> IV | cipher
// text.  d_piece_off[n_pieces + 1] are the stored piece offsets of the output ([0] = 0, [n_pieces] = out_len, pieces behind the
// cut empty), d_ivs one IV per piece (entry 0: the open partition's carried IV when `front` > 0 stored bytes of it lie in front
// of the output).  out_bound: what the host knows out_len not to exceed (sizes the grid).
//   kCsInPlace    d_dst holds a 16-byte hole + the plain bytes of every partition that starts in it; out_len is d_cut[kCutOutLen]
//   kCsFromPlain  plain piece p at d_src + d_plain_off[p] (piece 0: its bytes behind the front)  ->  d_dst; out_len = out_bound
enum { kCsInPlace = 0, kCsFromPlain = 1 };
void launch_aes_ctr_cstream(int mode, const AesKeys& keys, int rounds, const uint8_t* d_src, uint8_t* d_dst, const int64_t* d_piece_off,
                            const int64_t* d_plain_off, const uint8_t* d_ivs, const int64_t* d_cut, int32_t n_pieces, int64_t front,
                            int64_t out_bound, hipStream_t st);
// ... over the outputs of all windows of a batched feed, in place, one launch (aes_ctr_cstream_batch.hip): window i is
// d_wins[i], an s3s_cs::PassWindow (compress_stream_batch_core.h: d_dst, its clamped piece offsets, its IVs, its cut words, its
// first tile in the launch, its front), tile t of the launch belongs to window d_tile_win[t]; s3s_cs::pass_tiles sizes a window
void launch_aes_ctr_cstream_batch(const AesKeys& keys, int rounds, const void* d_wins, const int32_t* d_tile_win, int32_t total_tiles,
                                  hipStream_t st);
// item_size = 16 for every kItemIv record (between the codec kernels and the scan)
void launch_seed_iv_items(const Item* d_items, int32_t n_items, uint32_t* d_item_size, hipStream_t st);
// exclusive scan of item sizes + partition index extraction
void launch_scan_items(const Item* d_items, const uint32_t* d_item_size, int32_t n_items,
                       int64_t* d_item_off, const int32_t* d_part_first, int32_t n_parts,
                       int64_t* d_index, hipStream_t st);
// copy every item to its place in the .data image; sets *d_status != 0 on capacity overflow
void launch_gather_items(const uint8_t* d_src, const Item* d_items, int32_t n_items,
                         const uint8_t* d_slots, int64_t slot_stride, const uint32_t* d_item_size,
                         const int64_t* d_item_off, uint8_t* d_dst, int64_t dst_capacity,
                         int32_t* d_status, hipStream_t st);
// per-range Adler32 / CRC32: out[i] over data[offsets[i], offsets[i+1])
//   d_seg_start[n+1]: prefix of worst-case 16 KiB segment counts (host-built from upper bounds)
//   d_tables: constant tables (checksum_tables_build), d_partial: 4 x uint32 per segment slot
size_t checksum_tables_bytes();
void checksum_tables_build(void* host_buf);
//   max_segs_per_range / d_partial2: a range of more than kChecksumFoldFrom segments has groups of kChecksumFoldGroup
//   segments folded first (checksum_fold_kernel); d_partial2 then holds 4 x uint32 per (range, group):
//   n x checksum_fold_groups(n, max_segs_per_range) entries.  nullptr / 0: no folding (one wavefront folds a whole range).
void launch_checksum_with_tables(int algo, const uint8_t* d_data, const int64_t* d_offsets,
                                 int32_t n, const int32_t* d_seg_start, int32_t total_segs,
                                 const void* d_tables, uint32_t* d_partial, int64_t* d_out,
                                 int64_t data_len /* bytes readable at d_data */, hipStream_t st,
                                 int32_t max_segs_per_range = 0, uint32_t* d_partial2 = nullptr);
// ---- batched tails (round 6) --------------------------------------------------------------------------------------------
// A batched call used to launch its small kernels PER TASK (scan, gather, memset + segments + combine of the checksums: six
// launches per map task, 2 - 5 us each plus the gap between them): 32 blocks of 8 MiB in one call spent 2.2 of its 5.6 ms
// there (profiles/r06e_*).  One descriptor per task / fetched range, uploaded with the plan; every tail kernel is launched
// ONCE per call and finds its task by a binary search over the descriptors (a handful of scalar loads).
struct TaskTail {
  int32_t first_item, n_items;   // compress: the task's plan records (scan / gather)
  int32_t first_pp, n_parts;     // its partitions in the packed arrays that hold n + 1 entries per task (index, part_first, seg_start)
  int32_t first_part;            // ... and in the arrays that hold n entries per task (checksums out)
  int32_t first_seg;             // its first checksum segment slot in the call's partial array (seg_start is task-relative)
  int32_t n_segs, pad;
  const uint8_t* data;           // what the checksums run over: the task's .data image / the fetched range
  int64_t data_len;              // bytes readable there
  uint8_t* dst;                  // compress: the .data image the gather writes
  int64_t dst_capacity;
};
void launch_scan_items_batch(const TaskTail* d_tails, int32_t n_tasks, const uint32_t* d_item_size, int64_t* d_item_off,
                             const int32_t* d_part_first, int64_t* d_index, hipStream_t st);
void launch_gather_items_batch(const TaskTail* d_tails, int32_t n_tasks, int32_t n_items_total, const uint8_t* d_src, const Item* d_items,
                               const uint8_t* d_slots, int64_t slot_stride, const uint32_t* d_item_size, const int64_t* d_item_off,
                               int32_t* d_status, hipStream_t st);
// checksums of every task's ranges: offsets / seg_start packed (n + 1 per task), partial zeroed here, out packed (n per task)
void launch_checksum_batch(int algo, const TaskTail* d_tails, int32_t n_tasks, int32_t total_segs, int32_t total_parts,
                           const int64_t* d_offsets, const int32_t* d_seg_start, const void* d_tables, uint32_t* d_partial,
                           int64_t* d_out, hipStream_t st);
constexpr int kChecksumSegBytes = 16384;
constexpr int kChecksumFoldGroup = 256;   // segments per folded group (4 MiB)
constexpr int kChecksumFoldFrom = 2048;   // a range with more segments than this (32 MiB) is folded in two levels
// groups per range of the folded layout, 0 = do not fold (no range is large, or n x groups would not be small)
inline int32_t checksum_fold_groups(int32_t n, int32_t max_segs_per_range) {
  if (max_segs_per_range <= kChecksumFoldFrom) return 0;
  const int64_t g = ((int64_t)max_segs_per_range + kChecksumFoldGroup - 1) / kChecksumFoldGroup;
  return (int64_t)n * g <= (1 << 20) ? (int32_t)g : 0;
}

// reduce side ------------------------------------------------------------------------------
struct Frame {        // one discovered codec frame
  int64_t comp_off;   // payload offset in the compressed range
  int32_t comp_len;   // payload bytes
  int32_t orig_len;   // decoded bytes
  uint32_t check;     // LZ4Block: xxh32 & 0x0FFFFFFF; snappy: unused
  int32_t method;     // 0x10 raw / 0x20 lz4 (LZ4Block); 1 = snappy chunk; LZF: 0x10 stored chunk / 2 compressed chunk
};
// LZ4Block frame discovery over the whole range (see lz4_decompress.hip): 64 KiB tiles are
// walked speculatively, resolved into the true chain, then emitted in stream order.
//   d_spec_count[n_tiles] (as uint32) -> d_frame_base[n_tiles+1] (exclusive scan; last = n_frames)
int32_t lz4_tile_count(int64_t comp_len);
// one fetched range of a batched reduce-side call (s3s_decompress_ranges_batch_device): the discovery kernels of ALL
// ranges run as one launch each (block -> range through a host-built tile map)
struct LzRange {
  const uint8_t* comp;
  int64_t comp_len;
  int32_t n_tiles, tile0;  // tiles of this range, index of its first tile in the batch-wide tile list
  int64_t *spec_entry, *spec_exit, *true_entry, *frame_base;
  int32_t* spec_count;
  int32_t* status;         // per-range status word
  int64_t* result;         // [0] = frames of the range (phase 1), [1] = decoded bytes (phase 2)
  // phase 2, filled by the host once the frame counts are known
  Frame* frames;
  uint32_t* frame_orig;
  int64_t* frame_out;      // n_frames + 1 offsets relative to the range's destination
  int64_t* out_abs;        // absolute output address per frame (the one decode launch runs with dst = nullptr)
  int64_t n_frames;
  int64_t dst_base, dst_capacity;
  int32_t skip, pad;       // the range failed an earlier check: its frames become empty
};
void launch_lz4_discover_batch(const LzRange* d_ranges, int32_t n_ranges, const int32_t* d_tile_range,
                               int32_t total_tiles, hipStream_t st);
void launch_lz4_frames_batch(LzRange* d_ranges, int32_t n_ranges, const int32_t* d_tile_range, int32_t total_tiles,
                             hipStream_t st);
void launch_lz4_discover(const uint8_t* d_comp, int64_t comp_len, int32_t n_tiles,
                         int64_t* d_spec_entry, int64_t* d_spec_exit, int32_t* d_spec_count,
                         int64_t* d_true_entry, int64_t* d_frame_base, int32_t* d_status,
                         hipStream_t st);
//   writes d_frames[n_frames], d_frame_orig[n_frames] and d_frame_out[n_frames+1] (scan of
//   decoded sizes; last = total decoded bytes)
void launch_lz4_emit_frames(const uint8_t* d_comp, int64_t comp_len, int32_t n_tiles,
                            const int64_t* d_true_entry, const int64_t* d_frame_base,
                            Frame* d_frames, uint32_t* d_frame_orig, int64_t n_frames,
                            int64_t* d_frame_out, int32_t* d_status, hipStream_t st);
//   variant 0: frame staged in LDS (3 frames per CU); 1: straight to global memory (no LDS)
//   after_decode (optional): recorded between the decode kernel and the frame-check kernel of variant 4
void launch_lz4_decompress(const uint8_t* d_comp, const Frame* d_frames, int32_t n_frames,
                           const int64_t* d_frame_out, uint8_t* d_dst, int32_t* d_status,
                           int variant, hipStream_t st, hipEvent_t after_decode = nullptr);
//   variant 4: batches of sequences, one lane per sequence (lz4_decode_batch.hip)
void launch_lz4_decompress_batch(const uint8_t* d_comp, const Frame* d_frames, int32_t n_frames,
                                 const int64_t* d_frame_out, uint8_t* d_dst, int32_t* d_status,
                                 hipStream_t st, hipEvent_t after_decode = nullptr);
void launch_snappy_decompress_batch(const uint8_t* d_comp, const Frame* d_frames, int32_t n_frames,
                                    const int64_t* d_frame_out, uint8_t* d_dst, int32_t* d_status,
                                    hipStream_t st);
void launch_lzf_decompress_batch(const uint8_t* d_comp, const Frame* d_frames, int32_t n_frames,
                                 const int64_t* d_frame_out, uint8_t* d_dst, int32_t* d_status, hipStream_t st);
// Snappy (SnappyInputStream framing): chunks are chained by their i32 BE length only, so the walk
// is one lane per partition (each non-empty partition is one or more complete streams, each
// starting with the 16-byte header).  Pass 1 counts, pass 2 (after a scan of the counts) writes
// d_frames / d_frame_orig at d_frame_base[partition].
// chunk_format: kChunkSnappy, or kChunkLzf (round 4: compress-lzf chunks 'Z' 'V' type | len BE [| ulen BE]; stored chunks
// become frames with method 0x10, compressed ones method 2) - the same two passes, the same batch decoder behind them.
enum { kChunkSnappy = 0, kChunkLzf = 1 };
void launch_snappy_count_frames(const uint8_t* d_comp, const int64_t* d_part_off, int32_t n_parts,
                                uint32_t* d_part_nframes, int32_t* d_status, hipStream_t st, int chunk_format = kChunkSnappy);
void launch_snappy_emit_frames(const uint8_t* d_comp, const int64_t* d_part_off, int32_t n_parts,
                               const int64_t* d_frame_base, Frame* d_frames, uint32_t* d_frame_orig,
                               int32_t* d_status, hipStream_t st, int chunk_format = kChunkSnappy);
//   variant 0: block staged in LDS; otherwise the VALU ring decoder
void launch_snappy_decompress(const uint8_t* d_comp, const Frame* d_frames, int32_t n_frames,
                              const int64_t* d_frame_out, uint8_t* d_dst, int32_t* d_status,
                              int variant, hipStream_t st, int chunk_format = kChunkSnappy);
void launch_scan_u32(const uint32_t* d_in, int64_t n, int64_t* d_out, hipStream_t st);

// ---- streaming reduce side (decode_stream.hip: s3s_dstream_feed*; its host rules: decode_stream_core.h) ---------------------
// The window comp[0, comp_len) starts on a unit boundary of the range and may end inside a unit; range_left >= comp_len is
// what the RANGE still holds from the window's start.  A unit that crosses comp_len ends the chain there (d_result[0] = the
// stop offset, d_result[1] = the unit's length as far as the window shows it: header + payload when the header is whole,
// else the header's length; 0 when the chain ends on a unit boundary); one that crosses range_left too, and anything
// malformed, raises *d_status as in the one-shot kernels.  No byte at or beyond comp_len is read.
//   LZ4Block: the one-shot speculation (launch_lz4_speculate), then a resolve that stops instead of failing, then the scan of
//   the tile counts (d_frame_base[n_tiles] = frames in front of the stop).  The frames are emitted by launch_lz4_emit_frames with the stop
//   offset as comp_len.
void launch_lz4_speculate(const uint8_t* d_comp, int64_t comp_len, int32_t n_tiles, int64_t* d_spec_entry, int64_t* d_spec_exit,
                          int32_t* d_spec_count, hipStream_t st);
void launch_lz4_discover_stream(const uint8_t* d_comp, int64_t comp_len, int64_t range_left, int32_t n_tiles,
                                int64_t* d_spec_entry, int64_t* d_spec_exit, int32_t* d_spec_count, int64_t* d_true_entry,
                                int64_t* d_frame_base, int32_t* d_status, int64_t* d_result, hipStream_t st);
//   Snappy / LZF: d_piece_off[n_pieces + 1] are the pieces of partitions inside the window (window-relative).  Piece 0
//   starts inside a Snappy stream when first_mid != 0 (no stream header expected there); the partition of the last piece
//   ends at last_pend >= d_piece_off[n_pieces] (beyond the window: its last unit may be cut).
void launch_snappy_count_frames_stream(const uint8_t* d_comp, const int64_t* d_piece_off, int32_t n_pieces, int32_t first_mid,
                                       int64_t last_pend, uint32_t* d_piece_nframes, int32_t* d_status, int64_t* d_result,
                                       hipStream_t st, int chunk_format);
void launch_snappy_emit_frames_stream(const uint8_t* d_comp, const int64_t* d_piece_off, int32_t n_pieces, int32_t first_mid,
                                      int64_t last_pend, const int64_t* d_frame_base, Frame* d_frames, uint32_t* d_frame_orig,
                                      int32_t* d_status, hipStream_t st, int chunk_format);
//   The cut of a frame table at the caller's output capacity, behind the scan of the decoded sizes: k = the largest index
//   with d_frame_out[k] <= dst_capacity.  d_result = {k, consumed, out_len, need}: consumed = where unit k starts (the stop
//   offset when k == n_frames), out_len = d_frame_out[k], need = decoded bytes of frame k (0 when k == n_frames).
void launch_frames_cut(int codec, const Frame* d_frames, const uint32_t* d_frame_orig, const int64_t* d_frame_out, int64_t n_frames,
                       int64_t dst_capacity, int64_t stop, int64_t* d_result, hipStream_t st);
//   java.util.zip.Checksum continued: d_out[i] (the checksum of range i alone) becomes the state after range i when it was
//   d_seeds[i] before (getValue() of the bytes so far) - the combine identities with the seed as one more leading term.
void launch_checksum_seed(int algo, const int64_t* d_offsets, int32_t n, const void* d_tables, const int64_t* d_seeds,
                          int64_t* d_out, hipStream_t st);

// ---- batched feed (decode_stream.hip: s3s_dstream_feed_batch*, the same host rules; kernels: decode_stream_batch.hip) ------
// One window of each of several streams per call.  A window is an LzRange - comp / comp_len = the window, status = its status
// word, result = its kWinWords result words ([0] stop, [1] need, [2] frames in front of the stop; [4] k, [5] consumed,
// [6] out_len, [7] decoded bytes of frame k), spec_count / frame_base = per tile (LZ4) or per piece (Snappy, LZF) - plus a
// StreamWin.  The kernels are the single feed's with the window found through the descriptors; each is ONE launch per call.
constexpr int kWinWords = 8;
struct StreamWin {
  int64_t range_left;    // LZ4: what the range still holds from the window's start (launch_lz4_discover_stream)
  int64_t last_pend;     // Snappy / LZF: where the last piece's partition ends (launch_snappy_count_frames_stream)
  int32_t first_piece;   // the window's first piece in the batch-wide piece list; it owns n_pieces + 1 consecutive offsets,
  int32_t n_pieces;      // so its offsets start at first_piece + the window's index
  int32_t first_mid, pad;
  int64_t stop;          // phase 2: the stop offset discovery returned
  int64_t first_frame;   // phase 2: the window's first frame in the batch-wide frame table
};
//   the per-tile launches of launch_lz4_discover_batch / launch_lz4_frames_batch on their own (lz4_decompress.hip)
void launch_lz4_speculate_batch(const LzRange* d_ranges, const int32_t* d_tile_range, int32_t total_tiles, hipStream_t st);
void launch_lz4_emit_batch(const LzRange* d_ranges, const int32_t* d_tile_range, int32_t total_tiles, hipStream_t st);
//   LZ4: one wavefront per window resolves the chain with the stop rule and scans the tile counts
void launch_lz4_resolve_stream_batch(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, hipStream_t st);
//   Snappy / LZF: one lane per piece of every window (d_piece_win: piece -> window); count is followed by the per-window scan
void launch_snappy_count_stream_batch(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, const int64_t* d_piece_off,
                                      const int32_t* d_piece_win, int32_t total_pieces, int chunk_format, hipStream_t st);
void launch_snappy_emit_stream_batch(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, const int64_t* d_piece_off,
                                     const int32_t* d_piece_win, int32_t total_pieces, int chunk_format, hipStream_t st);
//   the scan of every window's decoded sizes and its cut at its own dst_capacity (launch_frames_cut per window)
void launch_frames_cut_batch(int codec, const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, hipStream_t st);
//   absolute addresses for the frames in front of every window's cut, empty frames behind it and for a window with skip set
void launch_frames_rebase_cut(const LzRange* d_ranges, const StreamWin* d_wins, int32_t n_wins, int64_t total_frames, hipStream_t st);
//   launch_checksum_seed over the flattened piece table (d_offsets: n_pieces + 1 per window, d_seeds / d_out: one per piece)
void launch_checksum_seed_batch(int algo, const int64_t* d_offsets, const int32_t* d_piece_win, int32_t total_pieces,
                                const void* d_tables, const int64_t* d_seeds, int64_t* d_out, hipStream_t st);

// ---- streaming map side (compress_stream.hip: s3s_cstream_feed*) -----------------------------------------------------------
//   The cut of a window's plan at the caller's output capacity, behind the scan of the item sizes (compress_stream_kernels.hip;
//   the arithmetic is compress_stream_core.h).  d_marks: one s3s_cs::Mark per item; d_part_first[n_pieces + 1]: first item of
//   every piece of a partition (the last piece is the partition the window leaves open); first_last: the last item of the
//   first unit (-1: no unit); ends0: ends passed in front of the first unit; open_img: image bytes the open partition has
//   already.  d_result[s3s_cs::kCutWords]; d_piece_off[n_pieces + 1]; d_lengths[n_pieces - 1].
void launch_cstream_cut(const void* d_marks, const int64_t* d_item_off, int32_t n_items, const int32_t* d_part_first, int32_t n_pieces,
                        int64_t dst_capacity, int32_t first_last, int32_t ends0, int64_t open_img, int64_t* d_result,
                        int64_t* d_piece_off, int64_t* d_lengths, hipStream_t st);
//   launch_gather_items for the items [0, d_cut[0]) - the cut is read on the device, the grid covers all n_items
void launch_gather_items_cut(const uint8_t* d_src, const Item* d_items, int32_t n_items, const int64_t* d_cut,
                             const uint8_t* d_slots, int64_t slot_stride, const uint32_t* d_item_size,
                             const int64_t* d_item_off, uint8_t* d_dst, int64_t dst_capacity,
                             int32_t* d_status, hipStream_t st);
// ---- batched feed of the streaming map side (compress_stream.hip: s3s_cstream_feed_batch*; kernels:
//      compress_stream_batch_kernels.hip; the layout of the call's packed arrays: compress_stream_batch_core.h) -----------------
//   launch_cstream_cut for the windows of all entries, one wavefront each.  d_cuts: one s3s_cs::CutEntry per entry; d_marks,
//   d_item_off, d_part_first and the three outputs are the call's packed arrays (d_result: s3s_cs::kCutWords words an entry)
void launch_cstream_cut_batch(const void* d_cuts, int32_t n_entries, const void* d_marks, const int64_t* d_item_off,
                              const int32_t* d_part_first, int64_t* d_result, int64_t* d_piece_off, int64_t* d_lengths, hipStream_t st);
//   launch_gather_items_cut over the items of all entries: entry e's items [0, d_result[kCutWords e]) go to d_tails[e].dst and
//   never at or beyond d_tails[e].dst_capacity; d_status: one word an entry
void launch_gather_items_cut_batch(const TaskTail* d_tails, int32_t n_entries, int32_t n_items_total, const uint8_t* d_src,
                                   const Item* d_items, const int64_t* d_result, const uint8_t* d_slots, int64_t slot_stride,
                                   const uint32_t* d_item_size, const int64_t* d_item_off, int32_t* d_status, hipStream_t st);

// ---- device helpers shared by several kernels --------------------------------------------
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) {
  return __builtin_amdgcn_alignbit(x, x, 32 - r);
}

// unaligned 32-bit read from LDS: two aligned dwords + v_alignbyte
__device__ __forceinline__ uint32_t lds_rd32(const uint8_t* base, int pos) {
  const uint32_t* p = reinterpret_cast<const uint32_t*>(base + (pos & ~3));
  const uint32_t lo = p[0], hi = p[1];
  return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)pos & 3u);
}

}  // namespace s3s
