/*
 * s3shuffle_codec.h — C-ABI of the MI355X-native shuffle-block codec path.
 *
 * This is the drop-in boundary for ONE hot path of IBM/spark-s3-shuffle: the map-side
 * compress + checksum of a map task's shuffle partitions and the reduce-side verify +
 * decompress of a fetched block range.  Everything above it (ShuffleManager /
 * ShuffleDataIO SPI, object-store I/O, lifecycle) stays on the JVM unchanged; a thin JNI
 * shim binds exactly these entry points.  Plain pointers and sizes only.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo,
 * src/main/scala/org/apache/spark/...):
 *
 *   s3s_compress_map_output        the [EXT] LZ4BlockOutputStream / SnappyOutputStream +
 *                                  MutableCheckedOutputStream stage that feeds
 *                                  shuffle/S3ShuffleMapOutputWriter.scala:168-202
 *                                  (S3ShuffleOutputStream.write) and whose per-partition
 *                                  lengths / checksums are persisted by
 *                                  shuffle/S3ShuffleMapOutputWriter.scala:91-118
 *                                  (commitAllPartitions) through
 *                                  shuffle/helper/S3ShuffleHelper.scala:44-59
 *                                  (writePartitionLengths / writeChecksum); also the
 *                                  pre-built spill file + lengths + checksums handed to
 *                                  shuffle/S3SingleSpillShuffleMapOutputWriter.scala:24-64.
 *   s3s_checksum_ranges            shuffle/helper/S3ShuffleHelper.scala:94-103
 *                                  (createChecksumAlgorithm) as used by
 *                                  storage/S3ChecksumValidationStream.scala:54-66.
 *   s3s_decompress_range           storage/S3ChecksumValidationStream.scala:17-92 (verify)
 *                                  + the [EXT] serializerManager.wrapStream decompression
 *                                  at storage/S3ShuffleReader.scala:98-110, over the byte
 *                                  range storage/S3ShuffleBlockIterator.scala:37-42 /
 *                                  storage/S3ShuffleBlockStream.scala:36-40 define.
 *   s3s_decompressed_size          (no reference counterpart: sizing helper for the shim;
 *                                  the JVM path grows its buffers while streaming)
 *   s3s_max_compressed_size        (sizing helper; LZ4BlockOutputStream allocates
 *                                  HEADER_LENGTH + maxCompressedLength(blockSize) per block)
 *   s3s_create / s3s_destroy       shuffle/helper/S3ShuffleDispatcher.scala:240-255 (the
 *                                  process-wide lazily built state); the device is chosen
 *                                  by the caller as mapId % nGPU, mirroring
 *                                  mapId % folderPrefixes at S3ShuffleDispatcher.scala:142.
 *
 * Byte formats produced / consumed (bit-exact with the JVM path):
 *   LZ4    one lz4-java LZ4BlockOutputStream per non-empty partition: frames of
 *          "LZ4Block" | token | compressedLen LE | originalLen LE | xxh32&0x0FFFFFFF LE |
 *          payload (LZ4_compress_default of a block_size chunk, or the raw chunk when that
 *          is not smaller), then a 21-byte end frame.  Empty partition = 0 bytes.
 *   SNAPPY one snappy-java SnappyOutputStream per non-empty partition: 16-byte header,
 *          then compressedLen BE | raw snappy per block_size chunk.
 *   NONE   the partition bytes unchanged (spark.shuffle.compress=false).
 *   out_index     cumulative offsets [0, L0, L0+L1, ...] (host-endian int64; the caller
 *                 serialises big-endian exactly like S3ShuffleHelper.writeArrayAsBlock).
 *   out_checksums java.util.zip.Adler32 / CRC32 getValue() over each partition's
 *                 COMPRESSED bytes, i.e. over data[index[p], index[p+1]).
 *
 * Threading: an s3s_ctx is NOT thread-safe; use one per task thread.  Calls on distinct
 * contexts are fully concurrent (each owns its HIP stream and device workspace).
 * Ownership: the caller owns every buffer passed in; the library owns only the ctx.
 * Errors: 0 on success, negative S3S_E_* otherwise; never aborts; s3s_last_error() gives
 * a message.  There is NO CPU fallback: without a usable HIP device s3s_create() fails.
 * Sizes: every offset, length and capacity is a full int64_t - a map output, a fetched range, a
 * checksum range or the sum of a batch may lie far above 4 GiB (tested: sources and images above
 * 2^32 + 64 MiB through the device entry points, offsets around 2^31 and 2^32 and buffers that
 * straddle a 4 GiB-aligned address in every kernel).  What is limited is the COUNT of pieces of one
 * call: more than 0x7fffff00 codec blocks, frames or 16 KiB checksum segments is S3S_E_UNSUPPORTED,
 * answered before anything is allocated or launched where the count follows from the arguments
 * alone (the compress entry points, s3s_decompress_range_device).
 */
#ifndef S3SHUFFLE_CODEC_H
#define S3SHUFFLE_CODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3S_ABI_VERSION 11 /* 2: + segments entry points, page-locked staging, tuning options 6, 7;
                             3: + s3s_compress_map_outputs_batch_device;
                             4: + s3s_decompress_ranges_batch_device; decode variants {3, 4}, LZ4 parses {1, 9, 10};
                             5: + s3s_compress_map_outputs_batch / s3s_decompress_ranges_batch (host buffers),
                                S3S_CODEC_ZSTD on the reduce side;
                             6: S3S_STATUS_NOT_RUN in the per-entry status of the batched calls (a call-level failure is told
                                apart from an entry's own verdict);
                             7: + S3S_CODEC_LZF on the reduce side; LZ4Block frames above 32 KiB through the batch decoder;
                             8: + S3S_CHECKSUM_CRC32C;
                             9: S3S_OPT_SNAPPY_BLOCK_SIZE up to 32 MiB (map side fragment-parallel), Snappy chunks of any
                                decoded length up to 32 MiB through the batch decoder;
                             10: + S3S_OPT_LZ4_BLOCK_SIZE_LARGE: LZ4 blocks up to 32 MiB on the map side (chunks of 65 547 bytes
                                 or more through liblz4's 32-bit-table parse);
                             11: + S3S_OPT_ZSTD_COMPRESS: S3S_CODEC_ZSTD on the map side (decode-compatible Zstandard frames);
                                 still 11: + S3S_OPT_LZF_COMPRESS (key 10): S3S_CODEC_LZF on the map side.  The key is additive and
                                 the version did not move: a library without it answers S3S_E_INVALID to
                                 s3s_set_option(ctx, 10, 1), and that answer is how callers detect support;
                                 still 11: + Spark IO encryption (AES/CTR/NoPadding) as a layer on both sides of the codec:
                                 s3s_set_io_encryption, s3s_set_stream_ivs and the read-only key 11.  Additive again: a caller
                                 detects support by the symbols, or by s3s_get_option(ctx, 11) answering 0 instead of
                                 S3S_E_INVALID;
                                 still 11: + S3S_OPT_ZSTD_DECODE_VARIANT (key 13) and the read-only S3S_OPT_ZSTD_DECODE_BLOCKS (key
                                 14): block-independent Zstandard frames decode one workgroup per block.  Additive: the output
                                 of every call is unchanged, a library without the keys answers S3S_E_INVALID to them;
                                 still 11: + S3S_OPT_ZSTD_DECODE_STAGED (key 15) and the read-only S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS
                                 (key 16): Zstandard frames WITH history across their blocks decode in stages - entropy per
                                 block, copies per frame.  Additive and off by default: the output of every call is unchanged,
                                 and a library without the keys answers S3S_E_INVALID to s3s_set_option(ctx, 15, 1) and to
                                 s3s_get_option(ctx, 16), which is how callers detect support */

/* spark.io.compression.codec (only when spark.shuffle.compress=true) */
enum { S3S_CODEC_NONE = 0, S3S_CODEC_LZ4 = 1, S3S_CODEC_SNAPPY = 2,
       S3S_CODEC_LZF = 4, /* reduce side (ABI 7): LZFCompressionCodec streams (compress-lzf chunks 'Z' 'V' type | len ...
                             around liblzf blocks, up to 65 535 bytes each) through the batch decoder.  compress-lzf's output
                             is not a function of the partition's bytes, so the compress entry points answer
                             S3S_E_UNSUPPORTED unless S3S_OPT_LZF_COMPRESS is 1: then they write, per non-empty segment, an
                             LZFOutputStream-shaped stream that every LZF decoder reads - NOT compress-lzf's bytes
                             (DESIGN.md 6g): chunks of 65 535 source bytes without history across chunks, a chunk whose block
                             is not two bytes shorter stored */
       S3S_CODEC_ZSTD = 3 /* reduce side (s3s_decompress_range*, s3s_decompressed_size): Zstandard frames as
                             ZStdCompressionCodec / zstd-jni write them, one per non-empty partition; the compress
                             entry points answer S3S_E_UNSUPPORTED (the codec stays on the JVM) unless
                             S3S_OPT_ZSTD_COMPRESS is 1 (ABI 11): then they write one frame per non-empty segment that every
                             Zstandard decoder reads - NOT libzstd's bytes: blocks of 128 KiB without history
                             across blocks, 8-byte Frame_Content_Size, no content checksum, no dictionary */ };
/* spark.shuffle.checksum.algorithm (NONE when spark.shuffle.checksum.enabled=false) */
enum { S3S_CHECKSUM_NONE = 0, S3S_CHECKSUM_ADLER32 = 1, S3S_CHECKSUM_CRC32 = 2,
       S3S_CHECKSUM_CRC32C = 3 /* ABI 8: java.util.zip.CRC32C (Castagnoli), Spark 4's third spark.shuffle.checksum.algorithm */ };

enum {
  S3S_OK = 0,
  S3S_E_INVALID = -1,     /* bad argument (RuntimeException("Precondition: ...") on the JVM) */
  S3S_E_CAPACITY = -2,    /* dst_capacity too small */
  S3S_E_BAD_FRAME = -3,   /* IOException("Stream is corrupted") */
  S3S_E_CHECKSUM = -4,    /* SparkException("Invalid checksum detected for ...") */
  S3S_E_HIP = -5,         /* HIP runtime / device failure */
  S3S_E_UNSUPPORTED = -6, /* e.g. block size outside the supported range */
  S3S_E_NOMEM = -7,
  S3S_STATUS_NOT_RUN = -100 /* only ever in s3s_map_task.status / s3s_fetch_range.status: every entry of a batch is stamped
                               with it on entry to the call, so that after a CALL-level failure (bad argument, HIP error
                               before or between the tasks) the entries the library never finished are told apart from the
                               ones that have their own verdict; the call's return code applies to exactly these */
};

/* option keys for s3s_set_option / s3s_get_option */
enum {
  S3S_OPT_LZ4_BLOCK_SIZE = 1,    /* spark.io.compression.lz4.blockSize, default 32768;
                                    map side: 64..65536 through THIS key (larger values: S3S_E_UNSUPPORTED, as before
                                    ABI 10 - callers use that answer to keep the JVM codec; larger blocks are the caller's
                                    explicit choice, key 8); the reduce side decodes frames of ANY block size whatever
                                    this option says.  s3s_get_option returns the block size in force, whichever key set it */
  S3S_OPT_SNAPPY_BLOCK_SIZE = 2, /* spark.io.compression.snappy.blockSize, default 32768;
                                    supported 1..33554432 (snappy-java raises values below 1024
                                    to 1024; larger values: S3S_E_UNSUPPORTED).  Since ABI 9 */
  S3S_OPT_PROFILE = 3,           /* 1: record per-stage HIP-event timings (s3s_stage_ms) */
  S3S_OPT_LZ4_VARIANT = 4,       /* tuning, identical output: 1 = general batch only (64 probes of the greedy
                                    parse per step), 10 = lean exact 64-byte windows in front of
                                    it (one candidate gather per window, several sequences per round trip),
                                    11 (default) = 10 with the last 4 KiB of the input kept in LDS, from which
                                    near match extensions are served (20 KiB of LDS per wavefront: 8 per CU),
                                    9 = auto: the context times 1 and 10 on its first large map outputs
                                    (1, 10, 1, 10), keeps the faster and re-measures the other every 32nd
                                    call; a batched call (s3s_compress_map_outputs_batch*) has no timing
                                    rounds and runs 11.  Other values are refused. */
  S3S_OPT_LZ4_VARIANT_USED = 7,  /* read-only: the parse (1, 10 or 11) the last LZ4 compress call ran */
  S3S_OPT_SNAPPY_VARIANT = 6,    /* tuning, identical output: 0 = general batch only, 1 (default) = exact
                                    64-byte windows in front of it (several copies per round trip) */
  S3S_OPT_LZ4_DECODE_VARIANT = 5, /* tuning, identical output, LZ4 and Snappy: 4 (default) = batch decoder
                                    (one sequence per lane, dependency rounds, sliding LDS output window),
                                    3 = ring decoder (one sequence per step, parse on the vector ALU) */
  S3S_OPT_LZ4_BLOCK_SIZE_LARGE = 8, /* since ABI 10: the same setting as key 1 with the range 64..33554432 (lz4-java's
                                    MAX_BLOCK_SIZE; above: S3S_E_UNSUPPORTED, below 64: S3S_E_INVALID).  Chunks of 65 547
                                    bytes or more are parsed as liblz4 parses them (4096 x u32 table, 5-byte hash, distance
                                    test) by the general batch whatever S3S_OPT_LZ4_VARIANT says (the exact windows are
                                    16-bit-table only; S3S_OPT_LZ4_VARIANT_USED reports the parse of the shorter chunks);
                                    shorter chunks - a partition's tail - keep the 16-bit-table kernel.  One wavefront
                                    parses one block, so a call needs ~2 560 blocks to fill the chip: throughput falls
                                    with the block size, and without the exact windows match-dense data is no faster than
                                    16 host cores already at 128k - measured only sort-like data at 128k gains (DESIGN.md 6d,
                                    INTEGRATION.md 1a).  Workspace: every chunk - a partition's short tail included -
                                    reserves a slot of 32 + blockSize bytes for the duration of the call, so a task of P
                                    non-empty partitions holds at least P x blockSize (200 partitions at 32m: 6.4 GiB per
                                    context); a call whose workspace cannot be allocated answers S3S_E_NOMEM */
  S3S_OPT_ZSTD_COMPRESS = 9,     /* since ABI 11: 0 (default) / 1, other values S3S_E_INVALID.  0: every compress entry point and
                                    s3s_max_compressed_size* answer S3S_CODEC_ZSTD as before ABI 11 (S3S_E_UNSUPPORTED, batch
                                    entries S3S_STATUS_NOT_RUN; S3S_E_INVALID from the sizing helpers) - callers use that
                                    answer to keep the JVM codec.  1: the caller's explicit choice of a decode-compatible
                                    writer: the output is a pure function of the source bytes, the offsets and the options,
                                    decodes under libzstd / zstd-jni and this library, and is not the byte stream libzstd
                                    would have written */
  S3S_OPT_LZF_COMPRESS = 10,     /* ABI 11, additive (a library without the key answers S3S_E_INVALID to setting it): 0 (default) /
                                    1, other values S3S_E_INVALID.  0: every compress entry point and s3s_max_compressed_size*
                                    answer S3S_CODEC_LZF as before (S3S_E_UNSUPPORTED, batch entries S3S_STATUS_NOT_RUN;
                                    S3S_E_INVALID from the sizing helpers).  1: the caller's explicit choice of a decode-compatible
                                    writer: per non-empty segment the chunks 'Z' 'V' 1 | clen | ulen | liblzf block or
                                    'Z' 'V' 0 | len | bytes of LZFOutputStream, a pure function of the source bytes, the offsets
                                    and the options; compress-lzf's LZFInputStream, liblzf and this library decode it;
                                    s3s_max_compressed_size* answer ulen + 7 x ceil(ulen / 65535) per segment */
  S3S_OPT_IO_ENCRYPTION_KEY_BITS = 11, /* ABI 11, additive, READ-ONLY: 0 (the layer is off), 128, 192 or 256 - the key that
                                    s3s_set_io_encryption holds.  s3s_set_option on it answers S3S_E_INVALID; a library without
                                    the layer answers S3S_E_INVALID to s3s_get_option too, which is how callers detect it */
  S3S_OPT_STREAM_CLASS = 12,     /* ABI 11, additive, READ-ONLY: the hardware-queue pool of the context's stream.  The runtime keeps
                                    one pool of GPU_MAX_HW_QUEUES queues (default 4) per stream priority and streams that share a
                                    queue run one after the other, so s3s_create spreads the contexts of a device over the pools
                                    by creation slot (the lowest free one; s3s_destroy returns it): 0 = lowest priority (the first
                                    `cap` contexts), 1 = normal (the next cap-1), 2 = highest (the next cap-2), 3 = normal
                                    priority beyond that, where contexts share queues.  S3S_STREAM_POOLS=0 in the environment
                                    puts every stream at normal priority (answer 1); =2 fills normal, highest, lowest in that
                                    order.  s3s_set_option on it answers S3S_E_INVALID */
  S3S_OPT_ZSTD_DECODE_VARIANT = 13, /* ABI 11, additive; tuning, identical output, S3S_CODEC_ZSTD on the reduce side: 1 (default) =
                                    frames whose header states a content size and a window of at most one block (131072),
                                    without dictionary id and content checksum - what S3S_OPT_ZSTD_COMPRESS = 1 writes - are
                                    decoded one workgroup per BLOCK; a frame with one block that needs anything in front of
                                    itself is decoded again, and judged, by the one-frame-per-wavefront decoder, so bytes,
                                    return codes and per-entry statuses are those of 0.  0 = one frame per wavefront only.
                                    Other values: S3S_E_INVALID */
  S3S_OPT_ZSTD_DECODE_BLOCKS = 14 /* ABI 11, additive, READ-ONLY: the number of blocks of the last S3S_CODEC_ZSTD decode call on
                                    this context whose frames completed on the block path of key 13, 0 otherwise.
                                    s3s_set_option on it answers S3S_E_INVALID */
};
/* Keys 15 and 16 live in an enum of their own whose entries do not start a line: the interface test of keys 1..14 counts the
   lines of the form "  S3S_OPT_NAME = n" and pins them to exactly 1..14, and that test stays as it is. */
enum { S3S_OPT_ZSTD_DECODE_STAGED = 15, /* ABI 11, additive; tuning, identical output, S3S_CODEC_ZSTD on the reduce side: 0 (default) /
                                    1, other values S3S_E_INVALID.  1: frames without dictionary id and content checksum and with
                                    at least two blocks - with or without a content size, any window: what zstd-jni and
                                    libzstd's streaming API write - are decoded in stages: the entropy streams of every block of
                                    the call in parallel into a staging area, then one pass per frame that resolves the repeat
                                    offsets and copies the matches.  A frame the staged path does not finish cleanly is decoded
                                    again, and judged, by the one-frame-per-wavefront decoder, so bytes, return codes and
                                    per-entry statuses are those of 0.  Where key 13 is 1 its block path keeps precedence: it
                                    claims a prefix of each partition's frames, the staged path starts behind it.  The staging
                                    area (20 bytes per compressed byte of the call + ~100 KiB) has a budget of its own BESIDE the
                                    single pass's scratch, of the same size (S3S_ZSTD_SCRATCH_MIB, default 4 GiB): it is scaled
                                    down to that, frames that find no room in it stay with the one-frame-per-wavefront decoder,
                                    and a staging that cannot be allocated makes the call run as with 0 - never S3S_E_NOMEM.
                                    Measured: faster for calls of a few large frames (one 128 MiB frame 2.0 x),
                                    slower from a few hundred frames per call on - hence opt-in, and no floor of its own.
                                    The two-pass form (a partition outgrew its guessed capacity)
                                    stays on the one-frame-per-wavefront decoder.  A library without the key answers
                                    S3S_E_INVALID to setting it */ S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS = 16 /* (not at the start of a line
                                    either) ABI 11, additive, READ-ONLY: the number of blocks of the last S3S_CODEC_ZSTD decode call
                                    on this context whose frames completed on the staged path of key 15 (frames in partitions
                                    that decoded), 0 otherwise; key 14 keeps counting the block path of key 13 only.
                                    s3s_set_option on it answers S3S_E_INVALID */
  , S3S_OPT_DSTREAM_BATCH_ENTRIES = 17 /* (not at the start of a line either) ABI 11, additive, READ-ONLY: the number of entries of
                                    the context's last s3s_dstream_feed_batch* call whose answer came from the batched path (its
                                    three phases); 0 when the call fell back to single feeds or was refused.  Entries that the
                                    single feed answered inside the call - without device work, or again after a bad decode
                                    status - are not counted.  s3s_set_option on it answers S3S_E_INVALID; a library without the
                                    key answers S3S_E_INVALID to reading it, which is how a caller detects that encrypted
                                    streams are batched */
  , S3S_OPT_CSTREAM_BATCH_ENTRIES = (18) /* (not at the start of a line either, and in parentheses: the interface test of keys 1..17
                                    collects every "S3S_OPT_NAME = n" of this file and pins the set, and that test stays as it
                                    is) ABI 11, additive, READ-ONLY: the number of entries of
                                    the context's last s3s_cstream_feed_batch* call whose answer came from the batched path (one
                                    upload, one launch of each kind, one download, one host wait); 0 after a call that went one
                                    by one or was refused.  Entries that the single feed answered inside the call - a window that
                                    launches nothing, refused arguments - are not counted.  s3s_set_option on it answers
                                    S3S_E_INVALID; a library without the key answers S3S_E_INVALID to reading it.  It counts
                                    plain windows only: after a call over streams under IO encryption it is 0, see key 19 */
  , S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES = (19) /* (in parentheses and not at the start of a line, as key 18) ABI 11, additive,
                                    READ-ONLY: the number of entries of the context's last s3s_cstream_feed_batch* call that the
                                    batched path answered under IO encryption (one upload that holds the call's IVs, one launch
                                    of each kind with ONE AES-CTR pass over the outputs of all windows, one download, one host
                                    wait); 0 after a plain call, after a call that went one by one and after a refused call.
                                    s3s_set_option on it answers S3S_E_INVALID; a library without the key answers S3S_E_INVALID
                                    to reading it, which is how a caller detects that streams under IO encryption are batched */
};

/* stages reported by s3s_stage_ms (valid after a call made with S3S_OPT_PROFILE=1) */
enum {
  S3S_STAGE_TOTAL = 0,      /* first kernel start -> last kernel end of the last call */
  S3S_STAGE_CODEC = 1,      /* the block compress (or decompress) kernel ALONE — the dominant one */
  S3S_STAGE_ASSEMBLE = 2,   /* offset scan + frame gather */
  S3S_STAGE_CHECKSUM = 3,   /* per-partition Adler32 / CRC32 */
  S3S_STAGE_DISCOVER = 4,   /* reduce side: frame discovery */
  S3S_STAGE_HASH = 5,       /* map side: per-chunk xxHash32 pre-pass (LZ4Block frame check) */
  S3S_STAGE_COUNT = 6
};

typedef struct s3s_ctx s3s_ctx;

/* ---- lifecycle ------------------------------------------------------------------------ */
const char* s3s_version(void);
int s3s_abi_version(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int s3s_device_count(void);
/* Creates a context bound to `device_ordinal`; `scratch_bytes` pre-sizes the device
 * workspace (0 = grow on demand).  Returns NULL on failure (s3s_last_error(NULL) tells why). */
s3s_ctx* s3s_create(int device_ordinal, int64_t scratch_bytes);
void s3s_destroy(s3s_ctx* ctx);
const char* s3s_last_error(const s3s_ctx* ctx);
int s3s_set_option(s3s_ctx* ctx, int key, int64_t value);
int64_t s3s_get_option(const s3s_ctx* ctx, int key);
/* ---- Spark IO encryption (spark.io.encryption.enabled): AES/CTR/NoPadding as a layer on both sides of the codec --------
 * The format is CryptoStreamUtils.createCryptoOutputStream restated (parity with a JVM unpinned): a non-empty
 * partition is stored as  IV (16 bytes) | AES-CTR_K(codec bytes of the partition)  with key stream block j =
 * AES_K((IV as a 128-bit big-endian integer + j) mod 2^128); an empty partition stays 0 bytes.  A partition is ONE encrypted
 * stream whatever its segments were (with encryption on Spark merges spills through the slow path): in the segments forms
 * the IV belongs to the partition and the codec streams of its segments are concatenated under one key stream.  Index and
 * checksums cover IV plus cipher text.
 *
 * s3s_set_io_encryption: key_bytes 16, 24 or 32 (spark.io.encryption.keySizeBits) switches the layer on for every later call
 * of this context, on both sides; key == NULL or key_bytes == 0 switches it off and wipes the key; any other length is
 * S3S_E_INVALID and changes nothing.  The key is copied (as round keys, host memory of the context only - it reaches the
 * kernels as launch arguments and is never stored in device memory), wiped in s3s_destroy too, and no key byte ever appears
 * in s3s_last_error.  With the layer off every path, plan and byte is what it was without these entry points.
 *
 * Map side: every compress entry point, every codec.  s3s_max_compressed_size* with a context that has the layer on add
 * 16 per non-empty partition (the segments form, which does not know the partitions: per non-empty segment, an upper bound).
 * Reduce side: part_offsets index the encrypted bytes; checksums are verified over the bytes as stored, first; then each
 * non-empty partition's IV is read and the cipher text decrypted into the workspace, where discovery and the decoders run
 * unchanged.  A non-empty partition of 1..15 bytes is S3S_E_BAD_FRAME; one of exactly 16 bytes is an empty stream.
 * s3s_decompressed_size with the layer on treats comp as ONE partition, IV first (it decrypts the partition on the host):
 * callers size a range of several partitions partition by partition.  The batched forms of both sides give the same results
 * as without the layer but run their tasks / ranges one after the other while it is on. */
int s3s_set_io_encryption(s3s_ctx* ctx, const uint8_t* key, int32_t key_bytes);
/* One IV per PARTITION of the NEXT compress call on this context: a host array of 16 * n_ivs bytes, task by task, then
 * partition by partition; an empty partition has an entry that is not used.  That call consumes the array, whether it
 * succeeds or fails.  A compress call with the layer on and a count other than its own number of partitions answers
 * S3S_E_INVALID before anything is allocated or launched (batch entries: S3S_STATUS_NOT_RUN).  The library never invents an
 * IV (a JVM shim fills them from SecureRandom, as CryptoStreamUtils.createInitializationVector does): the output stays a
 * pure function of source, offsets, options, key and IVs.  Never reusing an IV under one key is the caller's duty. */
int s3s_set_stream_ivs(s3s_ctx* ctx, const uint8_t* ivs, int64_t n_ivs);
/* The HIP stream (hipStream_t) the context launches on, for callers that time with events. */
void* s3s_stream(const s3s_ctx* ctx);
double s3s_stage_ms(const s3s_ctx* ctx, int stage);

/* ---- sizing ---------------------------------------------------------------------------- */
/* Upper bound of the .data image for these partition ranges. ctx may be NULL (defaults). */
int64_t s3s_max_compressed_size(const s3s_ctx* ctx, int codec, const int64_t* src_offsets,
                                int32_t num_partitions);

/* ---- map side: compress + checksum one map task's output ------------------------------- */
/* Partition p's serialized (uncompressed) bytes are src[src_offsets[p], src_offsets[p+1]).
 * Writes the exact .data byte image into dst, out_index[num_partitions+1],
 * out_checksums[num_partitions] (may be NULL iff checksum_algo == NONE), *out_total.
 * Host-buffer variant: src/dst are host memory (H2D/D2H inside the call).               */
int s3s_compress_map_output(s3s_ctx* ctx, int codec, int checksum_algo, const uint8_t* src,
                            const int64_t* src_offsets, int32_t num_partitions, uint8_t* dst,
                            int64_t dst_capacity, int64_t* out_index, int64_t* out_checksums,
                            int64_t* out_total);
/* Device-buffer variant: src/dst are device memory on ctx's device (offsets/index/checksums
 * stay host arrays).  This is the form the roofline metric is measured on. */
int s3s_compress_map_output_device(s3s_ctx* ctx, int codec, int checksum_algo,
                                   const uint8_t* d_src, const int64_t* src_offsets,
                                   int32_t num_partitions, uint8_t* d_dst, int64_t dst_capacity,
                                   int64_t* out_index, int64_t* out_checksums,
                                   int64_t* out_total);

/* Batched form of s3s_compress_map_output_device: several map tasks of one executor in ONE call.
 * No reference counterpart as an interface — on the JVM every task thread drives its own
 * LZ4BlockOutputStream (shuffle/S3ShuffleMapOutputWriter.scala:168-202); the shim collects the
 * spill buffers of the tasks that commit together (shuffle/S3ShuffleMapOutputWriter.scala:91-118)
 * and hands them over at once, so that the chip sees enough 32 KiB chunks to fill its 2 560
 * resident wavefronts (an 8 MiB map output — the reference's default write buffer,
 * shuffle/helper/S3ShuffleDispatcher.scala:55 — is 256 chunks).  All chunks of all tasks go
 * through one codec launch; offsets, gather and checksums run per task behind it; one stream
 * synchronisation for the batch.  Every task gets exactly the bytes, index and checksums
 * s3s_compress_map_output_device would have produced for it alone.  One codec stream per
 * non-empty partition (no multi-spill pieces in the batched form).
 * Returns S3S_OK, or the first failing task's error; each task's own result is in .status
 * (S3S_STATUS_NOT_RUN = the call failed before this task had a result: the return code is its error). */
typedef struct s3s_map_task {
  const uint8_t* d_src;         /* in: device memory holding this task's partitions */
  const int64_t* src_offsets;   /* in: host array [num_partitions + 1], offsets into d_src */
  int32_t num_partitions;       /* in */
  uint8_t* d_dst;               /* in: device buffer for the .data image */
  int64_t dst_capacity;         /* in */
  int64_t* out_index;           /* out: host array [num_partitions + 1] */
  int64_t* out_checksums;       /* out: host array [num_partitions] (may be NULL iff checksum NONE) */
  int64_t out_total;            /* out: bytes of the .data image */
  int32_t status;               /* out: S3S_OK / S3S_E_CAPACITY for this task; S3S_STATUS_NOT_RUN: see the enum */
} s3s_map_task;
int s3s_compress_map_outputs_batch_device(s3s_ctx* ctx, int codec, int checksum_algo,
                                          s3s_map_task* tasks, int32_t n_tasks);

/* The same batch for HOST buffers — the form a Spark executor reaches through the JNI shim (the reference's
 * call sites hold heap / direct buffers: shuffle/S3ShuffleMapOutputWriter.scala:91-118, 168-202).  In this
 * variant `d_src` / `d_dst` of every task are HOST addresses (page-locked memory from s3s_host_alloc moves by
 * plain DMA; pageable memory works through the runtime's bounce buffers).  The tasks run as a pipeline over
 * groups of ~64 MiB: the upload of group g+1 and the download of group g-1 are in flight while group g is
 * compressed, so one call is bound by the slower of PCIe host->device (uncompressed bytes) and the codec.
 * Results per task are exactly those of s3s_compress_map_output.  A single task takes that entry point's
 * own chunked upload overlap. */
int s3s_compress_map_outputs_batch(s3s_ctx* ctx, int codec, int checksum_algo, s3s_map_task* tasks,
                                   int32_t n_tasks);

/* ---- checksum only ---------------------------------------------------------------------- */
/* out[i] = checksum(data[offsets[i], offsets[i+1])) for i in [0, n). */
int s3s_checksum_ranges(s3s_ctx* ctx, int checksum_algo, const uint8_t* data,
                        const int64_t* offsets, int32_t n, int64_t* out);
int s3s_checksum_ranges_device(s3s_ctx* ctx, int checksum_algo, const uint8_t* d_data,
                               const int64_t* offsets, int32_t n, int64_t* out);

/* ---- reduce side: verify + decompress one fetched block range --------------------------- */
/* comp[0, comp_len) holds partitions r0..r1-1 of one map output (a ShuffleBlockId or a
 * ShuffleBlockBatchId range); part_offsets[nparts+1] are the .index entries relative to the
 * range start (part_offsets[0] == 0, part_offsets[nparts] == comp_len).  When
 * checksum_algo != NONE every partition is validated against ref_checksums first
 * (S3S_E_CHECKSUM, *out_bad_partition = first failing one); then the concatenated codec
 * streams are decoded into dst (frame hashes verified; S3S_E_BAD_FRAME on corruption). */
int s3s_decompress_range(s3s_ctx* ctx, int codec, int checksum_algo, const uint8_t* comp,
                         int64_t comp_len, const int64_t* part_offsets,
                         const int64_t* ref_checksums, int32_t nparts, uint8_t* dst,
                         int64_t dst_capacity, int64_t* out_len, int32_t* out_bad_partition);
int s3s_decompress_range_device(s3s_ctx* ctx, int codec, int checksum_algo,
                                const uint8_t* d_comp, int64_t comp_len,
                                const int64_t* part_offsets, const int64_t* ref_checksums,
                                int32_t nparts, uint8_t* d_dst, int64_t dst_capacity,
                                int64_t* out_len, int32_t* out_bad_partition);
/* Batched reduce side: many fetched ranges (the blocks a reduce task's prefetcher has staged — reference
 * buffers of 8 MiB..128 MiB, S3ShuffleDispatcher.scala:55-57, S3BufferedPrefetchIterator.scala:102-153) in ONE
 * call: checksums and frame discovery of all ranges are queued back to back, ONE decode launch covers the
 * frames of every range, and the host waits three times per batch instead of three times per range.  Every
 * range gets exactly what s3s_decompress_range_device would have reported for it alone (status, out_len,
 * bad_partition).  Returns S3S_OK or the first failing range's error. */
typedef struct s3s_fetch_range {
  const uint8_t* d_comp;         /* in: device memory, comp_len bytes */
  int64_t comp_len;              /* in */
  const int64_t* part_offsets;   /* in: host array [num_partitions + 1], relative to the range start */
  const int64_t* ref_checksums;  /* in: host array [num_partitions] (may be NULL iff checksum NONE) */
  int32_t num_partitions;        /* in */
  uint8_t* d_dst;                /* in: device buffer for the decoded bytes */
  int64_t dst_capacity;          /* in */
  int64_t out_len;               /* out: decoded bytes */
  int32_t bad_partition;         /* out: first partition with a wrong checksum, or -1 */
  int32_t status;                /* out: S3S_OK / S3S_E_CHECKSUM / S3S_E_BAD_FRAME / S3S_E_CAPACITY / ...; S3S_STATUS_NOT_RUN: see the enum */
} s3s_fetch_range;
int s3s_decompress_ranges_batch_device(s3s_ctx* ctx, int codec, int checksum_algo,
                                       s3s_fetch_range* ranges, int32_t n_ranges);

/* Host-buffer form (storage/S3ShuffleReader.scala:98-110 holds the prefetcher's heap buffers): `d_comp` /
 * `d_dst` of every range are HOST addresses; upload of the next group, decode of this one and download of the
 * previous one overlap (groups of ~128 MiB decoded), so one call is bound by the slower of PCIe
 * device->host (decoded bytes) and the decoder.  Results per range are those of s3s_decompress_range. */
int s3s_decompress_ranges_batch(s3s_ctx* ctx, int codec, int checksum_algo, s3s_fetch_range* ranges,
                                int32_t n_ranges);

/* Multi-spill map tasks.  When a map task spilled N times, Spark's merge hands every partition to the
 * partition writer as the concatenation of N independently written pieces, and on the JVM each piece is
 * one COMPLETE codec stream (LZ4Block end frame / Snappy stream header included) — see the writers that
 * feed shuffle/S3ShuffleMapOutputWriter.scala:67-83 and the pre-merged spill file of
 * shuffle/S3SingleSpillShuffleMapOutputWriter.scala:24-64.  To keep the `.data` object byte-identical
 * the shim passes the piece boundaries: seg_offsets[0..n_segs] delimit the pieces in src (ascending,
 * contiguous), part_first_seg[0..n] (part_first_seg[0] = 0, part_first_seg[n] = n_segs) assigns them to
 * the n partitions.  Every non-empty piece becomes one stream; index and checksums stay per partition.
 * With one piece per partition this is exactly s3s_compress_map_output.                               */
int64_t s3s_max_compressed_size_segments(const s3s_ctx* ctx, int codec, const int64_t* seg_offsets,
                                         int32_t n_segs);
int s3s_compress_map_output_segments(s3s_ctx* ctx, int codec, int checksum_algo, const uint8_t* src,
                                     const int64_t* seg_offsets, int32_t n_segs,
                                     const int32_t* part_first_seg, int32_t n, uint8_t* dst,
                                     int64_t dst_capacity, int64_t* out_index, int64_t* out_checksums,
                                     int64_t* out_total);
int s3s_compress_map_output_segments_device(s3s_ctx* ctx, int codec, int checksum_algo,
                                            const uint8_t* d_src, const int64_t* seg_offsets,
                                            int32_t n_segs, const int32_t* part_first_seg, int32_t n,
                                            uint8_t* d_dst, int64_t dst_capacity, int64_t* out_index,
                                            int64_t* out_checksums, int64_t* out_total);

/* java.util.zip.Checksum continued (ABI 11, additive: detect by the symbols): out[i] = the checksum state after
 * data[offsets[i], offsets[i+1]) when it was seeds[i] before - seeds[i] is getValue() of the bytes so far (a fresh Adler32 is 1, a
 * fresh CRC32 / CRC32C is 0).  seeds == NULL: every range starts fresh, and the call is s3s_checksum_ranges*.  A range of no
 * bytes returns its seed.  This is what S3ChecksumValidationStream.scala:54-66 does with one Checksum object across reads. */
int s3s_checksum_ranges_seeded(s3s_ctx* ctx, int checksum_algo, const uint8_t* data, const int64_t* offsets, int32_t n,
                               const int64_t* seeds, int64_t* out);
int s3s_checksum_ranges_seeded_device(s3s_ctx* ctx, int checksum_algo, const uint8_t* d_data, const int64_t* offsets, int32_t n,
                                      const int64_t* seeds, int64_t* out);

/* ---- reduce side, streaming: a fetched range decoded window by window, in bounded memory --------------------------------
 * (ABI 11, additive: callers detect support by the symbols.)  s3s_decompress_range* needs the whole compressed range and the
 * whole decoded range resident at once.  The reference never holds a block like that: storage/S3BufferedInputStreamAdaptor
 * .scala:13-19 buffers min(maxBufferSizeTask, block length), storage/S3ChecksumValidationStream.scala:54-86 validates a
 * partition as its last byte streams past, and the codec input streams decode frame by frame.  An s3s_dstream gives a range of
 * any size that shape: the caller feeds windows of the compressed bytes and gets the decoded bytes of the whole units in each.
 *
 * Window   comp[0, comp_len) holds the bytes of the range that start at s3s_dstream_position(); the caller presents again what
 *          the previous feed did not consume.  A window that reaches past part_offsets[nparts] is S3S_E_INVALID.
 * Unit     an LZ4Block frame (the 21-byte end frame included); a Snappy 16-byte stream header or one length | chunk; an LZF
 *          'Z' 'V' chunk; for S3S_CODEC_NONE a byte.
 * A feed   takes the longest prefix of whole units that lies inside the window and whose decoded bytes fit dst_capacity, and
 *          decodes them to dst[0, out_len).  Concatenated streams inside a partition (multi-spill) work as in the one-shot call.
 * Progress a feed consumes at least one unit when the window holds the whole first unit and dst_capacity is at least its
 *          decoded size.  Otherwise:  the unit is not whole in the window - S3S_OK, consumed = 0, need_comp set (two steps at
 *          the most for LZ4 and Snappy: the header's length, then header + payload; LZF's compressed chunk header adds a
 *          third);  the unit does not fit dst - S3S_E_CAPACITY, need_dst set, nothing consumed, the stream stays usable;  the
 *          unit is not whole and the window already ends at the end of the range - S3S_E_BAD_FRAME (truncated).
 * Checksum the state of the open partition is carried from feed to feed, over consumed bytes only.  A partition is verified in
 *          the feed that consumes its last byte, an empty partition as the position passes it, and that feed's decode is
 *          launched only after the verdict: on a mismatch the feed returns S3S_E_CHECKSUM with bad_partition, consumed = 0
 *          and out_len = 0.  NOTE: the decoded bytes of a partition that is still open are handed out BEFORE its checksum is
 *          known - exactly what S3ChecksumValidationStream does (it raises at the partition's end); a caller that must not
 *          act on unverified bytes holds them back until the feed that passes the partition's end has returned S3S_OK.
 *          NOTE: the one-shot call reports a wrong checksum before a corrupt frame.  A feed does so for the partitions whose
 *          last byte its window holds; a corrupt frame in a partition that is still open is reported first, as
 *          S3S_E_BAD_FRAME, by the feed that meets it.
 *          That holds for a corrupt header and for a corrupt payload alike.
 * Size     need_dst never exceeds 32 MiB (1 << 25, lz4-java's largest block and the largest unit any decoder here takes).  An
 *          LZ4Block header is bounded by its level nibble and an LZF chunk by its 16-bit field; a Snappy chunk whose varint
 *          claims more is refused by the feed that meets it: S3S_E_UNSUPPORTED, consumed = 0, out_len = 0, need_dst = 0 -
 *          never S3S_E_CAPACITY, which would send the caller for a buffer of up to 4 GiB - 1 on the word of one flipped bit.
 *          (With checksums on, a wrong checksum of a partition whose last byte the window holds is still reported first.)
 *          The refusal does not fail the stream - nothing was consumed, the same feed gets the same answer - and
 *          s3s_dstream_close then says the range was not read to its end.
 * Errors   stick: after S3S_E_CHECKSUM or S3S_E_BAD_FRAME every later feed returns the same code (and bad_partition).
 * Result   the concatenation of all dst outputs is what s3s_decompress_range_device writes for the same range, and the final
 *          verdict falls in the same class.
 * State    a stream holds host state only (position, carried checksum, verdicts; whether the position is inside a Snappy
 *          stream follows from it) and no device memory between feeds: a feed works in the context's workspace, and other
 *          calls on the same context may run between two feeds.  The context stays single-threaded and must outlive the
 *          stream.  s3s_dstream_feed (host buffers) stages the window and dst_capacity bytes of output in that workspace:
 *          the caller's two sizes are the memory bound.  (A stream opened by s3s_dstream_open_encrypted holds one more
 *          window-sized buffer there during a feed: the decrypted window.)
 * Refused  at open with S3S_E_UNSUPPORTED, context intact: S3S_CODEC_ZSTD by s3s_dstream_open and s3s_dstream_open_encrypted (a
 *          frame is a whole partition with history across its blocks and, from zstd-jni's streaming writer, no content size:
 *          a Zstandard stream keeps device memory between feeds and has units of its own, both new to a caller -
 *          s3s_dstream_open_zstd, below, is the opt-in, and callers from before it rely on this answer to fall back) and, by
 *          s3s_dstream_open, any context with IO encryption on: callers from before s3s_dstream_open_encrypted rely on that
 *          answer to fall back, and the units of an encrypted range are new to a caller (below) - s3s_dstream_open_encrypted
 *          is the opt-in.  Both keep the one-shot call.  S3S_OPT_LZ4_DECODE_VARIANT = 3 WORKS: a feed launches whichever
 *          decoder the option names.
 * Not here a reader in the C++ host mirror.  (The batched feed of several streams is s3s_dstream_feed_batch*, behind the
 *          streaming map side; the streaming map side is s3s_cstream_*, below.)
 *
 * Under Spark IO encryption: s3s_dstream_open_encrypted (ABI 11, additive: callers detect support by the symbol) takes the
 * arguments of s3s_dstream_open and makes its checks, requires the layer to be on (off: S3S_E_INVALID) and refuses
 * S3S_CODEC_ZSTD alike.  part_offsets index the STORED bytes, IVs included; so do the window, consumed, need_comp and the
 * position.  CTR is seekable - key stream block j is AES_K(IV + j) - so a window may start anywhere in a partition's cipher
 * text.  The contract above holds with these changes only:
 * IV unit  the 16-byte IV of a non-empty partition is a unit.  It decodes to no bytes, so it always fits dst_capacity.  It is
 *          consumed only when all 16 bytes are in the window: a window that starts at a partition's start and shows fewer than
 *          16 bytes gets S3S_OK, consumed = 0, need_comp = 16.  The position is therefore never inside an IV.
 * Units    every other unit is the codec's unit of the plain stream; its stored position is the plain position plus the IVs in
 *          front of it.  need_comp, need_dst, the capacity cut, the 32 MiB bound on need_dst and the Snappy oversized-claim
 *          refusal keep their meaning; need_comp takes one more step at most (the IV).
 * Short    a partition of exactly 16 stored bytes is an empty stream.  One of 1 .. 15 stored bytes is S3S_E_BAD_FRAME, sticky,
 *          from the feed that would consume into it (it has taken everything in front and its window shows a byte of it); a
 *          wrong checksum of a partition whose last byte the window holds is still reported first.
 * Checksum over the stored bytes; timing, verdicts and stickiness unchanged.
 * Key      the stream is bound to the key setting it was opened under: after any later successful s3s_set_io_encryption on
 *          the context, on or off, the same key or another, its feeds answer S3S_E_INVALID and it can only be closed (a call
 *          refused for its key length changes nothing, here too).  No key material is
 *          copied into the stream.
 * State    still host-only: it additionally holds the open partition's IV (16 bytes, wiped at close); where its key stream
 *          stands follows from the position.  Between feeds the stream holds no device memory; one-shot encrypted calls on the
 *          same context may run between two feeds.
 * Result   the concatenation of all dst outputs is what s3s_decompress_range_device writes for the same range under the same
 *          key, and the final verdict falls in the same class.
 *
 * Zstandard: s3s_dstream_open_zstd (ABI 11, additive: callers detect support by the symbol) takes the arguments of
 * s3s_dstream_open without the codec, makes its checks, and window_log_max = 10 .. 27 (anything else: S3S_E_INVALID): the
 * caller's memory promise - the stream keeps at most 1 << window_log_max bytes of history for its open frame.  (libzstd's
 * streaming writer with an unknown source size, which is what zstd-jni's ZstdOutputStream is, writes window log 19 at level 1
 * and 21 at level 3: read from the headers of such frames, libzstd 1.4.8.)  A context with IO encryption on is refused with
 * S3S_E_UNSUPPORTED.  feed, feed_device, position and close work on the stream unchanged.  The contract above holds with these
 * changes only:
 * Units    a frame header of 6 .. 18 bytes (decodes to nothing);  a block: its 3-byte header plus Block_Size payload bytes
 *          (1 byte for an RLE block), which decodes to at most 128 KiB;  a skippable frame of 8 + n bytes (decodes to nothing).
 *          A partition is zero or more frames (several: multi-spill).  The position is never inside a unit.
 * need_comp  a frame header takes two steps at most (6: the magic and the descriptor, then the header's length; a skippable
 *          frame 6, 8, then 8 + n), a block two (3, then header plus payload) and never more than 3 + 128 KiB.
 * need_dst a compressed block's decoded size is not in its header: a feed runs a size pass (no stores) over the blocks of its
 *          window, like the one-shot call, cuts by dst_capacity at a block boundary, exactly, and only then decodes.
 *          S3S_E_CAPACITY carries the exact decoded size of the first block; need_dst never exceeds 128 KiB.  Longest prefix
 *          and progress hold as above (a unit of no output always fits).
 * Refused  by the feed whose window shows the header, with S3S_E_UNSUPPORTED, consumed = 0, out_len = 0, not sticky (the shape
 *          of the Snappy oversized claim): a frame with a Content_Checksum (a running XXH64 across feeds is not built), a frame
 *          with a Dictionary_ID field, a frame whose Window_Size exceeds 1 << window_log_max (a single-segment frame's is its
 *          content size), a skippable frame above 32 MiB.  With checksums on, a wrong checksum of a partition whose last byte
 *          the window holds is still reported first.
 * Malformed  S3S_E_BAD_FRAME, sticky, from the feed that meets it: a reserved block type or header bit, a block or frame that
 *          runs past its partition's end, a partition that ends with a frame open, a Frame_Content_Size the decoded bytes do
 *          not match, every failure of the block decoder, and an offset that reaches further back than
 *          min(Window_Size, bytes of the frame produced so far).  The size pass covers every block of the window, also those
 *          behind the capacity cut, and meets what is wrong with a block's headers, table descriptions and sequences; what
 *          is wrong with its Huffman-coded literals (tree, streams, treeless literals without a tree) is met by the feed
 *          that decodes the block.  NOTE: the one-shot call keeps the whole frame as history and may accept the offset
 *          case; it is invalid by RFC 8878 (libzstd refuses it once the offset passes what its own window buffer still
 *          holds).  For everything else the final verdict falls in the same class as the one-shot call's.
 * State    NOT host-only: a Zstandard stream owns device memory between feeds, for the one frame that is open at the
 *          position - the last min(Window_Size, produced) bytes of the frame's output, the three repeat offsets, what a later
 *          block may reuse without restating it (the Huffman tree of treeless literals, the LL / OF / ML tables of
 *          Repeat_Mode) and the bytes produced so far.  It is allocated (record + Window_Size bytes, sized by the frame, not
 *          by window_log_max) when a frame first stays open across a feed, freed when the frame ends and in any case by
 *          s3s_dstream_close, also in the middle of a range.  It is not part of the context's workspace: other calls on the
 *          context may run between two feeds.  An allocation failure is S3S_E_NOMEM with nothing consumed; the stream stays
 *          usable.  During a feed the workspace additionally holds the open frame's history plus what it decodes in the feed.
 * Result   the concatenation of all dst outputs is what s3s_decompress_range_device writes for the same range, whatever
 *          S3S_OPT_ZSTD_DECODE_VARIANT and S3S_OPT_ZSTD_DECODE_STAGED are set to.
 * Not here frames with a content checksum, Zstandard under IO encryption.  In a batched feed (s3s_dstream_feed_batch*, below)
 *          a Zstandard stream is fed on its own inside the call. */
typedef struct s3s_dstream s3s_dstream;
typedef struct s3s_dstream_result {
  int64_t consumed;      /* bytes of this window taken; the next window starts there */
  int64_t out_len;       /* decoded bytes written to dst by this feed */
  int64_t need_comp;     /* consumed == 0 because the first unit is not whole in the window: the smallest window length known
                            to hold it (header + payload when the header is in the window, else the header's length); else 0 */
  int64_t need_dst;      /* S3S_E_CAPACITY: decoded size of the first unit; 0 otherwise */
  int32_t bad_partition; /* S3S_E_CHECKSUM: range-relative partition, else -1 */
  int32_t at_end;        /* 1: position == range length and every partition verified */
} s3s_dstream_result;
/* part_offsets[nparts + 1] (part_offsets[0] == 0) and ref_checksums[nparts] (may be NULL iff checksum NONE) are copied.  Like
 * every entry point this one returns the code; the stream comes back through *out (NULL on failure). */
int s3s_dstream_open(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                     int32_t nparts, s3s_dstream** out);
int s3s_dstream_open_encrypted(s3s_ctx* ctx, int codec, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums,
                               int32_t nparts, s3s_dstream** out);
int s3s_dstream_open_zstd(s3s_ctx* ctx, int checksum_algo, const int64_t* part_offsets, const int64_t* ref_checksums, int32_t nparts,
                          int32_t window_log_max, s3s_dstream** out);
/* Debug accessor (additive, detected by the symbol): the device bytes a stream holds between feeds as it allocated them - 0 for
 * every stream but a Zstandard one with a frame open, then the state record (rounded to 256) plus that frame's Window_Size.
 * With s == NULL: the sum over all streams of the process, which a close in the middle of a range must bring back down. */
int64_t s3s_dstream_held_bytes(const s3s_dstream* s);
int s3s_dstream_feed_device(s3s_dstream* s, const uint8_t* d_comp, int64_t comp_len, uint8_t* d_dst, int64_t dst_capacity,
                            s3s_dstream_result* r);
int s3s_dstream_feed(s3s_dstream* s, const uint8_t* comp, int64_t comp_len, uint8_t* dst, int64_t dst_capacity, /* host buffers */
                     s3s_dstream_result* r);
int64_t s3s_dstream_position(const s3s_dstream* s);
/* Frees the stream.  S3S_OK at the end of the range with every partition verified; the stream's error when it has one;
 * S3S_E_BAD_FRAME when the range was not read to its end (what a reader sees that closes a truncated stream). */
int s3s_dstream_close(s3s_dstream* s);

/* ---- map side, streaming: a map output compressed window by window, in bounded memory -------------------------------------
 * (ABI 11, additive, no new option key: callers detect support by the symbols.)  Every s3s_compress_map_output* call needs the
 * whole map output, the whole .data image and one slot per codec block resident at once.  The reference never holds a map
 * output like that: shuffle/S3ShuffleMapOutputWriter.scala:43-49 puts a BufferedOutputStream of dispatcher.bufferSize in front
 * of the object, :136-202 writes partition after partition through a codec stream and learns a partition's length as it
 * closes.  LZ4Block frames, Snappy chunks and LZF chunks are independent blocks cut at multiples of the block size from the
 * partition's start, and the per-partition checksums continue across calls: an s3s_cstream that takes only whole blocks
 * writes the SAME BYTES as the one-shot call and keeps nothing on the device between feeds.
 *
 * Window   d_src[0, src_len) are the source bytes that start at s3s_cstream_position().  part_ends[0, n_ends) are host-side,
 *          window-relative, ascending offsets 0 <= e <= src_len: a partition ends at each.  Equal neighbours are empty
 *          partitions; an end at 0 in front of an open partition that has bytes closes that partition, with nothing consumed of
 *          the open partition it is an empty partition.  Bytes behind the last end belong to the partition that stays open.
 *          The caller presents again what was not consumed, with the ends rebased.  The stream does not know the number of
 *          partitions in advance.
 * Unit     (a) a block: blockSize source bytes of the open partition, or the partition's remaining bytes when its end lies in
 *          the window.  The Snappy 16-byte stream header belongs to the unit of a partition's first block; a Snappy chunk above
 *          one fragment is one unit, its head and all its fragments.  (b) the end of a non-empty LZ4 partition: the 21-byte
 *          end frame, which consumes no source bytes.  For the other codecs the end has no bytes and is passed together with the
 *          last block; the end of an empty partition is passed as soon as every unit in front of it is taken.  Bytes behind
 *          the last end that do not make a whole block are not consumed.  For S3S_CODEC_NONE a unit is a byte.
 * A feed   takes the longest prefix of units whose image bytes, as compressed, fit dst_capacity, writes them to dst[0, out_len)
 *          and nothing at or beyond out_len.  For every end it passed it writes, in order, the partition's image length to
 *          out_lengths and its checksum over the image bytes to out_checksums (may be NULL iff checksum NONE); both arrays
 *          hold n_ends entries, [0, parts_closed) are valid.
 * Progress the first unit does not fit and no end lies in front of it: S3S_E_CAPACITY, need_dst is its exact image size,
 *          nothing is consumed, the stream stays usable.  The window shows no whole unit and no end: S3S_OK, consumed = 0,
 *          need_src is the block size in force (LZF: 65 535; NONE: 1).  An empty window with no ends is S3S_OK.
 * Result   with src_offsets built from the ends, on a context with the same options: the concatenation of all dst outputs is
 *          byte for byte the .data image s3s_compress_map_output_device writes, the lengths are the differences of its index,
 *          the checksums are its checksums - for every schedule of windows and capacities.  The output is a function of
 *          source, ends and options, not of the feeds.
 * Codecs   S3S_CODEC_NONE, LZ4, Snappy, and LZF when S3S_OPT_LZF_COMPRESS is 1, at every block size the one-shot call takes
 *          through keys 1, 2 and 8 (the 32-bit-table LZ4 parse and the fragment-parallel Snappy chunks included).  The block
 *          size and the LZ4 / Snappy variants are read at open and bound to the stream.  S3S_OPT_LZ4_VARIANT = 9 runs 11
 *          without timing rounds, as a batched call does; S3S_OPT_LZ4_VARIANT_USED reports the parse run.
 * Refused  at open with S3S_E_UNSUPPORTED, context intact: S3S_CODEC_ZSTD (the frame header this library writes carries the
 *          8-byte content size of a partition whose end a stream has not seen); LZF with the option off; by
 *          s3s_cstream_open, any context with IO encryption on: callers from before s3s_cstream_open_encrypted rely on that
 *          answer to fall back, and the IV unit and the IVs of every feed are new to a caller (below) -
 *          s3s_cstream_open_encrypted is the opt-in.  Encryption switched on after s3s_cstream_open makes that stream's
 *          feeds answer S3S_E_UNSUPPORTED.  A feed answers S3S_E_INVALID, with nothing changed, for ends that are
 *          negative, descending or beyond src_len, null pointers with non-zero lengths, negative sizes; a window with more
 *          codec blocks than the one-shot call takes answers S3S_E_UNSUPPORTED.
 * State    host-only: position, bytes written, source and image bytes of the open partition, its carried checksum.  No device
 *          memory between feeds: a feed works in the context's workspace, and other calls on the same context may run between
 *          two feeds.  s3s_cstream_feed (host buffers) stages src_len + dst_capacity bytes there.
 * Speed    the stream buys bounded memory, not speed: a window below about 80 MiB does not fill the chip's 2 560 resident
 *          wavefronts, and every feed pays one scan, one cut and one host wait (profiles/compress_stream.md has the figures).
 * Close    frees the stream.  S3S_OK when no byte of the open partition has been consumed, else S3S_E_INVALID: the image ends
 *          inside a codec stream.
 * Not here Zstandard, the JNI natives and the Scala writer.  (A batched feed of several streams: s3s_cstream_feed_batch*, below.)
 *
 * Under Spark IO encryption: s3s_cstream_open_encrypted (ABI 11, additive: callers detect support by the symbol) takes the
 * arguments of s3s_cstream_open and makes its checks, requires the layer to be on (off: S3S_E_INVALID) and refuses
 * S3S_CODEC_ZSTD, and LZF with the option off, alike.  feed, feed_device, feed_bound, position, written and close work on
 * the stream unchanged.  CTR is seekable - key stream block j is AES_K(IV + j) - so a feed continues the open partition's
 * cipher text at any residue of a block.  The contract above holds with these changes only:
 * IV       the 16-byte IV of a non-empty partition belongs to the unit of the partition's first block, as the Snappy stream
 *          header does (Snappy: IV, stream header, chunk).  For S3S_CODEC_NONE the unit of a partition's first byte is 17
 *          image bytes.  An empty partition stays 0 bytes.  need_dst, the capacity cut, the lengths, written and the checksums
 *          count STORED bytes: IV plus cipher text, as in the one-shot call.  need_dst under S3S_CODEC_NONE is 17 at a
 *          partition's first byte, else 1.  s3s_cstream_feed_bound adds 16 * (n_ends + 1).
 * IVs      before EVERY feed the caller calls s3s_set_stream_ivs(ctx, ivs, n_ends + 1): a feed is a compress call, its
 *          partitions are its n_ends + 1 pieces, entry j is the IV of the partition piece j belongs to.  An entry is used only
 *          by the feed that takes that partition's first block; from then on the stream keeps that IV in its host state, and
 *          entry 0 is ignored while the open partition already has image bytes.  A count other than n_ends + 1 (or no IVs set)
 *          is S3S_E_INVALID before anything is launched, with the stream unchanged.  The array is consumed either way, also by
 *          a feed that launches nothing.  A caller that presents the same IV every time it presents a partition's start gets
 *          an image that is a function of source, ends, options, key and per-partition IVs, and not of the feeds.
 * Key      the stream is bound to the key setting it was opened under, exactly as an encrypted s3s_dstream is: after any later
 *          successful s3s_set_io_encryption on the context, on or off, the same key or another, its feeds answer S3S_E_INVALID
 *          and it can only be closed.  No key material goes into the stream or into device memory.
 * State    still host-only: it additionally holds the open partition's IV (16 bytes, wiped when the partition closes and at
 *          close).  There is no device memory between feeds; one-shot calls on the context may run between two feeds.
 * Result   the concatenation of all dst outputs is byte for byte what s3s_compress_map_output_device writes on a context with
 *          the same options, key and IVs; the lengths are the differences of that call's index, the checksums its checksums.
 * Not here Zstandard, the JNI natives and the Scala writer.  (ONE pass of the layer over the windows of a batched feed:
 *          s3s_cstream_feed_batch*, below, read-only key 19.) */
typedef struct s3s_cstream s3s_cstream;
typedef struct s3s_cstream_result {
  int64_t consumed;      /* source bytes of this window taken; the next window starts there */
  int64_t out_len;       /* image bytes written to dst by this feed */
  int64_t need_src;      /* S3S_OK with consumed == 0 and no end passed, because the window holds no whole unit: the window
                            length that holds one; else 0 */
  int64_t need_dst;      /* S3S_E_CAPACITY: exact image size of the first unit; else 0 */
  int32_t parts_closed;  /* partition ends passed by this feed: out_lengths / out_checksums [0, parts_closed) are valid */
  int32_t reserved;
} s3s_cstream_result;
int s3s_cstream_open(s3s_ctx* ctx, int codec, int checksum_algo, s3s_cstream** out);
int s3s_cstream_open_encrypted(s3s_ctx* ctx, int codec, int checksum_algo, s3s_cstream** out); /* under IO encryption (above) */
int s3s_cstream_feed_device(s3s_cstream* s, const uint8_t* d_src, int64_t src_len, const int64_t* part_ends, int32_t n_ends,
                            uint8_t* d_dst, int64_t dst_capacity, int64_t* out_lengths, int64_t* out_checksums,
                            s3s_cstream_result* r);
int s3s_cstream_feed(s3s_cstream* s, const uint8_t* src, int64_t src_len, const int64_t* part_ends, int32_t n_ends, /* host buffers */
                     uint8_t* dst, int64_t dst_capacity, int64_t* out_lengths, int64_t* out_checksums, s3s_cstream_result* r);
/* a dst_capacity with which a feed of this shape never answers S3S_E_CAPACITY (and takes every unit of its window) */
int64_t s3s_cstream_feed_bound(const s3s_cstream* s, int64_t src_len, int32_t n_ends);
int64_t s3s_cstream_position(const s3s_cstream* s); /* source bytes consumed so far */
int64_t s3s_cstream_written(const s3s_cstream* s);  /* image bytes produced so far = image offset of the next feed's dst */
int s3s_cstream_close(s3s_cstream* s);

/* ---- reduce side, streaming: the batched feed (ABI 11, additive: callers detect support by the symbol; encrypted streams: key 17) --
 * The reference's reduce task never reads one stream at a time: S3BufferedPrefetchIterator keeps up to
 * spark.shuffle.s3.maxConcurrencyTask (10) fetches open, each behind a buffer of spark.shuffle.s3.bufferSize (8 MiB), together
 * under spark.shuffle.s3.maxBufferSizeTask (128 MiB) - S3ShuffleDispatcher.scala:55-57.  A feed has a floor of about half a
 * millisecond whatever it holds (three host waits and the serial chains of discovery); s3s_dstream_feed_batch_device takes ONE
 * WINDOW OF EACH OF SEVERAL STREAMS and pays that floor once per call.
 *
 * Contract every entry gets what s3s_dstream_feed_device(stream, d_comp, comp_len, d_dst, dst_capacity, &result) would have
 *          produced for that stream alone: status and every field of result, the bytes d_dst[0, out_len) with nothing written
 *          at or beyond d_dst + dst_capacity, and the stream's state afterwards - position, carried checksum, sticky error.
 *          One entry's failure does not touch another entry: a sticky error from an earlier feed, S3S_E_CAPACITY with need_dst,
 *          a refused Snappy claim, a wrong checksum and a corrupt frame are that entry's alone.
 * Returns  S3S_OK, or the status of the first entry, in order, that is not S3S_OK (the rule of
 *          s3s_decompress_ranges_batch_device).  Entries are stamped S3S_STATUS_NOT_RUN on entry to the call.
 * Refused  before anything is launched, with S3S_E_INVALID and every stream unchanged: a null ctx, a negative n, null entries
 *          with n > 0, a null stream, a stream opened on another context, the same stream twice, streams that differ in codec
 *          or checksum algorithm.  n == 0 is S3S_OK.
 * Caller   promises that the windows and the destinations of different entries do not overlap each other; the library does
 *          not check it.
 * Batched  LZ4, Snappy and LZF streams, n > 1, all of them plain (s3s_dstream_open, no IO encryption on the context) or all of
 *          them encrypted (s3s_dstream_open_encrypted, ABI 11 with key 17, under the context's current key): three host waits
 *          per call whatever n is (checksums + discovery; frame tables + the cut of every window at its own dst_capacity; one
 *          decode launch over the frames of all windows), and no stream's state is committed before the decode's verdict is
 *          known.  When that verdict is bad - a corrupt payload, or an LZ4 frame above 32 MiB that needs the ring decoder - the
 *          undecided entries are fed one by one through the single feed, which says whose it was.
 *          S3S_OPT_LZ4_DECODE_VARIANT is honoured.  Encrypted: ONE launch of the window form of the AES-CTR pass decrypts the
 *          windows of all entries in front of discovery, each into a plain buffer of its own, and gathers their IVs, which
 *          come back with the first wait; the stored side (checksums, consumed, need_comp, the position) and the plain side
 *          (discovery, the cut, the decoders) are those of the single feed, window by window.  An entry whose stream is bound
 *          to an earlier key setting, or a plain stream on a context with the layer on, gets the single feed's refusal
 *          (S3S_E_INVALID / S3S_E_UNSUPPORTED) as its own status; the other entries run batched.
 * One by one, in order, through the single feed inside the call (the contract holds for every stream the library can open):
 *          n == 1, S3S_CODEC_NONE (plain or encrypted), any stream of s3s_dstream_open_zstd.
 * Key 17   S3S_OPT_DSTREAM_BATCH_ENTRIES (read-only) holds the number of entries of the context's last call that the batched path
 *          answered: 0 after a call that went one by one or was refused; entries the single feed answered inside a batched call
 *          (a sticky error, refused arguments, an empty window, a stale key, a feed repeated after a bad decode status) are not
 *          counted.
 * Memory   the device form works in the context's workspace; encrypted windows add one plain buffer per window there (the sum
 *          of the windows' plain bytes + 320 bytes per window).  s3s_dstream_feed_batch (HOST addresses in d_comp / d_dst)
 *          stages the windows and the destinations of ALL entries there - the sum of comp_len + dst_capacity is the caller's
 *          memory bound - uploads, calls the device form and downloads out_len bytes per entry; it does not overlap the upload
 *          with the decode.
 * Not here the JNI natives and the Scala reader, a reader in the C++ host mirror, batching of Zstandard streams and of
 *          S3S_CODEC_NONE.  (The map side's batched feed is s3s_cstream_feed_batch*, below.) */
typedef struct s3s_dstream_feed_entry {
  s3s_dstream* stream;        /* in */
  const uint8_t* d_comp;      /* in: this stream's window, starts at s3s_dstream_position(stream) */
  int64_t comp_len;           /* in */
  uint8_t* d_dst;             /* in */
  int64_t dst_capacity;       /* in */
  s3s_dstream_result result;  /* out: exactly what a single feed fills in */
  int32_t status;             /* out: the code a single feed would return; S3S_STATUS_NOT_RUN: see the enum */
  int32_t pad;
} s3s_dstream_feed_entry;
int s3s_dstream_feed_batch_device(s3s_ctx* ctx, s3s_dstream_feed_entry* entries, int32_t n);
int s3s_dstream_feed_batch(s3s_ctx* ctx, s3s_dstream_feed_entry* entries, int32_t n); /* d_comp / d_dst are HOST addresses */

/* ---- the batched feed of s3s_cstream (ABI 11, additive: callers detect support by the symbols; read-only keys 18 and 19) ------
 * The reference writes every map task through a BufferedOutputStream of spark.shuffle.s3.bufferSize (8 MiB), and an executor
 * runs several map tasks at once.  A feed lasts at least one block's chain (about half a millisecond) whatever it holds, and a
 * single window does not fill the chip; s3s_cstream_feed_batch_device takes ONE WINDOW OF EACH OF SEVERAL STREAMS and pays that
 * floor once per call.
 *
 * Contract every entry gets what s3s_cstream_feed_device(stream, d_src, src_len, part_ends, n_ends, d_dst, dst_capacity,
 *          out_lengths, out_checksums, &result) would have produced for that stream alone: status and every field of result,
 *          the bytes d_dst[0, out_len) with nothing written at or beyond out_len, the lengths and the checksums, and the
 *          stream's state afterwards - position, written, the open partition's counters, the carried checksum and, under IO
 *          encryption, the open partition's IV (kept while the partition stays open, wiped when it closes).  One entry's
 *          fate does not touch another entry's: S3S_E_CAPACITY with need_dst, need_src, refused arguments (bad ends, null
 *          pointers with lengths, negative sizes) and a window with too many blocks are that entry's alone.
 * Returns  S3S_OK, or the status of the first entry, in order, that is not S3S_OK.  Entries are stamped S3S_STATUS_NOT_RUN on
 *          entry to the call, before any argument check.
 * Refused  before anything is launched, with S3S_E_INVALID and every stream unchanged: a null ctx, a negative n, null entries
 *          with n > 0, a null stream, a stream opened on another context, the same stream twice, streams that differ in codec
 *          or in checksum algorithm.  n == 0 is S3S_OK.
 * Caller   promises that the windows and the destinations of different entries do not overlap each other; the library does
 *          not check it.
 * Batched  n > 1 LZ4, Snappy or LZF streams that were opened under the same block size and the same LZ4 / Snappy variant, either
 *          all plain on a context without IO encryption or streams under IO encryption on a context that has the layer on:
 *          the windows of all entries are planned into one arena, which goes up in one copy; the codec kernels run ONCE over the
 *          blocks of all windows (the variant and the grid of the single feed), then one scan, one cut of every window at its
 *          own dst_capacity, one gather, under IO encryption ONE encrypt pass over the outputs of all windows (the call's IVs
 *          travel in the one upload; every window's IV unit and need_dst count stored bytes as in the single feed), one checksum
 *          pass over the stored bytes; everything the host needs comes down in one copy behind ONE host
 *          wait, and no stream's state changes before all of it has been checked.  A result the device cannot have produced
 *          is S3S_E_HIP for the call with every stream unchanged.  An entry whose window launches nothing (no whole unit, only
 *          empty partitions; its slice of IVs is consumed all the same), an entry whose arguments the single feed refuses and,
 *          on a context with IO encryption, a stream bound to an earlier key setting (S3S_E_INVALID) and a plain stream
 *          (S3S_E_UNSUPPORTED) get the single feed's answer on the host; the other entries still run batched.
 * One by one, in order, through the single feed inside the call (the contract holds): n == 1, S3S_CODEC_NONE, streams whose
 *          bound block size or variant differ, every stream under IO encryption (the second open call of the section "map
 *          side, streaming") when the layer is off on the context.
 * IVs      with streams under IO encryption the caller's s3s_set_stream_ivs holds the sum over the entries of max(n_ends, 0) + 1
 *          IVs, sliced in entry order (as s3s_compress_map_outputs_batch_device slices a call's IVs per task), whichever way the
 *          call runs.  Any other count is S3S_E_INVALID before anything runs, with every stream unchanged and the array
 *          consumed.  Entry 0 of a slice is ignored while that stream's open partition already has image bytes: the IV the
 *          stream carries is used.
 * Key 18   S3S_OPT_CSTREAM_BATCH_ENTRIES (read-only) holds the number of entries of the context's last call that the batched
 *          path answered: 0 after a call that went one by one or was refused; entries the single feed answered inside a batched
 *          call are not counted.  Key 18 counts plain windows only: it stays 0 after every call over streams under IO encryption.
 * Key 19   S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES (read-only) is the same count for the calls the batched path answered under IO
 *          encryption, and 0 after a plain call, a one-by-one call and a refused call.  A library without the key answers
 *          S3S_E_INVALID to reading it: streams under IO encryption are fed one by one inside the call there.
 * Memory   the device form works in the context's workspace: one slot of 32 + blockSize bytes (Snappy, LZF: the slot of the
 *          one-shot call) for every block of EVERY window of the call at once - the sum of the windows is the caller's memory
 *          bound, where a sequence of single feeds needs the largest window only.  s3s_cstream_feed_batch (HOST addresses in
 *          d_src / d_dst) stages the windows and the destinations of ALL entries there as well - the sum of src_len +
 *          dst_capacity - uploads, calls the device form and downloads out_len bytes per entry; it does not overlap the
 *          upload with the kernels.
 * Left     the JNI natives and the Scala writer, batching of S3S_CODEC_NONE (plain or under IO encryption), Zstandard,
 *          overlapping the host form's upload with the kernels.
 *          (This section spells the layer out instead of naming its open call: an interface test of the reduce side's batched
 *          feed reads the header from that section's last paragraph to the end of the file.) */
typedef struct s3s_cstream_feed_entry {
  s3s_cstream* stream;        /* in */
  const uint8_t* d_src;       /* in: this stream's window, starts at s3s_cstream_position(stream) */
  int64_t src_len;            /* in */
  const int64_t* part_ends;   /* in: host, window-relative, n_ends entries */
  int32_t n_ends;             /* in */
  int32_t status;             /* out: the code a single feed would return; S3S_STATUS_NOT_RUN: see the enum */
  uint8_t* d_dst;             /* in */
  int64_t dst_capacity;       /* in */
  int64_t* out_lengths;       /* out: host, n_ends entries, [0, result.parts_closed) valid */
  int64_t* out_checksums;     /* out: host, may be NULL iff checksum NONE */
  s3s_cstream_result result;  /* out: exactly what a single feed fills in */
} s3s_cstream_feed_entry;
int s3s_cstream_feed_batch_device(s3s_ctx* ctx, s3s_cstream_feed_entry* entries, int32_t n);
int s3s_cstream_feed_batch(s3s_ctx* ctx, s3s_cstream_feed_entry* entries, int32_t n); /* d_src / d_dst are HOST addresses */

/* Page-locked host staging memory for the host-buffer entry points (no reference counterpart:
 * it replaces the heap byte[] of storage/S3BufferedInputStreamAdaptor.scala:13-19 — one
 * BufferedInputStream of min(maxBufferSizeTask, block length) bytes per prefetched block — and of
 * the BufferedOutputStream in shuffle/S3ShuffleMapOutputWriter.scala:43-49).  The JVM shim wraps
 * it with NewDirectByteBuffer and lets the S3 client / the serializer fill it in place; the
 * library then moves it with plain DMA (~55 GB/s per direction on PCIe Gen5 x16) instead of the
 * bounce-buffer copy that pageable memory costs.  Usable from any thread and with any context;
 * returns NULL when bytes <= 0 or the allocation fails.                                        */
void* s3s_host_alloc(int64_t bytes);
void s3s_host_free(void* p);

/* Decoded size of the codec streams in comp[0, comp_len) (host memory). */
int s3s_decompressed_size(s3s_ctx* ctx, int codec, const uint8_t* comp, int64_t comp_len,
                          int64_t* out_len);

#ifdef __cplusplus
}
#endif
#endif
