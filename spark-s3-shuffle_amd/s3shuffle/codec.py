"""ctypes binding of include/s3shuffle_codec.h (one method per C entry point)."""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np

CODEC_NONE, CODEC_LZ4, CODEC_SNAPPY = 0, 1, 2
CODEC_ZSTD = 3  # decode of Zstandard frames; the compress entry points refuse it unless OPT_ZSTD_COMPRESS is 1 (ABI 11)
CODEC_LZF = 4  # LZFCompressionCodec streams (compress-lzf chunks around liblzf blocks); compression only with OPT_LZF_COMPRESS = 1
CHECKSUM_NONE, CHECKSUM_ADLER32, CHECKSUM_CRC32, CHECKSUM_CRC32C = 0, 1, 2, 3

OPT_LZ4_BLOCK_SIZE, OPT_SNAPPY_BLOCK_SIZE, OPT_PROFILE = 1, 2, 3
STAGE_TOTAL, STAGE_CODEC, STAGE_ASSEMBLE, STAGE_CHECKSUM, STAGE_DISCOVER, STAGE_HASH = 0, 1, 2, 3, 4, 5
OPT_LZ4_VARIANT = 4
OPT_LZ4_DECODE_VARIANT = 5
OPT_SNAPPY_VARIANT = 6
OPT_LZ4_VARIANT_USED = 7
OPT_LZ4_BLOCK_SIZE_LARGE = 8  # ABI 10: spark.io.compression.lz4.blockSize 64 .. 32m (key 1 stops at 64k and keeps doing so)

OPT_ZSTD_COMPRESS = 9  # ABI 11: 1 = write decode-compatible Zstandard frames on the map side (not libzstd's bytes); default 0
OPT_LZF_COMPRESS = 10  # ABI 11, additive key: 1 = write decode-compatible LZF streams on the map side (not compress-lzf's bytes); default 0
OPT_STREAM_CLASS = 12  # ABI 11, additive, read-only: queue pool of the context's stream (0 lowest priority, 1 normal, 2 highest, 3 shared)
OPT_IO_ENCRYPTION_KEY_BITS = 11  # ABI 11, additive, read-only: 0 / 128 / 192 / 256 - the key Codec.set_io_encryption holds
OPT_ZSTD_DECODE_VARIANT = 13  # ABI 11, additive: 1 (default) = block-independent Zstandard frames one workgroup per block, 0 = one frame per wavefront
OPT_ZSTD_DECODE_BLOCKS = 14  # ABI 11, additive, read-only: blocks of the last Zstandard decode call whose frames completed on the block path
OPT_ZSTD_DECODE_STAGED = 15  # ABI 11, additive: 0 (default) / 1 = Zstandard frames with history across blocks decode in stages (entropy per block, copies per frame)
OPT_ZSTD_DECODE_STAGED_BLOCKS = 16  # ABI 11, additive, read-only: blocks of the last Zstandard decode call whose frames completed on the staged path
OPT_CSTREAM_BATCH_ENTRIES = 18  # ABI 11, additive, read-only: entries of the last compress_stream_feed_batch* call that the batched path answered
OPT_CSTREAM_BATCH_ENC_ENTRIES = 19  # ABI 11, additive, read-only: entries of the last compress_stream_feed_batch* call that the batched path answered under IO encryption
OPT_DSTREAM_BATCH_ENTRIES = 17  # ABI 11, additive, read-only: entries of the last feed_streams* call that the batched path answered (0: it went one by one)

E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_HIP, E_UNSUPPORTED, E_NOMEM = -1, -2, -3, -4, -5, -6, -7
STATUS_NOT_RUN = -100  # per-entry status of a batch call that failed as a call before this entry had a verdict (ABI 6)
_ERR_NAMES = {
    E_INVALID: "S3S_E_INVALID",
    E_CAPACITY: "S3S_E_CAPACITY",
    E_BAD_FRAME: "S3S_E_BAD_FRAME",
    E_CHECKSUM: "S3S_E_CHECKSUM",
    E_HIP: "S3S_E_HIP",
    E_UNSUPPORTED: "S3S_E_UNSUPPORTED",
    E_NOMEM: "S3S_E_NOMEM",
}

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class CodecError(RuntimeError):
    """A negative S3S_E_* return code.  `.code` is the code, `.partition` the failing
    partition for E_CHECKSUM (mirrors SparkException("Invalid checksum detected for ..."))."""

    def __init__(self, code: int, message: str, partition: int = -1):
        super().__init__(f"{_ERR_NAMES.get(code, code)}: {message}")
        self.code = code
        self.partition = partition


def library_path() -> str:
    """The product library; S3S_CODEC_LIB selects another build of the SAME library (e.g. the
    instrumented one used by tools/lz4_timing.py) — never a fallback implementation."""
    override = os.environ.get("S3S_CODEC_LIB")
    if override:
        return override
    return os.path.join(_PKG_ROOT, "lib", "libs3shuffle_codec.so")


class MapTask(ctypes.Structure):
    """struct s3s_map_task (include/s3shuffle_codec.h): one map task of a batched compress call."""
    _fields_ = [("d_src", ctypes.c_void_p), ("src_offsets", ctypes.POINTER(ctypes.c_int64)),
                ("num_partitions", ctypes.c_int32), ("d_dst", ctypes.c_void_p), ("dst_capacity", ctypes.c_int64),
                ("out_index", ctypes.POINTER(ctypes.c_int64)), ("out_checksums", ctypes.POINTER(ctypes.c_int64)),
                ("out_total", ctypes.c_int64), ("status", ctypes.c_int32)]


_LIB = None


class FetchRange(ctypes.Structure):
    """s3s_fetch_range (include/s3shuffle_codec.h)."""
    _fields_ = [("d_comp", ctypes.c_void_p), ("comp_len", ctypes.c_int64),
                ("part_offsets", ctypes.POINTER(ctypes.c_int64)), ("ref_checksums", ctypes.POINTER(ctypes.c_int64)),
                ("num_partitions", ctypes.c_int32), ("d_dst", ctypes.c_void_p), ("dst_capacity", ctypes.c_int64),
                ("out_len", ctypes.c_int64), ("bad_partition", ctypes.c_int32), ("status", ctypes.c_int32)]


class StreamResult(ctypes.Structure):
    """s3s_dstream_result (include/s3shuffle_codec.h): what one feed of a DecodeStream did."""
    _fields_ = [("consumed", ctypes.c_int64), ("out_len", ctypes.c_int64), ("need_comp", ctypes.c_int64),
                ("need_dst", ctypes.c_int64), ("bad_partition", ctypes.c_int32), ("at_end", ctypes.c_int32)]


class FeedEntry(ctypes.Structure):
    """s3s_dstream_feed_entry (include/s3shuffle_codec.h): one stream's window in a batched feed."""
    _fields_ = [("stream", ctypes.c_void_p), ("d_comp", ctypes.c_void_p), ("comp_len", ctypes.c_int64), ("d_dst", ctypes.c_void_p),
                ("dst_capacity", ctypes.c_int64), ("result", StreamResult), ("status", ctypes.c_int32), ("pad", ctypes.c_int32)]


class CompressStreamResult(ctypes.Structure):
    """s3s_cstream_result (include/s3shuffle_codec.h): what one feed of a CompressStream did."""
    _fields_ = [("consumed", ctypes.c_int64), ("out_len", ctypes.c_int64), ("need_src", ctypes.c_int64),
                ("need_dst", ctypes.c_int64), ("parts_closed", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CompressFeedEntry(ctypes.Structure):
    """s3s_cstream_feed_entry (include/s3shuffle_codec.h): one stream's window in a batched feed of the map side."""
    _fields_ = [("stream", ctypes.c_void_p), ("d_src", ctypes.c_void_p), ("src_len", ctypes.c_int64),
                ("part_ends", ctypes.POINTER(ctypes.c_int64)), ("n_ends", ctypes.c_int32), ("status", ctypes.c_int32),
                ("d_dst", ctypes.c_void_p), ("dst_capacity", ctypes.c_int64), ("out_lengths", ctypes.POINTER(ctypes.c_int64)),
                ("out_checksums", ctypes.POINTER(ctypes.c_int64)), ("result", CompressStreamResult)]


def load_library() -> ctypes.CDLL:
    """Loads the HIP codec library.  Fails loudly if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # The HIP runtime maps all streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4) and reads
    # the variable when libamdhip64 is loaded; kernels that share a queue run one after the other.  One context
    # per task thread with 8 threads on 8 MiB map outputs: 12 GB/s with 4 queues, 23 GB/s with 16.  A JVM gets
    # the same through spark.executorEnv.GPU_MAX_HW_QUEUES; an explicit setting wins.  Whatever the
    # value, the library spreads its contexts over the runtime's per-priority queue pools (OPT_STREAM_CLASS), so 3 x cap - 3
    # contexts get a queue of their own: 9 at the default of 4.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    path = library_path()
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it with `python __graft_entry__.py` (or "
            f"`make -C spark-s3-shuffle_amd/csrc`). There is no CPU fallback."
        )
    lib = ctypes.CDLL(path)
    c_i64p = ctypes.POINTER(ctypes.c_int64)
    vp = ctypes.c_void_p
    lib.s3s_version.restype = ctypes.c_char_p
    lib.s3s_abi_version.restype = ctypes.c_int
    lib.s3s_device_count.restype = ctypes.c_int
    lib.s3s_create.restype = vp
    lib.s3s_create.argtypes = [ctypes.c_int, ctypes.c_int64]
    lib.s3s_destroy.argtypes = [vp]
    lib.s3s_last_error.restype = ctypes.c_char_p
    lib.s3s_last_error.argtypes = [vp]
    lib.s3s_set_option.argtypes = [vp, ctypes.c_int, ctypes.c_int64]
    lib.s3s_get_option.restype = ctypes.c_int64
    lib.s3s_get_option.argtypes = [vp, ctypes.c_int]
    lib.s3s_stream.restype = vp
    lib.s3s_stream.argtypes = [vp]
    lib.s3s_stage_ms.restype = ctypes.c_double
    lib.s3s_stage_ms.argtypes = [vp, ctypes.c_int]
    lib.s3s_max_compressed_size.restype = ctypes.c_int64
    lib.s3s_max_compressed_size.argtypes = [vp, ctypes.c_int, c_i64p, ctypes.c_int32]
    comp_args = [vp, ctypes.c_int, ctypes.c_int, vp, c_i64p, ctypes.c_int32, vp, ctypes.c_int64,
                 c_i64p, c_i64p, c_i64p]
    lib.s3s_compress_map_output.argtypes = comp_args
    lib.s3s_compress_map_output_device.argtypes = comp_args
    ck_args = [vp, ctypes.c_int, vp, c_i64p, ctypes.c_int32, c_i64p]
    lib.s3s_checksum_ranges.argtypes = ck_args
    lib.s3s_checksum_ranges_device.argtypes = ck_args
    dec_args = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int64, c_i64p, c_i64p, ctypes.c_int32,
                vp, ctypes.c_int64, c_i64p, ctypes.POINTER(ctypes.c_int32)]
    lib.s3s_decompress_range.argtypes = dec_args
    lib.s3s_decompress_range_device.argtypes = dec_args
    lib.s3s_decompressed_size.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int64, c_i64p]
    c_i32p = ctypes.POINTER(ctypes.c_int32)
    lib.s3s_max_compressed_size_segments.restype = ctypes.c_int64
    lib.s3s_max_compressed_size_segments.argtypes = [vp, ctypes.c_int, c_i64p, ctypes.c_int32]
    seg_args = [vp, ctypes.c_int, ctypes.c_int, vp, c_i64p, ctypes.c_int32, c_i32p, ctypes.c_int32, vp,
                ctypes.c_int64, c_i64p, c_i64p, c_i64p]
    lib.s3s_compress_map_output_segments.argtypes = seg_args
    lib.s3s_compress_map_output_segments_device.argtypes = seg_args
    lib.s3s_compress_map_outputs_batch_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(MapTask),
                                                          ctypes.c_int32]
    lib.s3s_decompress_ranges_batch_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(FetchRange),
                                                       ctypes.c_int32]
    lib.s3s_compress_map_outputs_batch.argtypes = lib.s3s_compress_map_outputs_batch_device.argtypes
    lib.s3s_decompress_ranges_batch.argtypes = lib.s3s_decompress_ranges_batch_device.argtypes
    lib.s3s_host_alloc.restype = vp
    lib.s3s_host_alloc.argtypes = [ctypes.c_int64]
    lib.s3s_host_free.argtypes = [vp]
    if hasattr(lib, "s3s_set_io_encryption"):  # (S3S_CODEC_LIB may name an older build of the library)
        lib.s3s_set_io_encryption.argtypes = [vp, vp, ctypes.c_int32]
        lib.s3s_set_stream_ivs.argtypes = [vp, vp, ctypes.c_int64]
    if hasattr(lib, "s3s_dstream_open"):  # streaming reduce side + seeded checksums (additive, ABI 11)
        seeded_args = [vp, ctypes.c_int, vp, c_i64p, ctypes.c_int32, c_i64p, c_i64p]
        lib.s3s_checksum_ranges_seeded.argtypes = seeded_args
        lib.s3s_checksum_ranges_seeded_device.argtypes = seeded_args
        lib.s3s_dstream_open.argtypes = [vp, ctypes.c_int, ctypes.c_int, c_i64p, c_i64p, ctypes.c_int32, ctypes.POINTER(vp)]
        feed_args = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.POINTER(StreamResult)]
        lib.s3s_dstream_feed.argtypes = feed_args
        lib.s3s_dstream_feed_device.argtypes = feed_args
        lib.s3s_dstream_position.restype = ctypes.c_int64
        lib.s3s_dstream_position.argtypes = [vp]
        lib.s3s_dstream_close.argtypes = [vp]
    if hasattr(lib, "s3s_dstream_open_encrypted"):  # streams under IO encryption (additive, detected by the symbol)
        lib.s3s_dstream_open_encrypted.argtypes = lib.s3s_dstream_open.argtypes
    if hasattr(lib, "s3s_dstream_open_zstd"):  # resumable Zstandard streams (additive, detected by the symbol)
        lib.s3s_dstream_open_zstd.argtypes = [vp, ctypes.c_int, c_i64p, c_i64p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp)]
    if hasattr(lib, "s3s_cstream_open"):  # streaming map side (additive, detected by the symbols)
        lib.s3s_cstream_open.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        cfeed_args = [vp, vp, ctypes.c_int64, c_i64p, ctypes.c_int32, vp, ctypes.c_int64, c_i64p, c_i64p,
                      ctypes.POINTER(CompressStreamResult)]
        lib.s3s_cstream_feed.argtypes = cfeed_args
        lib.s3s_cstream_feed_device.argtypes = cfeed_args
        lib.s3s_cstream_feed_bound.restype = ctypes.c_int64
        lib.s3s_cstream_feed_bound.argtypes = [vp, ctypes.c_int64, ctypes.c_int32]
        lib.s3s_cstream_position.restype = ctypes.c_int64
        lib.s3s_cstream_position.argtypes = [vp]
        lib.s3s_cstream_written.restype = ctypes.c_int64
        lib.s3s_cstream_written.argtypes = [vp]
        lib.s3s_cstream_close.argtypes = [vp]
    if hasattr(lib, "s3s_cstream_open_encrypted"):  # the streaming map side under IO encryption (additive, detected by the symbol)
        lib.s3s_cstream_open_encrypted.argtypes = lib.s3s_cstream_open.argtypes
    if hasattr(lib, "s3s_dstream_held_bytes"):  # debug accessor: device bytes a stream (or, with NULL, all streams) holds between feeds
        lib.s3s_dstream_held_bytes.restype = ctypes.c_int64
        lib.s3s_dstream_held_bytes.argtypes = [vp]
    if hasattr(lib, "s3s_dstream_feed_batch_device"):  # the batched feed (additive, detected by the symbols)
        lib.s3s_dstream_feed_batch_device.argtypes = [vp, ctypes.POINTER(FeedEntry), ctypes.c_int32]
        lib.s3s_dstream_feed_batch.argtypes = lib.s3s_dstream_feed_batch_device.argtypes
    if hasattr(lib, "s3s_cstream_feed_batch_device"):  # the batched feed of the map side (additive, detected by the symbols)
        lib.s3s_cstream_feed_batch_device.argtypes = [vp, ctypes.POINTER(CompressFeedEntry), ctypes.c_int32]
        lib.s3s_cstream_feed_batch.argtypes = lib.s3s_cstream_feed_batch_device.argtypes
    _LIB = lib
    return lib


def device_count() -> int:
    return int(load_library().s3s_device_count())


def _i64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64))


def _p64(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def max_compressed_size(codec: int, src_offsets: Sequence[int], ctx: Optional["Codec"] = None) -> int:
    offs = _i64(src_offsets)
    r = load_library().s3s_max_compressed_size(ctx._h if ctx else None, codec, _p64(offs), len(offs) - 1)
    if r < 0:
        raise CodecError(int(r), "s3s_max_compressed_size")
    return int(r)


class Codec:
    """One s3s_ctx: not thread-safe, one per task thread; device = mapId % nGPU by convention
    (mirrors mapId % folderPrefixes, S3ShuffleDispatcher.scala:142)."""

    def __init__(self, device: int = 0, scratch_bytes: int = 0):
        self._lib = load_library()
        self._h = self._lib.s3s_create(int(device), int(scratch_bytes))
        if not self._h:
            msg = self._lib.s3s_last_error(None).decode()
            raise CodecError(E_HIP, f"s3s_create(device={device}) failed: {msg}")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.s3s_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- helpers -------------------------------------------------------------------------
    def _check(self, rc: int, partition: int = -1):
        if rc != 0:
            raise CodecError(int(rc), self._lib.s3s_last_error(self._h).decode(), partition)

    def set_option(self, key: int, value: int):
        self._check(self._lib.s3s_set_option(self._h, key, int(value)))

    def get_option(self, key: int) -> int:
        return int(self._lib.s3s_get_option(self._h, key))

    def set_io_encryption(self, key: Optional[bytes]):
        """Spark IO encryption (AES/CTR/NoPadding) as a layer on both sides of the codec: a key of 16, 24 or 32 bytes switches
        it on for every later call of this context, None (or b"") switches it off and wipes the key."""
        key = bytes(key) if key else b""
        self._check(self._lib.s3s_set_io_encryption(self._h, key if key else None, len(key)))

    def set_stream_ivs(self, ivs):
        """One 16-byte IV per PARTITION of the NEXT compress call (task by task, then partition by partition; the entry of an
        empty partition is not used): bytes or a uint8 array of 16 * n bytes.  That call consumes them.  Never reusing an IV
        under one key is the caller's duty."""
        a = np.ascontiguousarray(np.frombuffer(ivs, dtype=np.uint8) if isinstance(ivs, (bytes, bytearray)) else ivs, dtype=np.uint8).reshape(-1)
        if a.size % 16:
            raise ValueError("IVs are 16 bytes each")
        self._check(self._lib.s3s_set_stream_ivs(self._h, a.ctypes.data if a.size else None, a.size // 16))

    @property
    def io_encryption_key_bits(self) -> int:
        return self.get_option(OPT_IO_ENCRYPTION_KEY_BITS)

    @property
    def zstd_decode_blocks(self) -> int:
        """Blocks of the last Zstandard decode call whose frames completed on the block path (OPT_ZSTD_DECODE_VARIANT = 1), else 0."""
        return self.get_option(OPT_ZSTD_DECODE_BLOCKS)

    @property
    def zstd_decode_staged_blocks(self) -> int:
        """Blocks of the last Zstandard decode call whose frames completed on the staged path (OPT_ZSTD_DECODE_STAGED = 1), else 0."""
        return self.get_option(OPT_ZSTD_DECODE_STAGED_BLOCKS)

    @property
    def batch_entries(self) -> int:
        """Entries of the last feed_streams* call that the batched path answered; 0 when the call went one by one or was refused."""
        return self.get_option(OPT_DSTREAM_BATCH_ENTRIES)

    def stage_ms(self, stage: int) -> float:
        return float(self._lib.s3s_stage_ms(self._h, stage))

    @property
    def stream(self) -> int:
        return int(self._lib.s3s_stream(self._h) or 0)

    def max_compressed_size(self, codec: int, src_offsets) -> int:
        return max_compressed_size(codec, src_offsets, self)

    # ---- map side ----------------------------------------------------------------------------
    def compress_map_output(self, codec: int, checksum: int, src: np.ndarray, src_offsets,
                            dst_capacity: Optional[int] = None, out: Optional[np.ndarray] = None
                            ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """Host buffers in/out.  Returns (data image, index[N+1], checksums[N] or None).
        `out`: caller-owned destination (e.g. a pinned_buffer) instead of a fresh numpy array."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        offs = _i64(src_offsets)
        n = len(offs) - 1
        cap = self.max_compressed_size(codec, offs) if dst_capacity is None else int(dst_capacity)
        if out is not None:
            cap = min(cap, out.size) if dst_capacity is None else cap
            dst = out
        else:
            dst = np.empty(max(cap, 1), dtype=np.uint8)
        index = np.zeros(n + 1, dtype=np.int64)
        sums = np.zeros(max(n, 1), dtype=np.int64)
        total = ctypes.c_int64(0)
        rc = self._lib.s3s_compress_map_output(
            self._h, codec, checksum, src.ctypes.data, _p64(offs), n, dst.ctypes.data, cap,
            _p64(index), _p64(sums) if checksum != CHECKSUM_NONE else None, ctypes.byref(total))
        self._check(rc)
        return dst[: total.value], index, (sums[:n] if checksum != CHECKSUM_NONE else None)

    def compress_map_output_segments(self, codec: int, checksum: int, src: np.ndarray, seg_offsets,
                                     part_first_seg) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """Multi-spill map task: partition p = pieces [part_first_seg[p], part_first_seg[p+1]) of
        seg_offsets, one complete codec stream per non-empty piece (host buffers)."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        segs = _i64(seg_offsets)
        pfs = np.ascontiguousarray(part_first_seg, dtype=np.int32)
        ns, n = len(segs) - 1, len(pfs) - 1
        cap = int(self._lib.s3s_max_compressed_size_segments(self._h, codec, _p64(segs), ns))
        if cap < 0:
            self._check(cap)
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        index = np.zeros(n + 1, dtype=np.int64)
        sums = np.zeros(max(n, 1), dtype=np.int64)
        total = ctypes.c_int64(0)
        rc = self._lib.s3s_compress_map_output_segments(
            self._h, codec, checksum, src.ctypes.data, _p64(segs), ns,
            pfs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, dst.ctypes.data, cap, _p64(index),
            _p64(sums) if checksum != CHECKSUM_NONE else None, ctypes.byref(total))
        self._check(rc)
        return dst[: total.value], index, (sums[:n] if checksum != CHECKSUM_NONE else None)

    def compress_map_output_device(self, codec: int, checksum: int, d_src: int, src_offsets,
                                   d_dst: int, dst_capacity: int
                                   ) -> Tuple[int, np.ndarray, Optional[np.ndarray]]:
        """Device pointers in/out.  Returns (total bytes, index[N+1], checksums[N] or None)."""
        offs = _i64(src_offsets)
        n = len(offs) - 1
        index = np.zeros(n + 1, dtype=np.int64)
        sums = np.zeros(max(n, 1), dtype=np.int64)
        total = ctypes.c_int64(0)
        rc = self._lib.s3s_compress_map_output_device(
            self._h, codec, checksum, ctypes.c_void_p(d_src), _p64(offs), n, ctypes.c_void_p(d_dst),
            int(dst_capacity), _p64(index), _p64(sums) if checksum != CHECKSUM_NONE else None,
            ctypes.byref(total))
        self._check(rc)
        return int(total.value), index, (sums[:n] if checksum != CHECKSUM_NONE else None)

    def compress_map_outputs_batch(self, codec: int, checksum: int, tasks):
        """Batched HOST-buffer form (what the JNI shim binds): `tasks` = [(src_address, src_offsets, dst_address,
        dst_capacity), ...] with host addresses (e.g. `PinnedBuffer.address`, or `ndarray.ctypes.data`) -> per task
        (total bytes, index[N+1], checksums[N] or None).  Upload, codec and download of consecutive groups overlap."""
        return self.compress_map_outputs_batch_device(codec, checksum, tasks, _host=True)

    def compress_map_outputs_batch_device(self, codec: int, checksum: int, tasks, _host: bool = False):
        """Batched device form: `tasks` = [(d_src, src_offsets, d_dst, dst_capacity), ...] -> per task
        (total bytes, index[N+1], checksums[N] or None).  One codec launch and one stream sync for all."""
        arr = (MapTask * len(tasks))()
        keep = []
        for i, (d_src, src_offsets, d_dst, cap) in enumerate(tasks):
            offs = _i64(src_offsets)
            n = len(offs) - 1
            index = np.zeros(n + 1, dtype=np.int64)
            sums = np.zeros(max(n, 1), dtype=np.int64)
            keep.append((offs, index, sums, n))
            arr[i].d_src = d_src
            arr[i].src_offsets = _p64(offs)
            arr[i].num_partitions = n
            arr[i].d_dst = d_dst
            arr[i].dst_capacity = int(cap)
            arr[i].out_index = _p64(index)
            arr[i].out_checksums = _p64(sums) if checksum != CHECKSUM_NONE else None
        fn = self._lib.s3s_compress_map_outputs_batch if _host else self._lib.s3s_compress_map_outputs_batch_device
        rc = fn(self._h, codec, checksum, arr, len(tasks))
        self._check(rc)
        return [(int(arr[i].out_total), k[1], (k[2][:k[3]] if checksum != CHECKSUM_NONE else None))
                for i, k in enumerate(keep)]

    # ---- checksum only -----------------------------------------------------------------------
    def checksum_ranges(self, algo: int, data: np.ndarray, offsets) -> np.ndarray:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = _i64(offsets)
        n = len(offs) - 1
        out = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.s3s_checksum_ranges(self._h, algo, data.ctypes.data, _p64(offs), n, _p64(out)))
        return out[:n]

    def checksum_ranges_device(self, algo: int, d_data: int, offsets) -> np.ndarray:
        offs = _i64(offsets)
        n = len(offs) - 1
        out = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.s3s_checksum_ranges_device(self._h, algo, ctypes.c_void_p(d_data), _p64(offs), n, _p64(out)))
        return out[:n]

    def checksum_ranges_seeded(self, algo: int, data: np.ndarray, offsets, seeds=None) -> np.ndarray:
        """java.util.zip.Checksum continued: out[i] = the state after data[offsets[i]:offsets[i+1]] when it was seeds[i]
        before (getValue() of the bytes so far; None: fresh).  Host buffer."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offs = _i64(offsets)
        n = len(offs) - 1
        sd = _i64(seeds) if seeds is not None else None
        if sd is not None and sd.size != n:
            raise ValueError("one seed per range")
        out = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.s3s_checksum_ranges_seeded(self._h, algo, data.ctypes.data, _p64(offs), n,
                                                         _p64(sd) if sd is not None else None, _p64(out)))
        return out[:n]

    def checksum_ranges_seeded_device(self, algo: int, d_data: int, offsets, seeds=None) -> np.ndarray:
        offs = _i64(offsets)
        n = len(offs) - 1
        sd = _i64(seeds) if seeds is not None else None
        if sd is not None and sd.size != n:
            raise ValueError("one seed per range")
        out = np.zeros(max(n, 1), dtype=np.int64)
        self._check(self._lib.s3s_checksum_ranges_seeded_device(self._h, algo, ctypes.c_void_p(d_data), _p64(offs), n,
                                                                _p64(sd) if sd is not None else None, _p64(out)))
        return out[:n]

    def compress_stream(self, codec: int, checksum: int, encrypted: bool = False) -> "CompressStream":
        """A map output compressed window by window in bounded memory (s3s_cstream_*): the same bytes, lengths and checksums
        as compress_map_output_device for the same source, ends and options.  `encrypted`: under IO encryption, through
        s3s_cstream_open_encrypted (capacities, lengths and `written` count the stored bytes, IVs included; set_stream_ivs
        with `len(part_ends) + 1` IVs goes in front of every feed)."""
        return CompressStream(self, codec, checksum, encrypted=encrypted)

    @property
    def compress_batch_entries(self) -> int:
        """Entries of the last compress_stream_feed_batch* call that the batched path answered; 0 when it went one by one or was refused."""
        return self.get_option(OPT_CSTREAM_BATCH_ENTRIES)

    @property
    def compress_batch_encrypted_entries(self) -> int:
        """Entries of the last compress_stream_feed_batch* call that the batched path answered under IO encryption (key 19);
        0 after a plain call, a one-by-one call and a refused call.  `compress_batch_entries` (key 18) counts plain windows only."""
        return self.get_option(OPT_CSTREAM_BATCH_ENC_ENTRIES)

    def compress_stream_feed_batch(self, entries, _host: bool = False):
        """The batched feed of the map side (s3s_cstream_feed_batch_device): `entries` = [(CompressStream, d_src, src_len,
        part_ends, d_dst, dst_capacity), ...], one window of each of several streams of this context -> per entry the
        CompressStreamResult that `stream.feed_device` alone would have given, with `.code`, `.lengths` and `.checksums` (None
        when the stream has no checksums).  Nothing is raised for an entry's own verdict; `last_compress_batch_code` is the
        call's return code (the first entry's that is not S3S_OK, or S3S_E_INVALID with every entry S3S_STATUS_NOT_RUN)."""
        if not hasattr(self._lib, "s3s_cstream_feed_batch_device"):
            raise CodecError(E_UNSUPPORTED, "this build of the library has no s3s_cstream_feed_batch_device")
        arr = (CompressFeedEntry * max(len(entries), 1))()
        keep = []
        for i, (stream, d_src, src_len, part_ends, d_dst, cap) in enumerate(entries):
            ends = _i64(part_ends)
            n = len(ends)
            lengths = np.zeros(max(n, 1), dtype=np.int64)
            with_sums = getattr(stream, "_checksum", CHECKSUM_ADLER32) != CHECKSUM_NONE
            sums = np.zeros(max(n, 1), dtype=np.int64) if with_sums else None
            keep.append((ends, lengths, sums))
            arr[i].stream = getattr(stream, "_s", stream)  # a CompressStream, or a raw handle (None: a null stream)
            arr[i].d_src = d_src if src_len else None
            arr[i].src_len = int(src_len)
            arr[i].part_ends = _p64(ends) if n else None
            arr[i].n_ends = n
            arr[i].d_dst = d_dst if cap else None
            arr[i].dst_capacity = int(cap)
            arr[i].out_lengths = _p64(lengths) if n else None
            arr[i].out_checksums = _p64(sums) if (n and sums is not None) else None
        fn = self._lib.s3s_cstream_feed_batch if _host else self._lib.s3s_cstream_feed_batch_device
        self.last_compress_batch_code = int(fn(self._h, arr, len(entries)))
        out = []
        for i, e in enumerate(entries):
            r = CompressStreamResult.from_buffer_copy(arr[i].result)
            r.code = int(arr[i].status)
            closed = r.parts_closed if r.code == 0 else 0
            r.lengths = keep[i][1][:closed]
            r.checksums = keep[i][2][:closed] if keep[i][2] is not None else None
            if hasattr(e[0], "last_result"):
                e[0].last_result = r
            out.append(r)
        return out

    def compress_stream_feed_batch_host(self, entries):
        """The host-buffer form (s3s_cstream_feed_batch): `entries` = [(CompressStream, src, part_ends, dst), ...] or
        [(CompressStream, src, part_ends, dst, dst_capacity), ...] with uint8 arrays; the image bytes land in
        dst[:result.out_len].  The library stages the windows and destinations of ALL entries on the device: the sum of their
        sizes is the memory bound."""
        rows, keep = [], []
        for e in entries:
            stream, src, ends, dst = e[0], np.ascontiguousarray(e[1], dtype=np.uint8), e[2], e[3]
            if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable):
                raise ValueError("dst must be a writable C-contiguous uint8 array (the library writes into it)")
            cap = dst.size if len(e) < 5 or e[4] is None else int(e[4])
            if not 0 <= cap <= dst.size:
                raise ValueError(f"dst_capacity {cap} is outside dst's {dst.size} bytes")
            keep.append(src)
            rows.append((stream, src.ctypes.data, src.size, ends, dst.ctypes.data, cap))
        return self.compress_stream_feed_batch(rows, _host=True)

    # ---- reduce side ---------------------------------------------------------------------------
    def decode_stream(self, codec: int, checksum: int, part_offsets, ref_checksums=None, encrypted: bool = False,
                      window_log_max: Optional[int] = None) -> "DecodeStream":
        """A fetched range decoded window by window in bounded memory (s3s_dstream_*); `encrypted`: a range stored under IO
        encryption, through s3s_dstream_open_encrypted (offsets, windows and positions count the stored bytes, IVs included);
        `window_log_max` (10 .. 27, with ZSTD): a resumable Zstandard stream through s3s_dstream_open_zstd, which keeps at most
        1 << window_log_max bytes of history on the device for its open frame."""
        return DecodeStream(self, codec, checksum, part_offsets, ref_checksums, encrypted=encrypted, window_log_max=window_log_max)

    def feed_streams_device(self, entries, _host: bool = False):
        """The batched feed (s3s_dstream_feed_batch_device): `entries` = [(DecodeStream, d_comp, comp_len, d_dst, dst_capacity),
        ...], one window of each of several streams of this context -> per entry (status, StreamResult), each what
        `stream.feed_device` alone would have given.  Nothing is raised for an entry's own verdict; `last_batch_code` is the
        call's return code (the first entry's that is not S3S_OK, or S3S_E_INVALID with every entry S3S_STATUS_NOT_RUN)."""
        if not hasattr(self._lib, "s3s_dstream_feed_batch_device"):
            raise CodecError(E_UNSUPPORTED, "this build of the library has no s3s_dstream_feed_batch_device")
        arr = (FeedEntry * max(len(entries), 1))()
        for i, (stream, d_comp, comp_len, d_dst, cap) in enumerate(entries):
            arr[i].stream = getattr(stream, "_s", stream)  # a DecodeStream, or a raw handle (None: a null stream)
            arr[i].d_comp = d_comp if comp_len else None
            arr[i].comp_len = int(comp_len)
            arr[i].d_dst = d_dst if cap else None
            arr[i].dst_capacity = int(cap)
        fn = self._lib.s3s_dstream_feed_batch if _host else self._lib.s3s_dstream_feed_batch_device
        self.last_batch_code = int(fn(self._h, arr, len(entries)))
        out = []
        for i, e in enumerate(entries):
            r = StreamResult.from_buffer_copy(arr[i].result)
            r.code = int(arr[i].status)
            if hasattr(e[0], "last_result"):
                e[0].last_result = r
            out.append((r.code, r))
        return out

    def feed_streams(self, entries):
        """The host-buffer form (s3s_dstream_feed_batch): `entries` = [(DecodeStream, comp, dst), ...] or
        [(DecodeStream, comp, dst, dst_capacity), ...] with uint8 arrays; the decoded bytes land in dst[:result.out_len].  The
        library stages the windows and destinations of ALL entries on the device: the sum of their sizes is the memory bound."""
        rows, keep = [], []
        for e in entries:
            stream, comp, dst = e[0], np.ascontiguousarray(e[1], dtype=np.uint8), e[2]
            if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable):
                raise ValueError("dst must be a writable C-contiguous uint8 array (the library writes into it)")
            cap = dst.size if len(e) < 4 or e[3] is None else int(e[3])
            if not 0 <= cap <= dst.size:
                raise ValueError(f"dst_capacity {cap} is outside dst's {dst.size} bytes")
            keep.append(comp)
            rows.append((stream, comp.ctypes.data, comp.size, dst.ctypes.data, cap))
        return self.feed_streams_device(rows, _host=True)

    def decompressed_size(self, codec: int, comp: np.ndarray) -> int:
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        out = ctypes.c_int64(0)
        self._check(self._lib.s3s_decompressed_size(self._h, codec, comp.ctypes.data, comp.size, ctypes.byref(out)))
        return int(out.value)

    def decompress_range(self, codec: int, checksum: int, comp: np.ndarray, part_offsets,
                         ref_checksums=None, dst_capacity: Optional[int] = None,
                         out: Optional[np.ndarray] = None) -> np.ndarray:
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        offs = _i64(part_offsets)
        n = len(offs) - 1
        refs = _i64(ref_checksums) if ref_checksums is not None else None
        if out is not None:
            cap = out.size if dst_capacity is None else int(dst_capacity)
            dst = out
        else:
            if dst_capacity is not None:
                cap = int(dst_capacity)
            elif self.get_option(OPT_IO_ENCRYPTION_KEY_BITS) > 0:  # every partition is a stream of its own, IV first
                cap = sum(self.decompressed_size(codec, comp[offs[p]:offs[p + 1]]) for p in range(n))
            else:
                cap = self.decompressed_size(codec, comp)
            dst = np.empty(max(cap, 1), dtype=np.uint8)
        out_len = ctypes.c_int64(0)
        bad = ctypes.c_int32(-1)
        rc = self._lib.s3s_decompress_range(
            self._h, codec, checksum, comp.ctypes.data, comp.size, _p64(offs),
            _p64(refs) if refs is not None else None, n, dst.ctypes.data, cap,
            ctypes.byref(out_len), ctypes.byref(bad))
        self._check(rc, bad.value)
        return dst[: out_len.value]

    def decompress_range_device(self, codec: int, checksum: int, d_comp: int, comp_len: int,
                                part_offsets, ref_checksums, d_dst: int, dst_capacity: int) -> int:
        offs = _i64(part_offsets)
        n = len(offs) - 1
        refs = _i64(ref_checksums) if ref_checksums is not None else None
        out_len = ctypes.c_int64(0)
        bad = ctypes.c_int32(-1)
        rc = self._lib.s3s_decompress_range_device(
            self._h, codec, checksum, ctypes.c_void_p(d_comp), int(comp_len), _p64(offs),
            _p64(refs) if refs is not None else None, n, ctypes.c_void_p(d_dst), int(dst_capacity),
            ctypes.byref(out_len), ctypes.byref(bad))
        self._check(rc, bad.value)
        return int(out_len.value)



    def decompress_ranges_batch(self, codec: int, checksum: int, ranges, raise_on_error: bool = True):
        """Batched HOST-buffer form: `ranges` = [(comp_address, comp_len, part_offsets, ref_checksums, dst_address,
        dst_capacity), ...] with host addresses -> per range (status, decoded bytes, bad partition)."""
        return self.decompress_ranges_batch_device(codec, checksum, ranges, raise_on_error, _host=True)

    def decompress_ranges_batch_device(self, codec: int, checksum: int, ranges, raise_on_error: bool = True,
                                       _host: bool = False):
        """Batched device form: `ranges` = [(d_comp, comp_len, part_offsets, ref_checksums, d_dst, dst_capacity), ...]
        -> per range (status, decoded bytes, bad partition).  One decode launch for all, three stream syncs."""
        arr = (FetchRange * len(ranges))()
        keep = []
        for i, (d_comp, comp_len, part_offsets, refs, d_dst, cap) in enumerate(ranges):
            offs = _i64(part_offsets)
            r = _i64(refs) if refs is not None else None
            keep.append((offs, r))
            arr[i].d_comp = d_comp
            arr[i].comp_len = int(comp_len)
            arr[i].part_offsets = _p64(offs)
            arr[i].ref_checksums = _p64(r) if r is not None else None
            arr[i].num_partitions = len(offs) - 1
            arr[i].d_dst = d_dst
            arr[i].dst_capacity = int(cap)
        fn = self._lib.s3s_decompress_ranges_batch if _host else self._lib.s3s_decompress_ranges_batch_device
        rc = fn(self._h, codec, checksum, arr, len(ranges))
        out = [(int(arr[i].status), int(arr[i].out_len), int(arr[i].bad_partition)) for i in range(len(ranges))]
        if raise_on_error:
            bad = next((i for i, o in enumerate(out) if o[0] != 0), -1)
            self._check(rc, out[bad][2] if bad >= 0 else -1)
        return out


class DecodeStream:
    """One s3s_dstream: the streaming reduce side.  `feed` / `feed_device` take the window of compressed bytes that starts at
    `position` and return the StreamResult of the feed: `consumed` bytes of the window were decoded to `out_len` bytes;
    `consumed == 0` with `need_comp` asks for a longer window.  S3S_E_CAPACITY is NOT raised (the stream stays usable):
    the result carries `need_dst` and `.code == E_CAPACITY`.  Every other error raises CodecError; E_BAD_FRAME and E_CHECKSUM
    stick, E_UNSUPPORTED from a feed (a unit that claims more than any decoder takes) consumes nothing and repeats.
    `last_result` is the StreamResult of the latest feed, also of one that raised.
    `close()` raises E_BAD_FRAME when the range was not read to its end.  Also a context manager (which closes quietly after
    an exception, loudly otherwise).
    `encrypted=True` opens the stream with s3s_dstream_open_encrypted (the context's IO encryption must be on): a partition's
    16-byte IV is a unit of its own that decodes to nothing, and the stream is bound to the key setting it was opened under.
    `window_log_max=N` with ZSTD opens the stream with s3s_dstream_open_zstd: the units are frame headers, blocks and skippable
    frames, and the stream owns device memory (the open frame's history, at most 1 << N bytes) until the frame ends or `close()`.
    ZSTD without it is refused at open, as before."""

    def __init__(self, codec_ctx: Codec, codec: int, checksum: int, part_offsets, ref_checksums=None, encrypted: bool = False,
                 window_log_max: Optional[int] = None):
        self._ctx = codec_ctx
        self._lib = codec_ctx._lib
        offs = _i64(part_offsets)
        refs = _i64(ref_checksums) if ref_checksums is not None else None
        h = ctypes.c_void_p(None)
        self._s = None
        self.last_result = None
        if encrypted and not hasattr(self._lib, "s3s_dstream_open_encrypted"):
            raise CodecError(E_UNSUPPORTED, "this build of the library has no s3s_dstream_open_encrypted")
        if window_log_max is not None:
            if codec != CODEC_ZSTD or encrypted:
                raise ValueError("window_log_max goes with ZSTD and without `encrypted`")
            if not hasattr(self._lib, "s3s_dstream_open_zstd"):
                raise CodecError(E_UNSUPPORTED, "this build of the library has no s3s_dstream_open_zstd")
            rc = self._lib.s3s_dstream_open_zstd(codec_ctx._h, checksum, _p64(offs), _p64(refs) if refs is not None else None,
                                                 len(offs) - 1, int(window_log_max), ctypes.byref(h))
        else:
            fn = self._lib.s3s_dstream_open_encrypted if encrypted else self._lib.s3s_dstream_open
            rc = fn(codec_ctx._h, codec, checksum, _p64(offs), _p64(refs) if refs is not None else None, len(offs) - 1, ctypes.byref(h))
        codec_ctx._check(rc)
        self._s = h.value

    @property
    def position(self) -> int:
        return int(self._lib.s3s_dstream_position(self._s))

    @property
    def held_device_bytes(self) -> int:
        """Device bytes the stream holds between feeds (s3s_dstream_held_bytes): 0 unless a Zstandard frame is open."""
        return int(self._lib.s3s_dstream_held_bytes(self._s)) if self._s else 0

    def _feed(self, fn, comp_ptr, comp_len, dst_ptr, dst_capacity):
        if not self._s:
            raise ValueError("the stream is closed")
        r = StreamResult()
        rc = fn(self._s, comp_ptr, int(comp_len), dst_ptr, int(dst_capacity), ctypes.byref(r))
        r.code = int(rc)
        self.last_result = r
        if rc != 0 and rc != E_CAPACITY:
            self._ctx._check(rc, r.bad_partition)
        return r

    def feed(self, comp: np.ndarray, dst: np.ndarray, dst_capacity: Optional[int] = None) -> StreamResult:
        """Host buffers: `comp` is the window (uint8), the decoded bytes land in dst[:result.out_len]."""
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable):
            raise ValueError("dst must be a writable C-contiguous uint8 array (the library writes into it)")
        cap = dst.size if dst_capacity is None else int(dst_capacity)
        if not 0 <= cap <= dst.size:
            raise ValueError(f"dst_capacity {cap} is outside dst's {dst.size} bytes")
        return self._feed(self._lib.s3s_dstream_feed, comp.ctypes.data if comp.size else None, comp.size,
                          dst.ctypes.data if cap else None, cap)

    def feed_device(self, d_comp: int, comp_len: int, d_dst: int, dst_capacity: int) -> StreamResult:
        """Device pointers on the context's device."""
        return self._feed(self._lib.s3s_dstream_feed_device, ctypes.c_void_p(d_comp) if comp_len else None, comp_len,
                          ctypes.c_void_p(d_dst) if dst_capacity else None, dst_capacity)

    def close(self, check: bool = True) -> int:
        """Frees the stream; returns the code s3s_dstream_close gave (raises it when `check` and it is not S3S_OK)."""
        if not self._s:
            return 0
        rc = int(self._lib.s3s_dstream_close(self._s))
        self._s = None
        if check and rc != 0:
            raise CodecError(rc, "the stream was closed before the end of the range" if rc == E_BAD_FRAME else "the stream had failed")
        return rc

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *exc):
        self.close(check=exc_type is None)

    def __del__(self):
        try:
            if self._s and getattr(self._ctx, "_h", None):
                self.close(check=False)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class CompressStream:
    """One s3s_cstream: the streaming map side.  `feed` / `feed_device` take the window of source bytes that starts at
    `position` and the window-relative offsets at which partitions end in it, and return the CompressStreamResult of the feed
    with `.lengths` / `.checksums` (the image length and checksum of every partition the feed closed, `parts_closed` of them;
    `.checksums` is None with CHECKSUM_NONE): `consumed` source bytes became `out_len` image bytes.  `consumed == 0` with
    `need_src` asks for a longer window.  S3S_E_CAPACITY is NOT raised (the stream stays usable): the result carries
    `need_dst` and `.code == E_CAPACITY`.  Every other error raises CodecError.  `last_result` is the result of the latest feed.
    `close()` raises E_INVALID when bytes of the open partition have been consumed (the image would end inside a codec
    stream).  Also a context manager (which closes quietly after an exception, loudly otherwise).

    `encrypted=True` opens the stream with s3s_cstream_open_encrypted (the context's IO encryption must be on): a non-empty
    partition is stored as its IV and the cipher text, the IV in the unit of the partition's first block.  Before EVERY feed
    the caller gives `len(part_ends) + 1` IVs to Codec.set_stream_ivs: entry j is the IV of the partition piece j belongs to."""

    def __init__(self, codec_ctx: Codec, codec: int, checksum: int, encrypted: bool = False):
        self._ctx = codec_ctx
        self._lib = codec_ctx._lib
        self._s = None
        self._checksum = checksum
        self.last_result = None
        if not hasattr(self._lib, "s3s_cstream_open"):
            raise CodecError(E_UNSUPPORTED, "this build of the library has no s3s_cstream_open")
        if encrypted and not hasattr(self._lib, "s3s_cstream_open_encrypted"):
            raise CodecError(E_UNSUPPORTED, "this build of the library has no s3s_cstream_open_encrypted")
        h = ctypes.c_void_p(None)
        fn = self._lib.s3s_cstream_open_encrypted if encrypted else self._lib.s3s_cstream_open
        codec_ctx._check(fn(codec_ctx._h, codec, checksum, ctypes.byref(h)))
        self._s = h.value

    @property
    def position(self) -> int:
        """Source bytes consumed so far."""
        return int(self._lib.s3s_cstream_position(self._s))

    @property
    def written(self) -> int:
        """Image bytes produced so far: the image offset of the next feed's output."""
        return int(self._lib.s3s_cstream_written(self._s))

    def feed_bound(self, src_len: int, n_ends: int) -> int:
        """A dst capacity with which a feed of this shape never answers E_CAPACITY."""
        r = int(self._lib.s3s_cstream_feed_bound(self._s, int(src_len), int(n_ends)))
        if r < 0:
            raise CodecError(r, "s3s_cstream_feed_bound")
        return r

    def _feed(self, fn, src_ptr, src_len, part_ends, dst_ptr, dst_capacity):
        if not self._s:
            raise ValueError("the stream is closed")
        ends = _i64(part_ends)
        n = len(ends)
        lengths = np.zeros(max(n, 1), dtype=np.int64)
        sums = np.zeros(max(n, 1), dtype=np.int64) if self._checksum != CHECKSUM_NONE else None
        r = CompressStreamResult()
        rc = fn(self._s, src_ptr, int(src_len), _p64(ends) if n else None, n, dst_ptr, int(dst_capacity),
                _p64(lengths) if n else None, _p64(sums) if (n and sums is not None) else None, ctypes.byref(r))
        r.code = int(rc)
        r.lengths = lengths[: r.parts_closed]
        r.checksums = sums[: r.parts_closed] if sums is not None else None
        self.last_result = r
        if rc != 0 and rc != E_CAPACITY:
            self._ctx._check(rc)
        return r

    def feed(self, src: np.ndarray, part_ends, dst: np.ndarray, dst_capacity: Optional[int] = None) -> CompressStreamResult:
        """Host buffers: `src` is the window (uint8), the image bytes land in dst[:result.out_len]."""
        if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable):
            raise ValueError("dst must be a writable C-contiguous uint8 array (the library writes into it)")
        cap = dst.size if dst_capacity is None else int(dst_capacity)
        if not 0 <= cap <= dst.size:
            raise ValueError(f"dst_capacity {cap} is outside dst's {dst.size} bytes")
        src = np.ascontiguousarray(src, dtype=np.uint8)
        return self._feed(self._lib.s3s_cstream_feed, src.ctypes.data if src.size else None, src.size, part_ends,
                          dst.ctypes.data if cap else None, cap)

    def feed_device(self, d_src: int, src_len: int, part_ends, d_dst: int, dst_capacity: int) -> CompressStreamResult:
        """Device pointers on the context's device."""
        return self._feed(self._lib.s3s_cstream_feed_device, ctypes.c_void_p(d_src) if src_len else None, src_len, part_ends,
                          ctypes.c_void_p(d_dst) if dst_capacity else None, dst_capacity)

    def close(self, check: bool = True) -> int:
        """Frees the stream; returns the code s3s_cstream_close gave (raises it when `check` and it is not S3S_OK)."""
        if not self._s:
            return 0
        rc = int(self._lib.s3s_cstream_close(self._s))
        self._s = None
        if check and rc != 0:
            raise CodecError(rc, "the stream was closed inside a partition: the image ends inside a codec stream")
        return rc

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *exc):
        self.close(check=exc_type is None)

    def __del__(self):
        try:
            if self._s and getattr(self._ctx, "_h", None):
                self.close(check=False)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class PinnedBuffer:
    """Page-locked host memory from s3s_host_alloc (what the JVM shim would wrap with
    NewDirectByteBuffer).  `.array` is a uint8 view; the host-buffer entry points move it with
    plain DMA.  Keep the object alive while views of `.array` are in use; `free()` is explicit."""

    def __init__(self, nbytes: int):
        self._lib = load_library()
        self.nbytes = max(int(nbytes), 1)
        self.ptr = self._lib.s3s_host_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError(f"s3s_host_alloc({self.nbytes}) failed")
        self.array = np.frombuffer((ctypes.c_uint8 * self.nbytes).from_address(self.ptr), dtype=np.uint8)

    def free(self) -> None:
        if self.ptr:
            self.array = None
            self._lib.s3s_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
