"""CPU: the entry point of resumable Zstandard streams (s3s_dstream_open_zstd) as far as it goes without a GPU: the header's
declaration and words, the exported symbol, the Python binding, and the answer of a build without the symbol."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")


def test_header_declares_and_library_exports_the_symbol(codec_lib):
    import s3shuffle

    header = open(HEADER).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", s3shuffle.library_path()], check=True, capture_output=True, text=True).stdout
    assert re.search(r"int s3s_dstream_open_zstd\(s3s_ctx\* ctx, int checksum_algo, const int64_t\* part_offsets,\s*const int64_t\* ref_checksums,"
                     r"\s*int32_t nparts,\s*int32_t window_log_max, s3s_dstream\*\* out\);", header)
    assert re.search(r"\bT s3s_dstream_open_zstd\b", exported)
    fn = codec_lib.s3s_dstream_open_zstd
    assert len(fn.argtypes) == 7 and fn.argtypes[5] is ctypes.c_int32 and fn.argtypes[1] is ctypes.c_int
    assert re.search(r"int64_t s3s_dstream_held_bytes\(const s3s_dstream\* s\);", header) and re.search(r"\bT s3s_dstream_held_bytes\b", exported)
    assert codec_lib.s3s_dstream_held_bytes.restype is ctypes.c_int64 and codec_lib.s3s_dstream_held_bytes(None) == 0
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()


def test_header_states_the_contract():
    header = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    for needle in ("window_log_max = 10 .. 27", "window log 19 at level 1 and 21 at level 3", "a frame header of 6 .. 18 bytes",
                   "a skippable frame of 8 + n bytes", "never more than 3 + 128 KiB", "need_dst never exceeds 128 KiB", "Content_Checksum",
                   "Dictionary_ID", "a skippable frame above 32 MiB", "not sticky", "a partition that ends with a frame open",
                   "min(Window_Size, bytes of the frame produced so far)", "RFC 8878", "owns device memory between feeds",
                   "the three repeat offsets", "S3S_E_NOMEM with nothing consumed", "S3S_OPT_ZSTD_DECODE_VARIANT", "S3S_OPT_ZSTD_DECODE_STAGED",
                   # ... and the words of the contract it extends are still there
                   "S3S_CODEC_ZSTD", "streaming map side", "host mirror", "batched feed", "handed out BEFORE its checksum", "before a corrupt frame"):
        assert needle in header, needle


def test_open_checks_its_arguments_before_any_device_work(codec_lib):
    """window_log_max outside 10 .. 27 and a null context are refused before the context is looked at."""
    out = ctypes.c_void_p(None)
    offs = (ctypes.c_int64 * 1)(0)
    assert codec_lib.s3s_dstream_open_zstd(None, 0, offs, None, 0, 19, ctypes.byref(out)) == -1 and not out.value


def test_decode_stream_without_the_symbol_is_unsupported():
    import s3shuffle
    from s3shuffle import codec

    class Hidden:  # a build of the library from before the entry point
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "s3s_dstream_open_zstd":
                raise AttributeError(name)
            return getattr(self._lib, name)

    ctx = s3shuffle.Codec.__new__(s3shuffle.Codec)
    ctx._lib, ctx._h = Hidden(codec.load_library()), None
    with pytest.raises(s3shuffle.CodecError) as e:
        s3shuffle.DecodeStream(ctx, codec.CODEC_ZSTD, 0, np.array([0, 10], np.int64), window_log_max=19)
    assert e.value.code == codec.E_UNSUPPORTED
    with pytest.raises(ValueError):  # window_log_max goes with ZSTD only
        s3shuffle.DecodeStream(ctx, codec.CODEC_LZ4, 0, np.array([0, 10], np.int64), window_log_max=19)
    assert "window_log_max" in s3shuffle.Codec.decode_stream.__doc__
