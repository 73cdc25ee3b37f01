"""CPU: the streaming reduce side (s3s_dstream_*, s3s_checksum_ranges_seeded*) as far as it goes without a GPU - the header
declares the symbols and the cross-compiled library exports them, the Python binding binds them, the ABI version did not move;
the new natives of jni/s3s_jni.c run against the mock JNIEnv (tests/mock_jni/jni_exec_stream.c, as tests/test_jni_exec.py does
for the others) and the Scala text names them; the seed step of the three checksums against zlib's combine identities."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
MOCK = os.path.join(ROOT, "tests", "mock_jni")
JNI_C = os.path.join(ROOT, "jni", "s3s_jni.c")
SHIM = os.path.join(ROOT, "scala", "org", "apache", "spark", "shuffle", "gpu")
SYMBOLS = ["s3s_dstream_open", "s3s_dstream_feed_device", "s3s_dstream_feed", "s3s_dstream_position", "s3s_dstream_close",
           "s3s_checksum_ranges_seeded", "s3s_checksum_ranges_seeded_device"]
NATIVES = ["dstreamOpen", "dstreamFeed", "dstreamPosition", "dstreamClose", "checksumRangesSeeded"]


# ---- header and binding --------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols(codec_lib):
    header = open(HEADER).read()
    import s3shuffle

    exported = subprocess.run(["nm", "-D", "--defined-only", s3shuffle.library_path()], check=True, capture_output=True, text=True).stdout
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert re.search(r"\bT %s\b" % sym, exported), sym
        assert getattr(codec_lib, sym).argtypes, sym  # bound by s3shuffle.codec.load_library
    assert "typedef struct s3s_dstream_result" in header
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()
    # the contract's words are in the header: what is out of scope, and the two things a caller must know about order
    for needle in ("handed out BEFORE its checksum", "before a corrupt frame", "S3S_CODEC_ZSTD", "IO encryption", "streaming map side",
                   "host mirror", "batched feed"):
        assert needle in header, needle


def test_python_binding_shapes():
    import ctypes

    import s3shuffle
    from s3shuffle import codec

    assert [f[0] for f in codec.StreamResult._fields_] == ["consumed", "out_len", "need_comp", "need_dst", "bad_partition", "at_end"]
    assert ctypes.sizeof(codec.StreamResult) == 40  # 4 x int64 + 2 x int32, as the C struct
    for m in ("feed", "feed_device", "position", "close", "__enter__", "__exit__"):
        assert hasattr(s3shuffle.DecodeStream, m), m
    for m in ("checksum_ranges_seeded", "checksum_ranges_seeded_device", "decode_stream"):
        assert hasattr(s3shuffle.Codec, m), m


def test_feed_refuses_a_destination_the_library_would_overrun(codec_lib):
    """DecodeStream.feed hands dst's address and a capacity to the library: the capacity may not exceed the array, and the
    array must be the bytes the address names (uint8, C-contiguous, writable).  Checked before the stream is touched."""
    import s3shuffle

    s = s3shuffle.DecodeStream.__new__(s3shuffle.DecodeStream)
    s._s, s._ctx, s._lib = None, None, codec_lib
    comp = np.zeros(8, np.uint8)
    read_only = np.zeros(16, np.uint8)
    read_only.flags.writeable = False
    for dst, cap in ((np.zeros(16, np.uint8), 17), (np.zeros(16, np.uint8), -1), (np.zeros(32, np.uint8)[::2], None),
                     (np.zeros(4, np.int32), None), (read_only, None), (bytearray(16), None)):
        with pytest.raises(ValueError, match="dst"):
            s.feed(comp, dst, cap)
    with pytest.raises(ValueError, match="closed"):  # a destination that passes reaches the stream
        s.feed(comp, np.zeros(16, np.uint8), 16)


# ---- JNI: the new natives against the mock JNIEnv ----------------------------------------------------------------------
BASE = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-g", "-I", MOCK, "-I", os.path.join(ROOT, "include")]


def _build(tmp_path, shim, name):
    exe = str(tmp_path / name)
    subprocess.run(BASE + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", shim,
                           os.path.join(MOCK, "jni_exec_stream.c"), os.path.join(MOCK, "fake_codec.c"),
                           os.path.join(MOCK, "fake_stream_codec.c"), "-o", exe], check=True)
    return exe


def _run(exe, leaks=1):
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=%d" % leaks))


def test_stream_natives_execute_against_the_mock_jvm(tmp_path):
    r = _run(_build(tmp_path, JNI_C, "jni_exec_stream"))
    assert r.returncode == 0 and "jni_exec_stream ok" in r.stdout, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("old,new", [
    ("  o[5] = r.at_end;\n  unpin(e, out, o, 0);", "  o[5] = r.at_end;\n  unpin(e, out, o, JNI_ABORT);"),
    ("  unpin(e, outStream, os, 0);", "  unpin(e, outStream, os, JNI_ABORT);"),
    ("cp ? cp + compOff : NULL", "cp"),
    ("  unpin(e, seeds, sd, JNI_ABORT);\n  unpin(e, out, o, 0);", "  unpin(e, out, o, 0);"),
    ("compOff > (*e)->GetDirectBufferCapacity(e, comp) - compLen", "0"),
    ("dstCap > (*e)->GetDirectBufferCapacity(e, dst)", "0"),
    ("of[n] > (*e)->GetDirectBufferCapacity(e, data)", "0"),
], ids=["result-not-copied-back", "stream-handle-not-copied-back", "window-offset-dropped", "seeds-left-pinned",
        "window-beyond-its-buffer", "capacity-beyond-its-buffer", "ranges-beyond-their-buffer"])
def test_the_harness_sees_a_broken_stream_native(tmp_path, old, new):
    src = open(JNI_C).read()
    assert src.count(old) == 1
    mutant = tmp_path / "s3s_jni_mutant.c"
    mutant.write_text(src.replace(old, new, 1))
    r = _run(_build(tmp_path, str(mutant), "jni_exec_stream_mutant"), leaks=0)
    # a CHECK of the harness fails, or - a window past its buffer - AddressSanitizer stops the stand-in library's read
    assert r.returncode != 0 and ("FAILED" in r.stdout or "AddressSanitizer" in r.stderr), (r.stdout, r.stderr[-2000:])


def test_jni_unit_loads_without_the_stream_symbols(tmp_path):
    """the library symbols are weak in the JNI unit: linked with a library from before the streams (fake_codec.c alone) the unit
    still links, and the natives answer S3S_E_UNSUPPORTED - the answer S3GpuBlockDecoder uses to keep the JVM stack"""
    main = tmp_path / "main.c"
    main.write_text('#include "mock_jvm.h"\n#include <stdio.h>\n'
                    "#define FN(n) Java_org_apache_spark_shuffle_gpu_S3SCodec_00024_##n\n"
                    "jint FN(dstreamOpen)(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jlongArray, jint, jlongArray);\n"
                    "jint FN(dstreamClose)(JNIEnv*, jclass, jlong);\n"
                    "int main(void) { JNIEnv* e = &mj_env; jlongArray a = mj_longs(2), o = mj_longs(1);\n"
                    "  int rc = FN(dstreamOpen)(e, NULL, 0, 1, 0, a, NULL, 1, o); int rc2 = FN(dstreamClose)(e, NULL, 0);\n"
                    '  printf("%d %d %d\\n", rc, rc2, mj_outstanding()); mj_free(a); mj_free(o); return 0; }\n')
    exe = str(tmp_path / "weak")
    subprocess.run(BASE + [JNI_C, str(main), os.path.join(MOCK, "fake_codec.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == ["-6", "-6", "0"], (r.stdout, r.stderr)


# ---- Scala text -----------------------------------------------------------------------------------------------------------
def test_scala_text_names_the_natives_the_jni_unit_defines():
    c_src = re.sub(r"/\*.*?\*/", "", open(JNI_C).read(), flags=re.S)
    defined = set(re.findall(r"FN\((\w+)\)\s*\(", c_src))
    codec = open(os.path.join(SHIM, "S3SCodec.scala")).read()
    declared = set(re.findall(r"@native def (\w+)\(", codec))
    for n in NATIVES:
        assert n in defined and n in declared, n
    dec = open(os.path.join(SHIM, "S3GpuBlockDecoder.scala")).read()
    used = set(re.findall(r"S3SCodec\.(dstream\w+|checksumRangesSeeded)", dec))
    assert {"dstreamOpen", "dstreamFeed", "dstreamClose"} <= used <= defined
    assert re.search(r"final class S3GpuStreamingInputStream\b.*?extends InputStream", dec, re.S)
    assert '"spark.shuffle.s3.gpu.streamWindowBytes"' in dec
    # accepts() and decode() stream where they fell back to the JVM stack for size
    assert 'n <= S3GpuBuffers.MaxBuffer || d.gpuReadCodec != "zstd"' in dec
    assert "if (compLen > S3GpuBuffers.MaxBuffer) return streamed(stream)" in dec
    assert "return streamed(new S3GpuStreams.DirectBufferInputStream(comp, compLen))" in dec
    # E_UNSUPPORTED at open keeps the JVM stack; errors go through S3SCodec.check with the range's first partition added
    assert "if (rc == S3SCodec.E_UNSUPPORTED) None" in dec and ".getOrElse(jvmPath(in))" in dec
    assert "firstPartition + result(4).toInt" in dec


# ---- seed arithmetic ------------------------------------------------------------------------------------------------------
def _mul(a, b, poly):
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (poly if b & 1 else 0)
    return p


def _x8n(n, poly):
    """x^(8 n) mod P in the reflected representation (checksum.hip: x8n)"""
    p, sq, n = 0x80000000, 0x40000000, 8 * n  # 1, x
    while n:
        if n & 1:
            p = _mul(sq, p, poly)
        sq = _mul(sq, sq, poly)
        n >>= 1
    return p


def seed_step(algo, seed, own, length):
    """checksum_seed_kernel restated: the seed as one more leading term of the combine"""
    if algo == 1:
        rem, a1, b1, a2, b2 = length % 65521, seed & 0xFFFF, seed >> 16, own & 0xFFFF, own >> 16
        return ((rem * a1 + b1 + b2 + 65521 - rem) % 65521) << 16 | (a1 + a2 + 65521 - 1) % 65521
    return _mul(_x8n(length, 0xEDB88320 if algo == 2 else 0x82F63B78), seed, 0xEDB88320 if algo == 2 else 0x82F63B78) ^ own


def _crc32c(b, crc=0):
    crc ^= 0xFFFFFFFF
    for x in b:
        crc ^= x
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


@pytest.mark.parametrize("algo", [1, 2, 3], ids=["adler32", "crc32", "crc32c"])
def test_seed_step_is_the_combine_identity(algo):
    """crc32_combine(crc(X), crc(Y), |Y|) = crc(X || Y) and adler32_combine likewise: the seed step on the host, and the
    compiled kernel through the gfx950 interpreter, against the checksum of the concatenation"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "isa"))
    import stream_kernel as sk

    f = {1: zlib.adler32, 2: zlib.crc32, 3: _crc32c}[algo]
    rng = np.random.default_rng(algo)
    buf = rng.integers(0, 256, 40_000 if algo != 3 else 3_000, dtype=np.uint8).tobytes()
    n = len(buf)
    cases = [(0, 0), (0, 1), (1, 1), (0, n), (n, n), (1, n), (n // 2, n), (n - 1, n), (777, 778), (5, 5)]
    seeds, owns, lens, want = [], [], [], []
    for split, end in cases:
        x, y = buf[:split], buf[split:end]
        seeds.append(f(x)), owns.append(f(y)), lens.append(len(y)), want.append(f(x + y))
        assert seed_step(algo, seeds[-1], owns[-1], lens[-1]) == want[-1], (split, end)
    assert seed_step(algo, 0xDEADBEEF if algo != 1 else (4321 << 16 | 1234), f(b""), 0) == (0xDEADBEEF if algo != 1 else (4321 << 16 | 1234))
    # the compiled kernel on the same cases, one lane per case
    assert sk.checksum_seed(algo, lens, seeds, owns) == want
    # the long-range powers: x^(8 n) for n = 2^29 + 3 (CRC-32C's table wraps differently there, checksum.hip x8n) - the kernel
    # against the host restatement, with own = 0 so that the result is the shifted seed alone
    if algo != 1:
        big = (1 << 29) + 3
        assert sk.checksum_seed(algo, [big], [0x12345678], [0]) == [seed_step(algo, 0x12345678, 0, big)]
