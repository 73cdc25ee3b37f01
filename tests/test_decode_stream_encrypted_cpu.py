"""CPU: streams under IO encryption (s3s_dstream_open_encrypted) as far as they go without a GPU, next to
tests/test_aes_ctr_stream_cpu.py (the kernel's arithmetic and the header): the new native of jni/s3s_jni.c against the mock
JNIEnv, with mutants that drop its argument checks; the Scala text; and the test helpers themselves - the stored unit list
and the analytic S3S_CODEC_NONE expectation against su.expected_feed."""
import os
import re
import subprocess

import numpy as np
import pytest

import stream_units as su
import stream_units_encrypted as sue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock_jni")
JNI_C = os.path.join(ROOT, "jni", "s3s_jni.c")
SHIM = os.path.join(ROOT, "scala", "org", "apache", "spark", "shuffle", "gpu")
BASE = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-g", "-I", MOCK, "-I", os.path.join(ROOT, "include")]


def _build(tmp_path, shim, name):
    exe = str(tmp_path / name)
    subprocess.run(BASE + ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", shim,
                           os.path.join(MOCK, "jni_exec_stream_enc.c"), os.path.join(MOCK, "fake_codec.c"),
                           os.path.join(MOCK, "fake_stream_codec.c"), os.path.join(MOCK, "fake_stream_enc_codec.c"), "-o", exe], check=True)
    return exe


def _run(exe, leaks=1):
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=%d" % leaks))


def test_native_executes_against_the_mock_jvm(tmp_path):
    r = _run(_build(tmp_path, JNI_C, "jni_exec_stream_enc"))
    assert r.returncode == 0 and "jni_exec_stream_enc ok" in r.stdout, (r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("old,new", [
    ("partOffsets && (*e)->GetArrayLength(e, partOffsets) < nparts + 1", "0"),
    ("refChecksums && (*e)->GetArrayLength(e, refChecksums) < nparts", "0"),
    ("!outStream || (*e)->GetArrayLength(e, outStream) < 1", "0"),
    ("return dstream_open(e, s3s_dstream_open_encrypted, h,", "return dstream_open(e, s3s_dstream_open, h,"),
], ids=["offsets-shorter-than-nparts", "checksums-shorter-than-nparts", "no-room-for-the-handle", "the-plain-entry-point"])
def test_the_harness_sees_a_native_without_its_checks(tmp_path, old, new):
    src = open(JNI_C).read()
    assert src.count(old) == 1
    mutant = tmp_path / "s3s_jni_mutant.c"
    mutant.write_text(src.replace(old, new, 1))
    r = _run(_build(tmp_path, str(mutant), "jni_exec_stream_enc_mutant"), leaks=0)
    # a CHECK of the harness fails, or AddressSanitizer stops the stand-in library's read past a Java array
    assert r.returncode != 0 and ("FAILED" in r.stdout or "AddressSanitizer" in r.stderr), (r.stdout, r.stderr[-2000:])


def test_native_answers_unsupported_without_the_symbol(tmp_path):
    """the symbol is weak on its own: a library that has the streams but not this entry point (fake_codec.c +
    fake_stream_codec.c) links, dstreamOpen works and dstreamOpenEncrypted answers S3S_E_UNSUPPORTED - the caller keeps the JVM"""
    main = tmp_path / "main.c"
    main.write_text('#include "mock_jvm.h"\n#include <stdio.h>\n'
                    "#define FN(n) Java_org_apache_spark_shuffle_gpu_S3SCodec_00024_##n\n"
                    "jlong FN(create)(JNIEnv*, jclass, jint, jlong);\nvoid FN(destroy)(JNIEnv*, jclass, jlong);\n"
                    "jint FN(dstreamOpen)(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jlongArray, jint, jlongArray);\n"
                    "jint FN(dstreamOpenEncrypted)(JNIEnv*, jclass, jlong, jint, jint, jlongArray, jlongArray, jint, jlongArray);\n"
                    "jint FN(dstreamClose)(JNIEnv*, jclass, jlong);\n"
                    "int main(void) { JNIEnv* e = &mj_env; jlongArray a = mj_longs(2), o = mj_longs(1); jlong h = FN(create)(e, NULL, 0, 0);\n"
                    "  int rc = FN(dstreamOpenEncrypted)(e, NULL, h, 1, 0, a, NULL, 1, o); long long got = mj_l(o)[0];\n"
                    "  int rc2 = FN(dstreamOpen)(e, NULL, h, 1, 0, a, NULL, 1, o); FN(dstreamClose)(e, NULL, mj_l(o)[0]); FN(destroy)(e, NULL, h);\n"
                    '  printf("%d %lld %d %d\\n", rc, got, rc2, mj_outstanding()); mj_free(a); mj_free(o); return 0; }\n')
    exe = str(tmp_path / "weak_enc")
    subprocess.run(BASE + [JNI_C, str(main), os.path.join(MOCK, "fake_codec.c"), os.path.join(MOCK, "fake_stream_codec.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.stdout.split() == ["-6", "0", "0", "0"], (r.stdout, r.stderr)


def test_scala_text_declares_the_native_and_picks_it_by_key_bits():
    c_src = re.sub(r"/\*.*?\*/", "", open(JNI_C).read(), flags=re.S)
    assert "dstreamOpenEncrypted" in set(re.findall(r"FN\((\w+)\)\s*\(", c_src))
    codec = open(os.path.join(SHIM, "S3SCodec.scala")).read()
    sig = re.search(r"@native def dstreamOpenEncrypted\(([^)]*)\): Int", codec)
    plain = re.search(r"@native def dstreamOpen\(([^)]*)\): Int", codec)
    assert sig and plain and re.sub(r"\s+", " ", sig.group(1)) == re.sub(r"\s+", " ", plain.group(1))
    dec = open(os.path.join(SHIM, "S3GpuBlockDecoder.scala")).read()
    body = dec[dec.index("def open(blockName: String"):]
    body = body[:body.index("final class S3GpuStreamingInputStream")]
    assert re.search(r"val encrypted = S3SCodec\.getOption\(ctx, S3SCodec\.OPT_IO_ENCRYPTION_KEY_BITS\) > 0", body)
    assert re.search(r"if \(encrypted\) S3SCodec\.dstreamOpenEncrypted\(ctx, codec, algo, rel, refs, rel\.length - 1, handle\)\s*"
                     r"else S3SCodec\.dstreamOpen\(ctx, codec, algo, rel, refs, rel\.length - 1, handle\)", body)
    assert "if (rc == S3SCodec.E_UNSUPPORTED) None" in body  # a library from before the entry point: the JVM stack
    # encrypted ranges are no longer listed as out of scope for streams
    for text in (dec, codec):
        for line in text.splitlines():
            if "ut of scope" in line:
                assert "encryption" not in line, line


# ---- the helpers of the GPU tests ------------------------------------------------------------------------------------------
def _toy():
    """a NONE image: partitions of 0, 40, 1, 0, 33 plain bytes and one stored as its IV alone"""
    rng = np.random.default_rng(3)
    sizes = [0, 40, 1, 0, 33, 0]
    img = rng.integers(0, 256, sum(sizes), dtype=np.uint8)
    index = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return img, index


def test_stored_units_and_the_reference_layer():
    img, index = _toy()
    key = sue.KEYS[24]
    ivs = sue.ivs_for(6, 1)
    enc, eidx, sums = sue.encrypt(img, index, key, ivs, iv_only={5}, algo=2)
    assert [int(x) for x in np.diff(eidx)] == [0, 56, 17, 0, 49, 16] and sums is not None
    import spark_crypto_ref as scr

    back, bidx = scr.decrypt_image(enc, eidx, key)
    assert np.array_equal(back, img) and np.array_equal(bidx, index)
    assert sue.plain_index(eidx) == [int(x) for x in index]
    u = sue.stored_units(su.NONE, img.tobytes(), eidx)
    ivs_at = [x[0] for x in u if x[1] == 16 and x[2] == 0]
    assert ivs_at == [0, 56, 73, 122] and sum(x[2] for x in u) == img.size
    covered = sorted((x[0], x[0] + x[1]) for x in u)
    assert covered[0][0] == 0 and covered[-1][1] == int(eidx[-1]) and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))


def test_analytic_none_expectation_is_expected_feed():
    img, index = _toy()
    enc, eidx, _ = sue.encrypt(img, index, sue.KEYS[16], sue.ivs_for(6, 2), iv_only={5})
    u = sue.stored_units(su.NONE, img.tobytes(), eidx)
    total = int(eidx[-1])
    for pos in [x[0] for x in u] + [total]:
        if any(eidx[p] < pos < eidx[p] + 16 for p in range(len(eidx) - 1) if eidx[p + 1] > eidx[p]):
            continue  # (never a position: inside an IV)
        for w in range(0, total - pos + 1):
            for cap in (0, 1, 7, 16, 33, 40, 41, 1000):
                assert sue.expected_feed_none(eidx, pos, w, cap) == su.expected_feed(u, pos, w, cap), (pos, w, cap)
