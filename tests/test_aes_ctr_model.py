"""The AES-CTR core (spark-s3-shuffle_amd/csrc/aes_ctr_core.h) on the CPU, before the same code runs on the GPU: the FIPS-197
Appendix C block vectors and the SP 800-38A CTR vectors (F.5.1, F.5.3, F.5.5) for all three key sizes, the counter's carries
through all 16 bytes, seeking, equality with libcrypto's EVP aes-*-ctr (skipped with a reason only where the machine has no
libcrypto; the standards' vectors always run), the same cases once more through an AddressSanitizer / UBSan program whose
buffers are heap allocations of exactly the permitted sizes, the restated Spark layer (tests/spark_crypto_ref.py) on hand-built
cases, and the constants of the additive interface (key 11 everywhere, ABI still 11)."""
import os
import re
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))

import aes_ctr_model_lib as A  # noqa: E402
import spark_crypto_ref as R  # noqa: E402

h = bytes.fromhex

# FIPS-197 Appendix C.1 - C.3: PLAINTEXT 00112233445566778899aabbccddeeff, KEY 000102...
FIPS_PT = h("00112233445566778899aabbccddeeff")
FIPS = [(bytes(range(16)), h("69c4e0d86a7b0430d8cdb78070b4c55a")),
        (bytes(range(24)), h("dda97ca4864cdfe06eaf70a0ec0d7191")),
        (bytes(range(32)), h("8ea2b7ca516745bfeafc49904b496089"))]

# SP 800-38A F.5: initial counter block and the four plaintext blocks are the same for the three key sizes
SP_CTR = h("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
SP_PT = h("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"
          "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
SP = {"F.5.1": (h("2b7e151628aed2a6abf7158809cf4f3c"),
                h("874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff"
                  "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee")),
      "F.5.3": (h("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"),
                h("1abc932417521ca24f2b0459fe7e6e0b" "090339ec0aa6faefd5ccc2c6f4ce8e94"
                  "1e36b26bd1ebc670d1bd1d665620abf7" "4f78a7f6d29809585a97daec58c6b050")),
      "F.5.5": (h("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"),
                h("601ec313775789a5b7a7f504bbf3d228" "f443e3ca4d62b59aca84e990cacaf5c5"
                  "2b0930daa23de94ce87017ba2d84988d" "dfc9c58db67aada613c2dd08457941a6"))}


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


@pytest.mark.parametrize("key,ct", FIPS, ids=["aes128", "aes192", "aes256"])
def test_fips197_appendix_c(key, ct):
    assert A.encrypt_block(key, FIPS_PT) == ct
    nr, rk = A.expand_key(key)
    assert nr == {16: 10, 24: 12, 32: 14}[len(key)] and rk.size == 4 * (nr + 1)


def test_key_expansion_fips197_appendix_a1():
    # A.1: the last round key of 2b7e1516 28aed2a6 abf71588 09cf4f3c is d014f9a8 c9ee2589 e13f0cc8 b6630ca6
    nr, rk = A.expand_key(SP["F.5.1"][0])
    assert nr == 10 and [int(w) for w in rk[40:44]] == [0xd014f9a8, 0xc9ee2589, 0xe13f0cc8, 0xb6630ca6]
    assert A.expand_key(bytes(17))[0] == 0 and A.expand_key(b"")[0] == 0


@pytest.mark.parametrize("name", sorted(SP))
def test_sp800_38a_ctr(name):
    key, ct = SP[name]
    assert _xor(SP_PT, A.keystream(key, SP_CTR, 0, 64)) == ct
    for b in range(4):  # every block on its own: the stream is seekable
        assert _xor(SP_PT[16 * b:16 * b + 16], A.keystream(key, SP_CTR, 16 * b, 16)) == ct[16 * b:16 * b + 16]
    assert A.xor_stream(key, SP_CTR, ct).tobytes() == SP_PT


def test_counter_carries_through_all_sixteen_bytes():
    ones, zeros = b"\xff" * 16, bytes(16)
    assert A.counter_add(ones, 1) == zeros
    assert A.counter_add(bytes(8) + b"\xff" * 8, 1) == bytes(7) + b"\x01" + bytes(8)  # carries into byte 7
    assert A.counter_add(bytes(8) + b"\xff" * 7 + b"\xf0", 0x10) == bytes(7) + b"\x01" + bytes(8)
    assert A.counter_add(b"\xff" * 8 + bytes(8), (1 << 64) - 1) == b"\xff" * 16
    for key in (bytes(range(16)), bytes(range(24)), bytes(range(32))):
        assert A.keystream(key, ones, 16, 16) == A.keystream(key, zeros, 0, 16)  # block 1 of ff..ff is block 0 of 00..00
        low = bytes(8) + b"\xff" * 8
        assert A.keystream(key, low, 16, 16) == A.keystream(key, bytes(7) + b"\x01" + bytes(8), 0, 16)
        assert A.keystream(key, low, 16, 16) == A.encrypt_block(key, bytes(7) + b"\x01" + bytes(8))


@pytest.mark.parametrize("kb", [16, 24, 32])
def test_seek_equals_slice(kb):
    rng = np.random.default_rng(kb)
    key, iv = rng.bytes(kb), rng.bytes(16)
    whole = A.keystream(key, iv, 0, 47 + 100)
    for o in range(48):
        for n in (0, 1, 15, 16, 17, 33, 100):
            assert A.keystream(key, iv, o, n) == whole[o:o + n], (o, n)
    far = (1 << 36) + 5  # block numbers beyond 32 bits
    assert A.keystream(key, iv, far, 40) == A.keystream(key, A.counter_add(iv, far // 16), far % 16, 40)


@pytest.mark.parametrize("kb", [16, 24, 32])
def test_equals_libcrypto_evp(kb):
    if A.libcrypto() is None:
        pytest.skip("ctypes.util.find_library('crypto') finds no libcrypto on this machine")
    rng = np.random.default_rng(100 + kb)
    for n in list(range(101)) + [65537]:
        key, iv, data = rng.bytes(kb), rng.bytes(16), rng.bytes(n)
        assert A.xor_stream(key, iv, data).tobytes() == A.evp_ctr(key, iv, data), n
    for iv in (b"\xff" * 16, bytes(8) + b"\xff" * 8, bytes(8) + b"\xff" * 7 + b"\xf0", b"\xff" * 15 + b"\xfe"):
        key, data = rng.bytes(kb), rng.bytes(300)
        assert A.xor_stream(key, iv, data).tobytes() == A.evp_ctr(key, iv, data), iv.hex()
    for name, (key, ct) in SP.items():
        if len(key) == kb:
            assert A.evp_ctr(key, SP_CTR, SP_PT) == ct, name


def test_sanitised_program_writes_the_same_key_streams(tmp_path):
    rng = np.random.default_rng(5)
    cases = [(SP[n][0], SP_CTR, 0, 64) for n in sorted(SP)]
    for kb in (16, 24, 32):
        for n in (0, 1, 15, 16, 17, 100, 65537):
            cases.append((rng.bytes(kb), rng.bytes(16), int(rng.integers(0, 48)), n))
        cases.append((rng.bytes(kb), b"\xff" * 16, 7, 50))
        cases.append((rng.bytes(kb), bytes(8) + b"\xff" * 8, (1 << 40) + 3, 50))
    got = A.run_asan(cases, str(tmp_path))
    for (key, iv, off, n), g in zip(cases, got):
        assert g == A.keystream(key, iv, off, n)
    for name, g in zip(sorted(SP), got):
        assert _xor(SP_PT, g) == SP[name][1]


# ---- the restated Spark layer ------------------------------------------------------------------------------------------
def _layer_case():
    rng = np.random.default_rng(9)
    key = rng.bytes(16)
    # partitions: empty | 1 byte | empty | 40 bytes made of three segments (5 + 0 + 35: the layer sees the concatenation) | empty
    image = np.frombuffer(rng.bytes(41), dtype=np.uint8)
    index = np.array([0, 0, 1, 1, 41, 41], dtype=np.int64)
    ivs = np.frombuffer(rng.bytes(16 * 5), dtype=np.uint8)
    return key, image, index, ivs


def test_layer_hand_built_cases():
    key, image, index, ivs = _layer_case()
    enc, eidx = R.encrypt_image(image, index, key, ivs)
    assert eidx.tolist() == [0, 0, 17, 17, 73, 73]  # an empty partition stays 0 bytes, a non-empty one grows by its IV
    iv1, iv3 = ivs[16:32].tobytes(), ivs[48:64].tobytes()
    assert enc[0:16].tobytes() == iv1 and enc[17:33].tobytes() == iv3
    assert enc[16] == image[0] ^ A.keystream(key, iv1, 0, 1)[0]
    # ONE key stream over the partition of several segments: byte 5 (the second segment's first) continues at offset 5
    assert enc[33:73].tobytes() == _xor(image[1:41].tobytes(), A.keystream(key, iv3, 0, 40))
    assert enc[33 + 5:73].tobytes() == _xor(image[6:41].tobytes(), A.keystream(key, iv3, 5, 35))
    if A.libcrypto() is not None:
        assert enc[33:73].tobytes() == A.evp_ctr(key, iv3, image[1:41].tobytes())
    back, bidx = R.decrypt_image(enc, eidx, key)
    assert np.array_equal(back, image) and bidx.tolist() == index.tolist()
    sums = R.checksums(enc, eidx, R.ADLER32)
    assert sums.tolist() == [1, zlib.adler32(enc[0:17].tobytes()), 1, zlib.adler32(enc[17:73].tobytes()), 1]
    assert R.checksums(enc, eidx, R.CRC32)[1] == zlib.crc32(enc[0:17].tobytes())
    assert R.crc32c(b"123456789") == 0xE3069283 and R.checksums(enc, eidx, R.CRC32C)[0] == 0
    img2, idx2, s2 = R.encrypt_map_output(image, index, key, ivs, R.CRC32)
    assert np.array_equal(img2, enc) and np.array_equal(idx2, eidx) and s2[3] == zlib.crc32(enc[17:73].tobytes())


def test_layer_refuses_a_stored_partition_shorter_than_an_iv():
    key, image, index, ivs = _layer_case()
    enc, eidx = R.encrypt_image(image, index, key, ivs)
    with pytest.raises(ValueError):
        R.decrypt_image(enc[:7], np.array([0, 7], dtype=np.int64), key)
    back, bidx = R.decrypt_image(enc[:16], np.array([0, 16], dtype=np.int64), key)  # exactly an IV: an empty stream
    assert back.size == 0 and bidx.tolist() == [0, 0]
    with pytest.raises(AssertionError):
        R.encrypt_image(image, index, key, ivs[:16 * 4])


# ---- constants of the additive interface ----------------------------------------------------------------------------------
def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_key_11_and_abi_11_everywhere():
    from s3shuffle import codec

    header = _read("include", "s3shuffle_codec.h")
    scala = _read("scala", "org", "apache", "spark", "shuffle", "gpu", "S3SCodec.scala")
    assert int(re.search(r"S3S_OPT_IO_ENCRYPTION_KEY_BITS\s*=\s*(\d+)", header).group(1)) == 11
    assert int(re.search(r"val OPT_IO_ENCRYPTION_KEY_BITS = (\d+)", scala).group(1)) == 11
    assert codec.OPT_IO_ENCRYPTION_KEY_BITS == 11
    abi = int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1))
    assert abi == 11 and int(re.search(r"val ABI_VERSION = (\d+)", scala).group(1)) == 11
    keys = [int(m) for m in re.findall(r"^\s+S3S_OPT_\w+ = (\d+)", header, re.M)]
    assert 11 in keys and len(keys) == len(set(keys)), "two options share a key"
    for sym in ("s3s_set_io_encryption", "s3s_set_stream_ivs"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _read("jni", "s3s_jni.c")
    for native in ("setIoEncryption", "setStreamIvs"):
        assert native in scala and native in _read("jni", "s3s_jni.c")


# ---- the inputs of the GPU tests: checked here, on the CPU, so that they cannot hide the cases they are there for --------------
def test_gpu_test_inputs_cover_the_residues_and_the_tile_edges(oracle):
    import io_encryption_inputs as I

    data, offs = I.words_input()
    assert len(offs) - 1 == 20 and int(np.sum(np.diff(offs) == 0)) >= 4
    img, index, _ = oracle.compress_map_output(oracle.CODEC_LZ4, 0, data, offs)
    _, eidx = R.encrypt_image(img, index, I.KEYS[16], I.ivs_for(offs))
    starts = {int(eidx[p]) % 16 for p in range(20) if eidx[p + 1] > eidx[p]}
    assert len(starts) >= 8, sorted(starts)
    ivs = I.ivs_for(offs).reshape(-1, 16)
    assert any(bytes(v) == I.IV_ONES for v in ivs) and any(bytes(v) == I.IV_LOW_CARRY for v in ivs)
    data, offs = I.none_sizes_input()
    sizes = np.diff(offs).tolist()
    assert sizes[:12] == [1, 0, 15, 16, 17, 0, 0, 31, 4095, 4096, 4097, 70000]
    _, eidx = R.encrypt_image(data, offs, I.KEYS[16], I.ivs_for(offs))
    ends = [int(e) for e in eidx[1:]]
    assert any(e % I.TILE == 0 for e in ends), "a stream ends exactly on a tile edge"
    assert any(0 < (-int(s)) % I.TILE < 16 for s, e in zip(eidx[:-1], eidx[1:]) if e > s), "an IV straddles a tile edge"
    assert eidx[-1] > 6 * I.TILE
