"""Spark's IO encryption layer (CryptoStreamUtils.createCryptoOutputStream, AES/CTR/NoPadding) restated in Python on top of
the host build of the product's AES-CTR core (tests/aes_ctr_model_lib.py).  Parity with a JVM is unpinned: neither Spark nor
commons-crypto is available to the tests, so this is the format as DESIGN.md 6h states it:

  a non-empty partition is stored as   IV (16 bytes) | AES-CTR_K(codec bytes of the partition)
  an empty partition stays 0 bytes (no stream is opened, no IV is written)
  a partition is ONE encrypted stream whatever its segments were: the IV belongs to the partition
  checksums and index cover IV plus cipher text

encrypt_image turns a plain .data image, its index and one IV per partition into the encrypted image and index;
checksums gives java.util.zip's values over the stored bytes; decrypt_image is the inverse."""
import zlib

import numpy as np

import aes_ctr_model_lib as acm

IV_BYTES = 16
ADLER32, CRC32, CRC32C = 1, 2, 3


def _ivs(ivs, n):
    a = np.frombuffer(bytes(ivs), dtype=np.uint8) if not isinstance(ivs, np.ndarray) else np.ascontiguousarray(ivs, dtype=np.uint8)
    a = a.reshape(-1)
    assert a.size == IV_BYTES * n, "one 16-byte IV per partition (empty ones included)"
    return a.reshape(n, IV_BYTES)


def encrypt_image(image, index, key, ivs):
    """(encrypted image uint8, encrypted index int64) of the plain image / index (n + 1 cumulative offsets)."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    index = np.asarray(index, dtype=np.int64)
    n = len(index) - 1
    iv = _ivs(ivs, n)
    parts, out_index = [], [0]
    for p in range(n):
        body = image[index[p]:index[p + 1]]
        if body.size:
            parts.append(iv[p])
            parts.append(acm.xor_stream(key, iv[p].tobytes(), body))
        out_index.append(out_index[-1] + (body.size + IV_BYTES if body.size else 0))
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return out, np.asarray(out_index, dtype=np.int64)


def decrypt_image(enc_image, enc_index, key):
    """(plain image, plain index); a non-empty partition shorter than an IV is an error."""
    enc_image = np.ascontiguousarray(enc_image, dtype=np.uint8)
    enc_index = np.asarray(enc_index, dtype=np.int64)
    parts, out_index = [], [0]
    for p in range(len(enc_index) - 1):
        stored = enc_image[enc_index[p]:enc_index[p + 1]]
        if stored.size == 0:
            out_index.append(out_index[-1])
            continue
        if stored.size < IV_BYTES:
            raise ValueError("partition %d: %d stored bytes, shorter than the IV" % (p, stored.size))
        parts.append(acm.xor_stream(key, stored[:IV_BYTES].tobytes(), stored[IV_BYTES:]))
        out_index.append(out_index[-1] + stored.size - IV_BYTES)
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return out, np.asarray(out_index, dtype=np.int64)


_CRC32C_TABLE = None


def crc32c(data):
    """java.util.zip.CRC32C (Castagnoli, reflected 0x82F63B78)."""
    global _CRC32C_TABLE
    if _CRC32C_TABLE is None:
        t = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            t.append(c)
        _CRC32C_TABLE = t
    c = 0xFFFFFFFF
    t = _CRC32C_TABLE
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def checksums(image, index, algo):
    """java.util.zip Adler32 / CRC32 / CRC32C getValue() of every partition's stored bytes, int64[n]."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    fn = {ADLER32: lambda b: zlib.adler32(b) & 0xFFFFFFFF, CRC32: lambda b: zlib.crc32(b) & 0xFFFFFFFF, CRC32C: crc32c}[algo]
    return np.asarray([fn(image[index[p]:index[p + 1]].tobytes()) for p in range(len(index) - 1)], dtype=np.int64)


def encrypt_map_output(image, index, key, ivs, algo=None):
    """(encrypted image, index, checksums or None): what a map task stores with spark.io.encryption.enabled."""
    img, idx = encrypt_image(image, index, key, ivs)
    return img, idx, (checksums(img, idx, algo) if algo else None)
