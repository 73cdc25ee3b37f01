"""The units of a stream under IO encryption (s3s_dstream_open_encrypted, include/s3shuffle_codec.h) on top of
tests/stream_units.py: the codec's units of the plain stream, each shifted by the IVs in front of it, plus one 16-byte unit of
no output per non-empty stored partition - its IV.  su.expected_feed over that list is what a feed may take.  Encrypted images
come from tests/spark_crypto_ref.py (the reference layer over the host build of the AES-CTR core), never from the code under
test.  Test infrastructure for tests/test_gpu_decode_stream_encrypted.py and tests/test_decode_stream_encrypted_cpu.py."""
from __future__ import annotations

import bisect
from typing import List, Tuple

import numpy as np

import spark_crypto_ref as scr
import stream_units as su

IV = 16
KEYS = {16: bytes(range(16)), 24: bytes(range(100, 124)), 32: bytes(range(7, 39))}


def ivs_for(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, IV), dtype=np.uint8)


def encrypt(img, index, key, ivs, iv_only=(), algo=0):
    """The reference layer over a plain image -> (stored image, stored index, checksums or None).  iv_only: partitions (empty
    in the plain image) that are stored as their IV alone - 16 stored bytes, an empty stream."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    index = [int(x) for x in index]
    enc, eidx = scr.encrypt_image(img, index, key, ivs)
    if iv_only:
        parts, out_index = [], [0]
        for p in range(len(index) - 1):
            body = enc[eidx[p]:eidx[p + 1]]
            if p in iv_only:
                assert body.size == 0
                body = np.asarray(ivs, np.uint8).reshape(-1, IV)[p]
            parts.append(body)
            out_index.append(out_index[-1] + body.size)
        enc, eidx = np.concatenate(parts).astype(np.uint8), np.asarray(out_index, np.int64)
    return enc, np.asarray(eidx, np.int64), (scr.checksums(enc, eidx, algo) if algo else None)


def plain_index(enc_index) -> List[int]:
    out = [0]
    for p in range(len(enc_index) - 1):
        ln = int(enc_index[p + 1]) - int(enc_index[p])
        out.append(out[-1] + (ln - IV if ln >= IV else 0))
    return out


def stored_units(codec: int, plain_img: bytes, enc_index) -> List[Tuple[int, int, int]]:
    """[(stored start, length, decoded)] of a well-formed encrypted range whose plain image is plain_img.  S3S_CODEC_NONE: one
    unit per byte, as in su.units."""
    pidx = plain_index(enc_index)
    out = []
    for p in range(len(enc_index) - 1):
        a, b = int(enc_index[p]), int(enc_index[p + 1])
        if b == a:
            continue
        assert b - a >= IV
        out.append((a, IV, 0))
        shift = a + IV - pidx[p]
        out += [(s + shift, ln, dec) for s, ln, dec in su.units(codec, plain_img, [pidx[p], pidx[p + 1]])]
    return out


def to_stored(enc_index, x: int) -> int:
    """The stored offset of plain offset x: 16 more for every IV passed; an IV in front of the next plain byte is passed."""
    pidx = plain_index(enc_index)
    p = bisect.bisect_right(pidx, x) - 1
    p = min(p, len(enc_index) - 2)
    ln = int(enc_index[p + 1]) - int(enc_index[p])
    return int(enc_index[p]) + (IV if ln >= IV else 0) + (x - pidx[p])


def expected_feed_none(enc_index, pos: int, window_len: int, dst_capacity: int) -> Tuple[int, int]:
    """su.expected_feed over stored_units(NONE, ...) without the list (a unit per byte is too many for an image of 100 KB):
    IVs whole in the window are taken, bytes while they fit dst_capacity.  tests/test_decode_stream_encrypted_cpu.py holds it
    against su.expected_feed on small images."""
    wend, at, out = pos + window_len, pos, 0
    for p in range(len(enc_index) - 1):
        a, b = int(enc_index[p]), int(enc_index[p + 1])
        if b <= pos or b == a:
            continue
        if a >= wend:
            break
        if at <= a:
            if a + IV > wend:
                break
            at = a + IV
        take = min(min(b, wend) - at, dst_capacity - out)
        at, out = at + take, out + take
        if at < b:
            break
    return at - pos, out
