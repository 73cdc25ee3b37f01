"""The units of the streaming reduce side (include/s3shuffle_codec.h, s3s_dstream_*) restated in a few lines of Python: where
the units of a range start, and what a feed may take from a window - the stop rule the stream-mode discovery kernels follow.
Test infrastructure for tests/test_gpu_decode_stream.py and tests/test_isa_decode_stream.py."""
from __future__ import annotations

import struct
from typing import List, Tuple

NONE, LZ4, SNAPPY, LZF = 0, 1, 2, 4
SNAPPY_MAGIC = b"\x82SNAPPY\x00"


def unit_at(codec: int, b: bytes, ip: int, end: int, at_partition_start: bool) -> Tuple[int, int, int]:
    """The unit that starts at b[ip] when only b[:end] is visible -> (visible, length, decoded): visible = 1 when the whole
    unit lies in front of `end`; else 0 and length = the smallest length known to hold it (the header's when the header is cut,
    else header + payload).  decoded = its decoded bytes (0 while unknown)."""
    def cut(n):
        return (0, n, 0)

    if codec == NONE:
        return (1, 1, 1)
    if codec == LZ4:
        if end - ip < 21:
            return cut(21)
        assert b[ip:ip + 8] == b"LZ4Block"
        cl, ol = struct.unpack_from("<ii", b, ip + 9)
        return (1, 21 + cl, ol) if 21 + cl <= end - ip else cut(21 + cl)
    if codec == SNAPPY:
        if at_partition_start or (end - ip >= 4 and b[ip:ip + 4] == SNAPPY_MAGIC[:4]):
            return (1, 16, 0) if end - ip >= 16 else cut(16)
        if end - ip < 4:
            return cut(4)
        cl = struct.unpack_from(">I", b, ip)[0]
        if 4 + cl > end - ip:
            return cut(4 + cl)
        ulen, sh, i = 0, 0, ip + 4
        while True:
            ulen |= (b[i] & 0x7F) << sh
            if not b[i] & 0x80:
                break
            i, sh = i + 1, sh + 7
        return (1, 4 + cl, ulen)
    if codec == LZF:
        if end - ip < 5:
            return cut(5)
        assert b[ip:ip + 2] == b"ZV"
        typ, ln = b[ip + 2], struct.unpack_from(">H", b, ip + 3)[0]
        if typ == 1 and end - ip < 7:
            return cut(7)
        head, ulen = (7, struct.unpack_from(">H", b, ip + 5)[0]) if typ == 1 else (5, ln)
        return (1, head + ln, ulen) if head + ln <= end - ip else cut(head + ln)
    raise ValueError(codec)


def units(codec: int, img: bytes, index) -> List[Tuple[int, int, int]]:
    """Every unit of a well-formed range: [(start, length, decoded)], partition by partition."""
    out = []
    for p in range(len(index) - 1):
        ip, end = int(index[p]), int(index[p + 1])
        first = True
        while ip < end:
            ok, ln, dec = unit_at(codec, img, ip, end, first and codec == SNAPPY)
            assert ok, (codec, p, ip)
            out.append((ip, ln, dec))
            ip, first = ip + ln, False
    return out


def expected_feed(unit_list, pos: int, window_len: int, dst_capacity: int) -> Tuple[int, int]:
    """What a feed takes: the longest prefix of whole units from `pos` inside [pos, pos + window_len) whose decoded bytes fit
    dst_capacity -> (consumed, out_len)."""
    consumed = out = 0
    for start, ln, dec in unit_list:
        if start < pos:
            continue
        if start + ln > pos + window_len or out + dec > dst_capacity:
            break
        consumed, out = start + ln - pos, out + dec
    return consumed, out


def lzf_cut_image(oracle, algo: int):
    """A small LZF image for the every-cut-position tests -> (data, offsets, img, index, sums): a stored chunk (300 random
    bytes), a partition of two compressed chunks (65535 + 2465 source bytes: dictionary words, then a short period) and a
    partition of one compressed chunk - a few KiB in all, so every cut position can be fed."""
    import numpy as np

    import corpus

    rng = np.random.default_rng(7)
    parts = [corpus.chunk_corpus(0, 300, rng), np.concatenate([corpus.chunk_corpus(3, 3_000, rng), corpus.chunk_corpus(5, 65_000, rng)]),
             corpus.chunk_corpus(3, 2_500, rng)]
    data = np.concatenate(parts).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    img, index, sums = oracle.compress_map_output(LZF, algo, data, offs)
    b = img.tobytes()
    ulist = units(LZF, b, index)
    assert [b[u[0] + 2] for u in ulist] == [0, 1, 1, 1] and img.size < 6_000, ([b[u[0] + 2] for u in ulist], img.size)
    return data, offs, img, index, sums
