"""liblz4's parse of inputs of 65 547 bytes and more (LZ4_compress_generic, noDict, byU32, acceleration 1, 64-bit host), restated
in Python, and the helpers the big-block tests share (TEST INFRASTRUCTURE: no oracle, no product).

`compress_u32(src)` returns the block payload and the number of table candidates the parse REFUSED because they lie more than
65 535 bytes back (the distance test), so that a test can say what its inputs exercise and a kernel diff can be localised to a
sequence.  tests/test_lz4_u32_ref.py pins it to the liblz4 of the machine.  Expected streams of the kernel tests come from
liblz4 itself (`jvm_stream`), never from this model.

Differences from the byU16 parse (inputs below 65 547 bytes):
  hash      ((read64le(p) << 24) * 889523592379) >> 52: twelve bits of the FIVE bytes at p
  table     4096 x u32, zero-initialised (entry 0 is position 0, a valid candidate)
  distance  the probe stores its position, then a candidate with cand + 65535 < pos is skipped without a compare
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

import framing

U32_FROM = 65536 + 11  # LZ4_64Klimit: the first input length liblz4 parses with the u32 table
_M64 = (1 << 64) - 1


def hash5(five_or_more: bytes) -> int:
    s = int.from_bytes(five_or_more[:8].ljust(8, b"\0"), "little")
    return ((((s << 24) & _M64) * 889523592379) & _M64) >> 52


def compress_u32(src: bytes, trace=None, stats=None):
    """-> (payload, refused).  trace (a list) receives (ip, match, literals, match length) of every sequence; stats (a dict)
    receives "refused_equal": the refused candidates whose four bytes DO match the probe's (only the distance test stands
    between them and a sequence with an offset the format cannot hold)."""
    n = len(src)
    out = bytearray()
    pad = src + b"\0" * 8
    table = [0] * 4096
    anchor = 0
    refused = refused_equal = 0

    def h5(p):
        return hash5(pad[p:p + 8])

    def emit(lit_start, lit_len, offset, mcode):
        tok_l = min(lit_len, 15)
        out.append((tok_l << 4) | (0 if offset is None else min(mcode, 15)))
        if lit_len >= 15:
            out.extend(_len_bytes(lit_len - 15))
        out.extend(src[lit_start:lit_start + lit_len])
        if offset is not None:
            out.append(offset & 255)
            out.append(offset >> 8)
            if mcode >= 15:
                out.extend(_len_bytes(mcode - 15))

    if n >= 13:
        mfl1 = n - 12 + 1
        matchlimit = n - 5
        table[h5(0)] = 0
        ip = 1
        fh = h5(ip)
        done = False
        while not done:
            fip, step, nb = ip, 1, 64
            while True:
                h, cur, mi = fh, fip, table[fh]
                ip = fip
                fip += step
                step = nb >> 6
                nb += 1
                if fip > mfl1:
                    done = True
                    break
                fh = h5(fip)
                table[h] = cur
                if mi + 65535 < cur:
                    refused += 1
                    refused_equal += src[mi:mi + 4] == src[ip:ip + 4]
                    continue
                if src[mi:mi + 4] == src[ip:ip + 4]:
                    break
            if done:
                break
            match = mi
            while ip > anchor and match > 0 and src[ip - 1] == src[match - 1]:
                ip -= 1
                match -= 1
            lit_start, lit_len = anchor, ip - anchor
            while True:
                offset = ip - match
                a, b = ip + 4, match + 4
                while a < matchlimit and src[a] == src[b]:
                    a += 1
                    b += 1
                mcode = a - (ip + 4)
                if trace is not None:
                    trace.append((ip, match, lit_len, mcode + 4))
                ip = a
                emit(lit_start, lit_len, offset, mcode)
                anchor = ip
                if ip >= mfl1:
                    done = True
                    break
                table[h5(ip - 2)] = ip - 2
                h = h5(ip)
                mi = table[h]
                table[h] = ip
                if mi + 65535 >= ip and src[mi:mi + 4] == src[ip:ip + 4]:
                    match = mi
                    lit_start, lit_len = ip, 0
                    continue
                if mi + 65535 < ip:
                    refused += 1
                    refused_equal += src[mi:mi + 4] == src[ip:ip + 4]
                ip += 1
                fh = h5(ip)
                break
    emit(anchor, n - anchor, None, 0)
    if stats is not None:
        stats["refused_equal"] = refused_equal
    return bytes(out), refused


def _len_bytes(r):
    out = bytearray()
    while r >= 255:
        out.append(255)
        r -= 255
    out.append(r)
    return out


def block_offsets(payload: bytes):
    """the offsets of the matches of an LZ4 block, in order"""
    ip, n, offs = 0, len(payload), []
    while ip < n:
        t = payload[ip]
        ip += 1
        lit = t >> 4
        if lit == 15:
            while True:
                b = payload[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        if ip >= n:
            break
        offs.append(payload[ip] | (payload[ip + 1] << 8))
        ip += 2
        if t & 15 == 15:
            while True:
                b = payload[ip]
                ip += 1
                if b != 255:
                    break
    return offs


# ---- liblz4-built expectations --------------------------------------------------------------------------------------------
def liblz4_block(d: np.ndarray) -> bytes:
    return framing.lz4_fast(np.ascontiguousarray(d))


def level(block_size: int) -> int:
    """LZ4BlockOutputStream.compressionLevel: ceil(log2(blockSize)) - 10, at least 0"""
    return max(0, (int(block_size) - 1).bit_length() - 10)


def frame(chunk: np.ndarray, block_size: int) -> bytes:
    """one LZ4Block frame as LZ4BlockOutputStream(blockSize) writes it, payload from liblz4"""
    chunk = np.ascontiguousarray(chunk)
    payload = liblz4_block(chunk)
    raw = len(payload) >= chunk.size
    body = chunk.tobytes() if raw else payload
    return b"LZ4Block" + bytes([(0x10 if raw else 0x20) | level(block_size)]) + struct.pack(
        "<iiI", len(body), chunk.size, framing.xxh32(chunk.tobytes()) & 0x0FFFFFFF) + body


def jvm_stream(data: np.ndarray, block_size: int) -> bytes:
    """what LZ4BlockOutputStream(blockSize) writes for one partition (nothing for an empty one)"""
    out = bytearray()
    for p in range(0, data.size, block_size):
        out += frame(data[p:p + block_size], block_size)
    if data.size:
        out += b"LZ4Block" + bytes([0x10 | level(block_size)]) + struct.pack("<iii", 0, 0, 0)
    return bytes(out)


def frame_tokens(stream: bytes):
    """(token, compressed length, original length) of every frame of a partition's stream"""
    out, p = [], 0
    while p < len(stream):
        assert stream[p:p + 8] == b"LZ4Block"
        clen, olen = struct.unpack_from("<ii", stream, p + 9)
        out.append((stream[p + 8], clen, olen))
        p += 21 + clen
    return out


def crc32c(b: bytes) -> int:
    """CRC32C (Castagnoli, reflected 0x82F63B78) as java.util.zip.CRC32C: slicing-by-8 over the 64-bit words, so that whole
    .data images (tens of MB) take seconds in Python"""
    t = _crc32c_tables()
    t0, t1, t2, t3, t4, t5, t6, t7 = t
    c = 0xFFFFFFFF
    n8 = len(b) & ~7
    for w in np.frombuffer(b, dtype="<u8", count=n8 // 8).tolist():
        c ^= w & 0xFFFFFFFF
        c = (t7[c & 255] ^ t6[(c >> 8) & 255] ^ t5[(c >> 16) & 255] ^ t4[c >> 24]
             ^ t3[(w >> 32) & 255] ^ t2[(w >> 40) & 255] ^ t1[(w >> 48) & 255] ^ t0[w >> 56])
    for x in b[n8:]:
        c = t0[(c ^ x) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


_TAB = []


def _crc32c_tables():
    if not _TAB:
        t0 = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
            t0.append(c)
        _TAB.append(t0)
        for k in range(1, 8):
            prev = _TAB[k - 1]
            _TAB.append([t0[v & 255] ^ (v >> 8) for v in prev])
    return _TAB


def checksum(algo: int, b: bytes) -> int:
    """algo as S3S_CHECKSUM_*: 1 Adler32, 2 CRC32, 3 CRC32C"""
    return zlib.adler32(b) if algo == 1 else zlib.crc32(b) if algo == 2 else crc32c(b)


def expected_map_output(parts, block_size: int, algo: int):
    """-> (image bytes, index list [n + 1], checksums list [n]) of partitions given as uint8 arrays"""
    streams = [jvm_stream(np.asarray(p, np.uint8), block_size) for p in parts]
    index = [0]
    for s in streams:
        index.append(index[-1] + len(s))
    return b"".join(streams), index, [checksum(algo, s) if algo else 0 for s in streams]


# ---- inputs that exercise the distance test ---------------------------------------------------------------------------------
def far_motif(rng) -> np.ndarray:
    """146 500 bytes: a 3 000-byte random motif, 70 000 bytes of filler, the motif, 67 000 bytes of filler, the motif, 500 bytes
    of filler.  The second and third copy find the table entries of the copy before them: more than 65 535 bytes back, with
    bytes that DO match - the parse must still refuse them."""
    motif = rng.integers(0, 256, 3000, dtype=np.uint8)

    def fill(k):
        return rng.integers(0, 4, k, dtype=np.uint8)

    return np.ascontiguousarray(np.concatenate([motif, fill(70000), motif, fill(67000), motif, fill(500)]))


def boundary_input(d: int, rng) -> np.ndarray:
    """a 64-byte motif of bytes 4..255, filler of bytes 0..3 (low entropy keeps the skip step at 1, so the second copy is
    probed), the motif again d bytes after its first copy, 3 000 more filler bytes"""
    motif = rng.integers(4, 256, 64, dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([motif, rng.integers(0, 4, d - 64, dtype=np.uint8), motif,
                                                rng.integers(0, 4, 3000, dtype=np.uint8)]))


def long_literals(rng) -> np.ndarray:
    """239 000 bytes: literal runs of 100 000 and 70 000 bytes (their length bytes alone are 392 and 275) in front of matches
    that run 60 000 and 9 000 bytes: sequences whose literal run is longer than a whole byU16 chunk"""
    return np.ascontiguousarray(np.concatenate([rng.integers(0, 256, 100_000, dtype=np.uint8), np.zeros(60_000, np.uint8),
                                                rng.integers(0, 256, 70_000, dtype=np.uint8), np.zeros(9_000, np.uint8)]))


def boundary_pair():
    """the two hand-built inputs at the exact boundary: distance 65 535 (a match of offset 65 535) and 65 536 (refused)"""
    return boundary_input(65535, np.random.default_rng(91)), boundary_input(65536, np.random.default_rng(92))
