"""Damaged ranges for the streaming reduce side (s3s_dstream_*), and what the stream's contract says about each of them.
Test infrastructure for tests/test_isa_decode_stream_damage.py (the compiled kernels on the CPU) and
tests/test_gpu_decode_stream_damage.py (the same cases on the hardware).  Deterministic: fixed seeds, a fixed case list.

  images()     the base images: the cut-position images of tests/test_isa_decode_stream.py, a Snappy multi-spill partition, an
               image with an empty partition on both sides of the damaged one, an LZ4 image with an inner stream in a payload
  cases()      every field-targeted mutation of a first, a middle and a last unit of a partition (the three base images) or of
               the middle unit (the other images); each records the unit and the byte span it touches
  Model        a plain sequential walk with the header rules of LZ4BlockInputStream.refill(), SnappyInputStream and
               LZFInputStream as csrc/discover_core.h and csrc/decode_stream_kernels.hip state them; the payload of every whole
               unit is decoded by the oracle.  classify() names the first thing a sequential reader objects to; feed() is what
               one feed answers (decode_stream.hip restated); run() is a caller that follows need_comp and need_dst.

The fifth byte of a Snappy varint: the product and the oracle both keep its low four bits and drop the rest, so "a 5-byte
varint with bits above 2^32" is the claim its low 32 bits spell."""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

import corpus
import stream_units as su

LZ4, SNAPPY, LZF = su.LZ4, su.SNAPPY, su.LZF
ADLER, CRC = 1, 2
OK, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_UNSUPPORTED = 0, -2, -3, -4, -6
K_MAX = 1 << 25  # kBatchMaxBlock (csrc/s3s_internal.h): the largest decoded unit a decoder takes
HEADER_INVALID, TRUNCATED, PAYLOAD_INVALID, OVERSIZED, VALID_DIFFERENT = (
    "header-invalid", "truncated", "payload-invalid", "oversized-claim", "valid-different")
CLASSES = (HEADER_INVALID, TRUNCATED, PAYLOAD_INVALID, OVERSIZED, VALID_DIFFERENT)
CODEC_NAME = {LZ4: "lz4", SNAPPY: "snappy", LZF: "lzf"}
MAGIC = b"LZ4Block"


def _concat(parts):
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return np.concatenate(parts).astype(np.uint8), offs


# ---- base images -------------------------------------------------------------------------------------------------------------
@dataclass
class Image:
    name: str
    codec: int
    img: bytes
    index: List[int]
    part: int          # the partition that gets damaged
    block: int         # decoded bytes of the largest unit the writer made
    full: bool         # True: first, middle and last unit are damaged; False: the middle one
    crc: bool = False  # the image whose checksum schedule is CRC32 (Adler32 elsewhere)


def images(oracle) -> List[Image]:
    out = []

    def add(name, codec, img, index, part, full, crc=False):
        b = img.tobytes() if hasattr(img, "tobytes") else bytes(img)
        idx = [int(x) for x in index]
        out.append(Image(name, codec, b, idx, part, max(u[2] for u in su.units(codec, b, idx)), full, crc))

    rng = np.random.default_rng(5)
    data, offs = _concat([corpus.chunk_corpus(3, 3 * 4096 - 100, rng), corpus.chunk_corpus(7, 2 * 4096 + 9, rng)])
    img, index, _ = oracle.compress_map_output(LZ4, 1, data, offs, 4096)
    add("lz4", LZ4, img, index, 0, True)
    rng = np.random.default_rng(6)
    data, offs = _concat([corpus.chunk_corpus(3, 2 * 4096 + 5, rng), corpus.chunk_corpus(7, 4096 + 900, rng)])
    img, index, _ = oracle.compress_map_output(SNAPPY, 2, data, offs, 4096)
    add("snappy", SNAPPY, img, index, 0, True, crc=True)
    _, _, img, index, _ = su.lzf_cut_image(oracle, 3)
    add("lzf", LZF, img, index, 1, True)
    # a Snappy partition of two concatenated streams (two spills), a partition of one stream behind it
    rng = np.random.default_rng(8)
    segs = [corpus.chunk_corpus(7, 2 * 4096 + 77, rng), corpus.chunk_corpus(3, 4096 + 300, rng), corpus.chunk_corpus(7, 1500, rng)]
    streams = [oracle.compress_stream(SNAPPY, s, 4096) for s in segs]
    add("snappy-spills", SNAPPY, np.concatenate(streams), [0, streams[0].size + streams[1].size, sum(s.size for s in streams)], 0, False)
    # an empty partition in front of and behind the damaged one
    for codec, name in ((LZ4, "lz4-empties"), (SNAPPY, "snappy-empties"), (LZF, "lzf-empties")):
        rng = np.random.default_rng(9)
        data, offs = _concat([corpus.chunk_corpus(3, 700, rng), np.zeros(0, np.uint8), corpus.chunk_corpus(7, 2 * 4096 + 31, rng),
                              np.zeros(0, np.uint8), corpus.chunk_corpus(3, 900, rng)])
        img, index, _ = oracle.compress_map_output(codec, 1, data, offs, 4096)
        add(name, codec, img, index, 2, False)
    # an inner LZ4 stream planted in a payload (test_lz4_windows_of_several_tiles), cut to two tiles
    rng = np.random.default_rng(21)
    inner = oracle.compress_stream(LZ4, rng.integers(0, 256, 3000, dtype=np.uint8), 1024)
    data, offs = _concat([corpus.chunk_corpus(0, 70_000, rng), np.resize(inner, 36_000), corpus.chunk_corpus(7, 9_000, rng)])
    img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs)
    add("lz4-planted", LZ4, img, index, 1, False)
    assert 65536 < len(out[-1].img) < 2 * 65536
    return out


# ---- the header rules ----------------------------------------------------------------------------------------------------------
def probe(codec: int, b: bytes, ip: int, end: int, pend: int, header_next: bool, bound: bool = True):
    """The unit at b[ip] when b[:end] is visible and its partition (LZ4: the range) ends at pend >= end ->
    ("ok", length, claim, head) | ("skip", length) a Snappy stream header | ("cut", need) the window ends inside it |
    ("trunc",) the partition ends inside it | ("bad",) a header rule refuses it | ("big", claim) it claims more than K_MAX
    decoded bytes (bound=False: without that rule, for sizing what such a range claims).  su.unit_at, answering instead of asserting."""
    state = {}

    def want(x):
        if x > pend - ip:
            state["r"] = ("trunc",)
        elif x > end - ip:
            state["r"] = ("cut", x)
        else:
            return True
        return False

    if codec == LZ4:
        unit, ol = 21, 0
        if end - ip >= 21:
            if b[ip:ip + 8] != MAGIC:
                return ("bad",)
            token = b[ip + 8]
            method, level = token & 0xF0, 10 + (token & 0x0F)
            cl, ol = struct.unpack_from("<ii", b, ip + 9)
            check = struct.unpack_from("<I", b, ip + 17)[0]
            if (method not in (0x10, 0x20) or ol < 0 or cl < 0 or ol > (1 << level) or (ol == 0) != (cl == 0) or
                    (method == 0x10 and ol != cl) or (ol == 0 and check != 0)):
                return ("bad",)
            unit += cl
        if not want(unit):
            return state["r"]
        return ("ok", unit, ol, 21)
    if codec == SNAPPY:
        if header_next:
            if not want(16):
                return state["r"]
            return ("skip", 16) if b[ip:ip + 8] == su.SNAPPY_MAGIC else ("bad",)
        if not want(4):
            return state["r"]
        cl = struct.unpack_from(">I", b, ip)[0]
        if cl == 0x82534E41:
            return ("skip", 0)  # the next concatenated stream starts here
        if cl == 0:
            return ("bad",)
        if not want(4 + cl):
            return state["r"]
        ulen, sh, i = 0, 0, 0
        while True:
            if i >= cl or sh > 28:
                return ("bad",)
            c = b[ip + 4 + i]
            ulen |= ((c & 0x7F) << sh) & 0xFFFFFFFF
            if not c & 0x80:
                break
            i, sh = i + 1, sh + 7
        if bound and ulen > K_MAX:
            return ("big", ulen)
        return ("ok", 4 + cl, ulen, 4)
    if codec == LZF:
        if not want(5):
            return state["r"]
        if b[ip:ip + 2] != b"ZV" or b[ip + 2] > 1:
            return ("bad",)
        typ, ln = b[ip + 2], struct.unpack_from(">H", b, ip + 3)[0]
        head, ulen = 5, ln
        if typ == 1:
            if not want(7):
                return state["r"]
            head, ulen = 7, struct.unpack_from(">H", b, ip + 5)[0]
            if ln == 0 or ulen == 0:
                return ("bad",)
        if not want(head + ln):
            return state["r"]
        return ("ok", head + ln, ulen, head)
    raise ValueError(codec)


@dataclass
class Case:
    name: str
    image: Image
    img: bytes
    index: List[int]
    unit: Tuple[int, int, int]  # (start, length, decoded) of the damaged unit in the base image
    span: Tuple[int, int]       # the bytes the mutation touches, [lo, hi) in the range
    cls: str = ""
    claim: int = 0              # the decoded size the damaged unit claims after the mutation (0: unknown / no unit)

    @property
    def codec(self):
        return self.image.codec


# ---- the model -----------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, oracle, bound: bool = True):
        self.oracle, self.bound = oracle, bound
        self._payload: Dict[tuple, Optional[bytes]] = {}
        self.calls: List[Tuple[int, bytes, int]] = []  # every decode asked of the oracle: (codec, bytes, capacity)
        self._sums: Dict[tuple, int] = {}

    # the payload of one whole unit through the oracle's decoder -> decoded bytes, or None when it refuses
    def payload(self, codec: int, b: bytes, start: int, length: int, claim: int, head: int) -> Optional[bytes]:
        unit = b[start:start + length]
        key = (codec, unit, claim)
        if key in self._payload:
            return self._payload[key]
        if claim > K_MAX:
            r = None
        elif codec == LZF and head == 5:
            r = unit[5:]
        elif codec == LZF:
            self.calls.append((LZF, unit[7:], claim))
            d = self.oracle.lzf_decompress_block(np.frombuffer(unit[7:], np.uint8), claim)
            r = d.tobytes() if not isinstance(d, int) and d.size == claim else None
        else:
            stream = unit if codec == LZ4 else su.SNAPPY_MAGIC + bytes(8) + unit
            self.calls.append((codec, stream, claim))
            try:
                d = self.oracle.decompress_stream(codec, np.frombuffer(stream, np.uint8), claim)
                r = d.tobytes() if d.size == claim else None
            except RuntimeError:
                r = None
        self._payload[key] = r
        return r

    def walk(self, codec: int, b: bytes, index: List[int], pos: int, end: int):
        """The units from pos while b[:end] is visible -> (units [(start, length, claim, head)], stop, need, verdict):
        verdict None | "trunc" | "bad" | "big" for the unit at stop.  LZ4: one chain over the range; Snappy / LZF: partition
        by partition, a Snappy stream header in front of every partition that starts at or behind pos."""
        total, out = index[-1], []
        if codec == LZ4:
            spans = [(pos, total, False)]
        else:
            spans = [(max(index[p], pos), index[p + 1], codec == SNAPPY and index[p] >= pos)
                     for p in range(len(index) - 1) if index[p + 1] > pos and index[p] < end]
        for beg, pend, header_next in spans:
            ip = beg
            while ip < min(pend, end):
                r = probe(codec, b, ip, min(pend, end), pend, header_next, self.bound)
                if r[0] == "skip":
                    header_next, ip = r[1] == 0, ip + r[1]
                elif r[0] == "ok":
                    out.append((ip, r[1], r[2], r[3]))
                    ip += r[1]
                elif r[0] == "cut":
                    return out, ip, r[1], None
                elif r[0] == "big" and any(self._corrupt(codec, b, index, q, end) for q in range(len(index) - 1) if index[q] >= pend):
                    return out, ip, 0, "bad"  # the pieces are walked side by side: corruption in a later one beats the refusal
                else:
                    return out, ip, 0, r[0]
            assert ip == min(pend, end)
        return out, min(end, total), 0, None

    def _corrupt(self, codec: int, b: bytes, index: List[int], q: int, end: int) -> bool:
        """partition q, as far as b[:end] shows it, ends in corruption"""
        if index[q] >= end or index[q + 1] == index[q]:
            return False
        return self._walk_one(codec, b, index[q], min(index[q + 1], end), index[q + 1]) in ("bad", "trunc")

    def _walk_one(self, codec: int, b: bytes, beg: int, end: int, pend: int):
        ip, header_next = beg, codec == SNAPPY
        while ip < end:
            r = probe(codec, b, ip, end, pend, header_next, self.bound)
            if r[0] == "skip":
                header_next, ip = r[1] == 0, ip + r[1]
            elif r[0] == "ok":
                ip += r[1]
            else:
                return r[0]
        return None

    def classify(self, c: Case) -> str:
        """What a reader that takes the range unit by unit objects to first."""
        b, index, codec = c.img, c.index, c.codec
        units, stop, _, verdict = self.walk(codec, b, index, 0, index[-1])
        c.claim = 0
        for start, length, claim, head in units:
            if start <= c.span[0] < start + length or start == c.unit[0]:
                c.claim = claim
            if claim >= K_MAX:  # a valid header that sends the caller for the largest buffer a decoder takes
                c.claim = claim
                return OVERSIZED
            if self.payload(codec, b, start, length, claim, head) is None:
                return PAYLOAD_INVALID
        if verdict == "big":
            c.claim = probe(codec, b, stop, index[-1], index[-1], False, False)[2]
            return OVERSIZED
        if verdict is not None:
            return TRUNCATED if verdict == "trunc" else HEADER_INVALID
        assert b != c.image.img or index != c.image.index, c.name
        return VALID_DIFFERENT

    # ---- one feed (csrc/decode_stream.hip) -----------------------------------------------------------------------------------
    def pieces(self, index: List[int], cur: int, pos: int, length: int):
        """-> (n pieces, window-relative piece offsets, the first piece starts inside a stream, where the last piece's partition ends)"""
        n, np_, wend = 0, len(index) - 1, pos + length
        while cur + n < np_ and (index[cur + n] < wend or index[cur + n + 1] <= wend):
            n += 1
        off = [0] * (n + 1)
        for i in range(n):
            off[i] = max(index[cur + i] - pos, 0)
            off[i + 1] = min(index[cur + i + 1] - pos, length)
        return n, off, pos > index[cur] if cur < np_ else False, (index[cur + n] - pos if n else 0)

    def discover(self, codec: int, b: bytes, index: List[int], cur: int, pos: int, length: int, cap: int) -> dict:
        """What the discovery kernels and the capacity cut answer for the window [pos, pos + length): the words that
        tests/isa/stream_kernel.py returns.  Offsets are window-relative."""
        units, stop, need, verdict = self.walk(codec, b, index, pos, pos + length)
        out = dict(status=0, stop=stop - pos, need=need, n_frames=len(units), k=0, consumed=stop - pos, out_len=0, need_dst=0, units=units)
        if verdict is not None:
            out["status"] = E_UNSUPPORTED if verdict == "big" else E_BAD_FRAME
            return out
        if not units:
            return out
        fo = [0]
        for u in units:
            fo.append(fo[-1] + u[2])
        k = next((i for i in range(len(units)) if fo[i + 1] > cap), len(units))
        out["k"], out["out_len"] = k, fo[k]
        if k < len(units):
            out["consumed"], out["need_dst"] = units[k][0] - pos, units[k][2]
        return out

    def checksum(self, algo: int, data: bytes) -> int:
        key = (algo, data)
        if key not in self._sums:
            self._sums[key] = (zlib.adler32(data) if algo == ADLER else zlib.crc32(data)) & 0xFFFFFFFF
        return self._sums[key]

    def front_bytes(self, c: Case) -> bytes:
        """the decoded bytes of the partitions in front of the damaged one"""
        img, index = c.image.img, c.image.index
        units = self.walk(c.codec, img, index, 0, index[c.image.part])[0]
        return b"".join(self.payload(c.codec, img, u[0], u[1], u[2], u[3]) for u in units)

    def ref_sums(self, image: Image, algo: int):
        return [self.checksum(algo, image.img[image.index[p]:image.index[p + 1]]) for p in range(len(image.index) - 1)]

    def feed(self, c: Case, algo: int, st: dict, length: int, cap: int) -> dict:
        """One feed of the stream in state st = {pos, cur, err, bad}: -> the s3s_dstream_result words, `code`, the decoded
        bytes, and `kernel` = discover()'s answer (None when the feed launches no discovery).  Advances st."""
        b, index, codec = c.img, c.index, c.codec
        np_, total = len(index) - 1, index[-1]
        r = dict(code=OK, consumed=0, out_len=0, need_comp=0, need_dst=0, at_end=0, bad=-1, data=b"", kernel=None, decoded=False)
        if st["err"]:
            r["code"], r["bad"] = st["err"], st["bad"]
            return r
        pos, cur, wend = st["pos"], st["cur"], st["pos"] + length
        ref = self.ref_sums(c.image, algo) if algo else None

        def wrong(q, upto):
            return algo and upto >= index[q + 1] and self.checksum(algo, b[index[q]:index[q + 1]]) != ref[q]

        def stick(code, bad):
            st["err"], st["bad"] = code, bad
            r["code"], r["bad"] = code, bad
            return r

        if length == 0:
            q = cur
            while q < np_ and index[q + 1] <= pos:
                if wrong(q, pos):
                    return stick(E_CHECKSUM, q)
                q += 1
            st["cur"] = q
            r["at_end"] = int(pos == total and q == np_)
            if total - pos > 0:
                r["need_comp"] = {LZ4: 21, LZF: 5}.get(codec, 16 if pos == index[min(q, np_)] else 4)
            return r
        n = self.pieces(index, cur, pos, length)[0]
        k = r["kernel"] = self.discover(codec, b, index, cur, pos, length, cap)
        if k["status"] != 0:
            for i in range(n):  # the partitions whose last byte the window holds: a wrong checksum comes first
                if wrong(cur + i, wend):
                    return stick(E_CHECKSUM, cur + i)
            if k["status"] == E_UNSUPPORTED:  # refused, not corrupt: nothing is consumed and the answer repeats
                r["code"] = E_UNSUPPORTED
                return r
            return stick(E_BAD_FRAME, -1)
        if k["n_frames"] > 0 and k["consumed"] == 0:
            r["code"], r["need_dst"] = E_CAPACITY, k["need_dst"]
            return r
        new_pos = pos + k["consumed"]
        q = cur
        while q < np_ and index[q + 1] <= new_pos:
            if wrong(q, new_pos):
                return stick(E_CHECKSUM, q)
            q += 1
        parts = []
        r["decoded"] = k["k"] > 0
        for start, length_, claim, head in k["units"][:k["k"]]:
            d = self.payload(codec, b, start, length_, claim, head)
            if d is None:  # as in discovery: a wrong checksum of a partition whose last byte the window holds comes first
                for i in range(n):
                    if wrong(cur + i, wend):
                        return stick(E_CHECKSUM, cur + i)
                return stick(E_BAD_FRAME, -1)
            parts.append(d)
        st["pos"], st["cur"] = new_pos, q
        r["consumed"], r["out_len"], r["data"] = k["consumed"], k["out_len"], b"".join(parts)
        r["need_comp"] = k["need"] if k["consumed"] == 0 else 0
        r["at_end"] = int(new_pos == total and q == np_)
        return r

    # ---- a caller that follows the contract ----------------------------------------------------------------------------------
    def run(self, c: Case, sched: "Schedule", algo: int, feed=None, max_feeds: int = 10_000):
        """Feeds the range as a caller does: the first window ends at sched.first_end, the later ones are the rest of the range
        (sched.unit_at_a_time: every window starts at one byte); a window grows to need_comp and dst to need_dst.
        feed(st, pos, window length, capacity) -> the result of one feed (default: the model's own).  -> the list of
        (pos, cur, window length, capacity, result) and the decoded bytes handed out."""
        st = dict(pos=0, cur=0, err=0, bad=-1)
        feed = feed or (lambda st_, pos_, w_, cap_: self.feed(c, algo, st_, w_, cap_))
        total, cap = c.index[-1], sched.capacity(c)
        trace, out, win = [], [], (1 if sched.unit_at_a_time else sched.first_end)
        while True:
            pos, cur = st["pos"], st["cur"]
            w = max(0, min(win, total - pos))
            r = feed(st, pos, w, cap)
            trace.append((pos, cur, w, cap, r))
            assert len(trace) <= max_feeds, ("the stream makes no progress", c.name, sched)
            if r["code"] == E_CAPACITY:
                assert r["need_dst"] > cap, ("asked for no more than it had", c.name, r["need_dst"], cap)
                cap = r["need_dst"]
                if cap > K_MAX:  # (a caller would go on to allocate this: the tests stop here and assert on it)
                    break
                continue
            if r["code"] != OK or r["at_end"]:
                break
            out.append(r["data"])
            if r["consumed"] == 0:
                assert r["need_comp"] > w, ("asked for no more than it had", c.name, pos, w, r["need_comp"])
                win = r["need_comp"]
            else:
                win = 1 if sched.unit_at_a_time else total
        if r["code"] == OK:
            out.append(r["data"])
        return trace, b"".join(out)


@dataclass(frozen=True)
class Schedule:
    where: str            # before | in-header | behind-field | behind-unit | whole | unit-at-a-time
    first_end: int
    cap_mode: str         # ample | front | claim-1
    unit_at_a_time: bool = False

    def capacity(self, c: Case) -> int:
        if self.cap_mode == "front":  # exactly the decoded bytes in front of the damaged unit
            return sum(u[2] for u in su.units(c.codec, c.image.img, c.image.index) if u[0] < c.unit[0])
        if self.cap_mode == "claim-1":  # the damaged unit's claimed size - 1 (no buffer above the decoder's largest block)
            return max(0, min(c.claim, K_MAX) - 1)
        return 1 << 18


WHERE = ("before", "in-header", "behind-field", "behind-unit", "whole", "unit-at-a-time")
CAP_MODES = ("ample", "front", "claim-1")


def schedules(c: Case, cap_modes=CAP_MODES) -> List[Schedule]:
    """The window ends of one case x the capacities.  A window end that the case does not have (the damaged field is the
    unit's first byte, or the range ends in front of it) falls on its neighbour, so every case has all six."""
    total, (start, length, _), (lo, hi) = c.index[-1], c.unit, c.span
    ends = {"before": start, "in-header": max(lo, start + 1), "behind-field": min(hi, start + length - 1),
            "behind-unit": start + length + 1, "whole": total, "unit-at-a-time": total}
    out = []
    for w in WHERE:
        e = max(1, min(ends[w], total))
        out += [Schedule(w, e, m, w == "unit-at-a-time") for m in cap_modes]
    return out


# ---- the mutations ---------------------------------------------------------------------------------------------------------------
def _set(b: bytes, at: int, new: bytes) -> bytes:
    return b[:at] + new + b[at + len(new):]


def _i32(v):
    return struct.pack("<I", v & 0xFFFFFFFF)


def _varint(v, nbytes=None):
    out = bytearray()
    while True:
        out.append(v & 0x7F | (0x80 if v > 0x7F or (nbytes and len(out) + 1 < nbytes) else 0))
        v >>= 7
        if not v and not (nbytes and len(out) < nbytes):
            return bytes(out)


def _varint_len(b, at):
    n = 1
    while b[at + n - 1] & 0x80:
        n += 1
    return n


def _mutations(image: Image, u, rng) -> List[Tuple[str, int, bytes, Optional[List[int]]]]:
    """-> [(name, offset in the range, the bytes written there, a new index or None)] for the unit u of the image"""
    b, codec, (s, ln, dec) = image.img, image.codec, u
    total, pend = image.index[-1], next(e for e in image.index[1:] if e > s)
    m = []

    def put(name, at, new, index=None):
        m.append((name, at, bytes(new), index))

    def cut_range(name, at):  # the range ends early: the last index entry shortened to `at`, with every entry behind it
        put(name, at, b"", [min(x, at) for x in image.index])

    if codec == LZ4:
        token, (cl, ol) = b[s + 8], struct.unpack_from("<ii", b, s + 9)
        level = 10 + (token & 15)
        for i in range(8):
            put(f"magic[{i}]", s + i, [b[s + i] ^ 0x20])
        put("method=0x00", s + 8, [token & 15])
        put("method=0x30", s + 8, [0x30 | token & 15])
        put("method-swapped", s + 8, [(0x30 - (token & 0xF0)) | token & 15])
        low = max(0, (ol - 1).bit_length() - 11)  # the largest level nibble with (1 << level) < orig_len
        put("level-lowered", s + 8, [token & 0xF0 | low])
        put("level-raised", s + 8, [token & 0xF0 | 15])  # still a valid stream: only a checksum can object
        put("level=15,orig=1<<25", s + 8, bytes([token & 0xF0 | 15]) + _i32(cl) + _i32(1 << 25))
        for name, v in (("-1", cl - 1), ("=0", 0), ("+1", cl + 1), ("=0x7fffffff", 0x7FFFFFFF), ("negative", -cl), ("=left+1", total - s - 21 + 1)):
            put("comp_len" + name, s + 9, _i32(v))
        for name, v in (("-1", ol - 1), ("=0", 0), ("+1", ol + 1), ("negative", -ol), ("=(1<<level)+1", (1 << level) + 1)):
            put("orig_len" + name, s + 13, _i32(v))
        put("stored,orig!=comp", s + 8, bytes([0x10 | token & 15]) + _i32(cl) + _i32(cl + 1))
        put("check-flipped", s + 17, [b[s + 17] ^ 1])
        end_frame = next((x[0] for x in su.units(LZ4, b, image.index) if x[0] >= s and x[2] == 0), None)
        if end_frame is not None:
            put("end-frame-check!=0", end_frame + 17, [1])
        inner = b.find(MAGIC, s + 21, s + ln)
        if inner >= 0:
            put("comp_len->planted-frame", s + 9, _i32(inner - s - 21))
        fields = (("magic", 3), ("token", 8), ("comp_len", 10), ("orig_len", 15), ("check", 19), ("payload", 21 + cl // 2))
    elif codec == SNAPPY:
        cl = struct.unpack_from(">I", b, s)[0]
        vl = _varint_len(b, s + 4)
        hs = max(e for e in image.index if e <= s)  # the stream header of the unit's partition
        for i in range(16):
            put(f"stream-header[{i}]", hs + i, [b[hs + i] ^ 0x40])
        for name, v in (("=0", 0), ("-1", cl - 1), ("+1", cl + 1), ("=0x7fffffff", 0x7FFFFFFF), ("=left+1", pend - s - 4 + 1), ("=magic", 0x82534E41)):
            put("chunk_len" + name, s, struct.pack(">I", v))
        for name, v in (("-1", dec - 1), ("+1", dec + 1), ("=1<<25", 1 << 25), ("=(1<<25)+1", (1 << 25) + 1), ("=2^31-1", (1 << 31) - 1),
                        ("=2^31", 1 << 31), ("=2^32-1", (1 << 32) - 1)):
            # (written over the varint and the payload's first bytes, with the varint's own length: the chunk keeps its length)
            put("claim" + name, s + 4, _varint(v))
        put("claim-5-bytes,bits-above-2^32", s + 4, _varint(dec, 5)[:4] + b"\x70")  # the low 32 bits spell the true size
        put("claim-5-bytes,bit-28-and-above", s + 4, _varint(dec, 5)[:4] + b"\x71")
        put("claim-sixth-byte", s + 4, b"\x80" * 5 + b"\x01")
        put("claim-continues-to-the-last-byte", s + 4, bytes(x | 0x80 for x in b[s + 4:s + 4 + cl]))
        fields = (("chunk_len", 2), ("claim", 4), ("payload", 4 + cl // 2))
    else:
        typ, l16 = b[s + 2], struct.unpack_from(">H", b, s + 3)[0]
        put("Z-damaged", s, [b[s] ^ 0x20])
        put("V-damaged", s + 1, [b[s + 1] ^ 0x20])
        put("type=2", s + 2, [2])
        put("type=255", s + 2, [255])
        for name, v in (("=0", 0), ("-1", l16 - 1), ("+1", l16 + 1), ("=65535", 65535)):
            put("len" + name, s + 3, struct.pack(">H", v & 0xFFFF))
        if typ == 1:
            for name, v in (("=0", 0), ("-1", dec - 1), ("+1", dec + 1), ("=65535", 65535)):
                put("ulen" + name, s + 5, struct.pack(">H", v & 0xFFFF))
        put("stored<->compressed", s + 2, [1 - typ])
        fields = (("ZV", 1), ("type", 2), ("len", 4)) + ((("ulen", 6),) if typ == 1 else ()) + (("payload", (7 if typ == 1 else 5) + l16 // 2),)
    for name, d in fields:
        cut_range(f"range-ends-in-{name}", s + d)
    head = 21 if codec == LZ4 else 4 + _varint_len(b, s + 4) if codec == SNAPPY else (7 if b[s + 2] == 1 else 5)
    if ln > head + 4:
        for n in (2, 3, 4):
            at = sorted(int(x) for x in rng.choice(np.arange(s + head, s + ln), n, replace=False))
            new = bytearray(b[at[0]:at[-1] + 1])
            for a in at:
                new[a - at[0]] = (new[a - at[0]] + 1 + int(rng.integers(0, 255))) & 0xFF
            put(f"payload-{n}-bytes", at[0], new)
    return m


_CASES: Dict[int, List[Case]] = {}


def cases(oracle, model: Optional[Model] = None) -> List[Case]:
    """The fixed case list, classified."""
    if id(oracle) in _CASES and model is None:
        return _CASES[id(oracle)]
    model = model or Model(oracle)
    out = []
    for image in images(oracle):
        p = image.part
        all_units = su.units(image.codec, image.img, image.index)
        data_units = [u for u in all_units
                      if image.index[p] <= u[0] < image.index[p + 1] and u[2] > 0]
        picks = [("first", data_units[0]), ("middle", data_units[len(data_units) // 2]), ("last", data_units[-1])]
        if image.codec == LZ4 and image.name == "lz4-planted":  # the unit that holds the inner stream
            picks = [x for x in picks if image.img.find(MAGIC, x[1][0] + 21, x[1][0] + x[1][1]) >= 0][:1] or picks
        rng = np.random.default_rng(77)
        for which, u in picks if image.full else picks[1:2] if len(picks) > 1 else picks:
            seen = set()
            for name, at, new, index in _mutations(image, u, rng):
                img = _set(image.img, at, new)
                idx = index or image.index
                img = img[:idx[-1]]
                if (img, tuple(idx)) in seen or (img == image.img and idx == image.index):
                    continue  # (a mutation that writes the bytes already there, or the bytes of an earlier one)
                seen.add((img, tuple(idx)))
                hit = next((x for x in all_units if x[0] <= at < x[0] + x[1]), u)  # (a stream header, an end frame: the unit hit)
                c = Case(f"{image.name}/{which}/{name}", image, img, list(idx), hit, (at, at + max(len(new), 1)))
                c.cls = model.classify(c)
                out.append(c)
    _CASES.setdefault(id(oracle), out)
    return out


def counts(case_list) -> Dict[str, Dict[str, int]]:
    t = {n: {k: 0 for k in CLASSES} for n in CODEC_NAME.values()}
    for c in case_list:
        t[CODEC_NAME[c.codec]][c.cls] += 1
    return t


def dump_oracle_calls(oracle, path: str) -> int:
    """Every decode the model asks of the oracle over the whole case list and its schedules, for oracle/asan_replay.c:
    records of [u32 codec][u32 capacity][u32 length][bytes] (codec | 0x100: a whole partition, else one unit)."""
    model = Model(oracle)
    for c in cases(oracle, model):
        for s in schedules(c, ("ample",)):
            model.run(c, s, 0)
    calls = list(model.calls)
    for c in cases(oracle):  # and every partition of every damaged range through the oracle's stream decoders (codec | 0x100)
        calls += [(c.codec | 0x100, c.img[c.index[p]:c.index[p + 1]], 1 << 18) for p in range(len(c.index) - 1)]
    with open(path, "wb") as f:
        for codec, blob, cap in calls:
            f.write(struct.pack("<III", codec, cap, len(blob)) + blob)
    return len(calls)


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import binding

    binding.lib()
    if len(sys.argv) > 2 and sys.argv[1] == "--dump":
        print(dump_oracle_calls(binding, sys.argv[2]), "decodes dumped")
    for codec, row in counts(cases(binding)).items():
        print(codec, row)
