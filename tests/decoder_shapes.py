"""A spec-level corpus of VALID LZ4, Snappy and LZF blocks in which every token form, offset class and window phase of the
batch decoder (csrc/lz4_decode_batch.hip) occurs: what writers other than a greedy one emit (LZ4 HC, lz4-java's and
snappy-java's pure-Java compressors, compress-lzf) - non-minimal length forms, copy-4 tags, references at the format's largest
distance, far matches directly behind a flush of the staged window.  TEST INFRASTRUCTURE: no GPU, no product code.

A case is (name, codec, classes, block_bytes, expected_bytes[, units]):
  * expected_bytes is kept BY CONSTRUCTION: the writer appends to the plain text it is describing while it emits the element
    (a literal appends its bytes, a match appends a slice of the text so far, repeated when it overlaps) - no decoder runs;
  * classes is the set of class labels the case covers (LABELS[codec] is the full list; tests/test_decoder_shapes_cpu.py
    asserts that every label has a case);
  * literal bytes are random with a fixed seed (derived from the case's name), so a wrong source position does not produce the
    right byte by accident;
  * units is the partition's content piece by piece, (stored, payload, expected): one compressed block for most cases, several
    where the case is about frames / chunks following one another.  block_bytes is the payload of a one-unit case and the
    payloads joined otherwise.  partition_stream(case) wraps the units in the codec's stream framing.

The sweeps bracket the two constants of the kernel's staged window, S3S_BWIN (4544 bytes staged) and S3S_BHIST (2048 bytes kept
by a slide).  They are hard-coded here ON PURPOSE (WINDOW, HISTORY): the CPU check reads the #defines from the kernel's text and
fails when they move, instead of the corpus silently aiming beside a retuned window."""
from __future__ import annotations

import zlib
from typing import List, NamedTuple, Tuple

import numpy as np

import framing

LZ4, SNAPPY, LZF = 1, 2, 4
WINDOW, HISTORY = 4544, 2048


class Case(NamedTuple):
    name: str
    codec: int
    classes: frozenset
    block: bytes
    expected: bytes
    units: Tuple[Tuple[bool, bytes, bytes], ...]


# every distance a match / copy / reference of the corpus uses, per codec (filled while the cases are built)
DISTANCES = {LZ4: set(), SNAPPY: set(), LZF: set()}


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


class _Text:
    """The plain text a writer is describing."""

    def __init__(self, name: str, codec: int):
        self.name, self.codec, self.rng, self.out = name, codec, _rng(name), bytearray()

    def _lit(self, n: int) -> bytes:
        b = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        self.out += b
        return b

    def _copy(self, dist: int, n: int):
        assert 1 <= dist <= len(self.out), (self.name, dist, len(self.out))
        DISTANCES[self.codec].add(dist)
        start = len(self.out) - dist
        if n <= dist:
            self.out += self.out[start:start + n]
        else:  # the match overlaps its own output: the last `dist` bytes repeat
            pat = bytes(self.out[start:])
            self.out += (pat * (n // dist + 1))[:n]

    def small(self, lo: int, hi: int) -> int:
        return int(self.rng.integers(lo, hi + 1))


class _Lz4(_Text):
    def __init__(self, name):
        super().__init__(name, LZ4)
        self.seqs = []

    def seq(self, lit: int, dist: int, ml: int):
        b = self._lit(lit)
        self._copy(dist, ml)
        self.seqs.append((b, dist, ml))

    def done(self, last: int = 12, fill_to: int = 0):
        """ends the block with `last` literals, or as many as reach fill_to (the format's end conditions: the last five bytes
        are literals and the last match starts twelve bytes or more in front of the block's end - liblz4 enforces both)"""
        if fill_to:
            last = fill_to - len(self.out)
            assert last >= 12, (self.name, last)
        b = self._lit(last)
        return framing.lz4_block(self.seqs, b), bytes(self.out)


class _Snappy(_Text):
    def __init__(self, name, force_len_bytes=0):
        super().__init__(name, SNAPPY)
        self.els, self.force = [], force_len_bytes

    def lit(self, n: int):
        self.els.append(("lit", self._lit(n)))

    def copy(self, dist: int, n: int, kind: int = 0):
        """a copy of any length as tags of at most 64 bytes (copy-1: 4 .. 11 bytes, distance below 2048; copy-2: distance
        below 65536; kind 0: copy-2 where the distance fits, else copy-4)"""
        kind = kind or (2 if dist < 65536 else 4)
        assert kind == 4 or dist < 65536
        while n > 0:
            k = min(n, 64)
            if kind == 1:
                assert 4 <= n <= 11 and dist < 2048
            self._copy(dist, k)
            self.els.append(("copy", dist, k, kind))
            n -= k

    def done(self):
        return framing.snappy_block(self.els, force_len_bytes=self.force), bytes(self.out)


class _Lzf(_Text):
    def __init__(self, name):
        super().__init__(name, LZF)
        self.els = []

    def lit(self, n: int):
        """n literal bytes as runs of at most 32"""
        while n > 0:
            k = min(n, 32)
            self.els.append(("lit", self._lit(k)))
            n -= k

    def ref(self, dist: int, n: int):
        self._copy(dist, n)
        self.els.append(("ref", dist, n))

    def done(self):
        return framing.lzf_block(self.els), bytes(self.out)


def _case(w: _Text, classes, done=None) -> Case:
    block, expected = done if done is not None else w.done()
    return Case(w.name, w.codec, frozenset(classes), block, expected, ((False, block, expected),))


def _multi(name, codec, classes, units) -> Case:
    units = tuple(units)
    return Case(name, codec, frozenset(classes), b"".join(u[1] for u in units), b"".join(u[2] for u in units), units)


def partition_stream(case: Case) -> bytes:
    """The case as one partition of a fetched range: LZ4Block frames and the end frame (the token's level is the smallest
    block size that holds the frame, 32 KiB at least), a SnappyOutputStream image, or ZV chunks."""
    if case.codec == LZ4:
        out = bytearray()
        for stored, payload, expected in case.units:
            level = max(5, (max(len(expected), 1) - 1).bit_length() - 10)
            out += framing.lz4_frame(payload, expected, raw=stored, level=level)
        return bytes(out + framing.lz4_end_frame())
    if case.codec == SNAPPY:
        assert not any(u[0] for u in case.units)
        return framing.snappy_stream([u[1] for u in case.units])
    return b"".join(framing.lzf_chunk(payload, len(expected), stored) for stored, payload, expected in case.units)


# ---- the chain generator (moved here from tests/test_batch_decode_model.py) -----------------------------------------------
def _chain_sequences(rng, n_seq, max_out=30000):
    """Random (literal length, offset, match length) lists in which matches copy from inside earlier matches, from
    literal runs, from periodic patterns and across several of them — what the decoder's source redirection
    (a match inside the output of one earlier match reads from that match's source) has to get right."""
    seqs, pos, regions = [], 0, []  # regions: (start, end) of earlier match outputs
    for _ in range(n_seq):
        lit = int(rng.choice([0, 0, 0, 1, 2, 3, 5, 10, 14, 15, 16, 40]))
        pos += lit
        if pos == 0:
            lit = 4
            pos = 4
        ml = int(rng.choice([4, 5, 7, 8, 15, 16, 17, 19, 29, 32, 33, 48, 59, 64, 65, 100]))
        how = rng.integers(0, 8)
        if how <= 2 and regions:      # wholly inside one earlier match output (the last few)
            rs, re_ = regions[-int(rng.integers(1, min(len(regions), 6) + 1))]
            ml = min(ml, re_ - rs)
            src = int(rng.integers(rs, re_ - ml + 1))
            off = pos - src
        elif how == 3:                # short period
            off = int(rng.choice([1, 2, 3, 4, 5, 8]))
        elif how == 4 and regions:    # straddles the end of an earlier match output
            rs, re_ = regions[-1]
            off = pos - max(re_ - 2, 0)
        elif how == 5:                # into the own literals
            off = max(1, min(lit, pos))
        else:
            off = int(rng.integers(1, pos + 1))
        off = max(1, min(off, pos, 65535))
        seqs.append((lit, off, ml))
        regions.append((pos, pos + ml))
        pos += ml
        if pos > max_out:
            break
    return seqs


N_CHAIN_BLOCKS = 40
FAR_D = [2047, 2048, 2049, 4543, 4544, 4545, 4608, 8191, 8192, 32767, 65534, 65535]
FAR_M = [4, 16, 64, 65, 300, 5000]
FAR_RUN = 320  # sequences of one far-source run (the issue asks for 300 at least)


def _chain_lists():
    rng = np.random.default_rng(2311)
    lists = [_chain_sequences(rng, int(rng.integers(20, 400))) for _ in range(N_CHAIN_BLOCKS)]
    big = _chain_sequences(rng, 6000, max_out=60_000)
    return lists, big


# ---- LZ4 ------------------------------------------------------------------------------------------------------------------
LZ4_LEN_L = [0, 1, 14, 15, 16, 17, 269, 270, 271, 524, 525, 526]
LZ4_LEN_M = [4, 5, 18, 19, 20, 273, 274, 275, 528, 529, 530]
LZ4_PERIOD_D = list(range(1, 18)) + [31, 32, 33, 63, 64, 65]
LZ4_PERIOD_M = [4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 100, 300]
LZ4_STRADDLE_D = [2049, 2050, 2064, 2100, 2300]


def lz4_cases() -> List[Case]:
    cases = []
    # length forms: every (L, M) pair of the two lists, one case per L
    for L in LZ4_LEN_L:
        w = _Lz4("lz4.len.L%d" % L)
        w.seq(24, 9, 4)
        for M in LZ4_LEN_M:
            w.seq(L, w.small(1, min(len(w.out) + L, 4000)), M)
        cases.append(_case(w, ["lz4.len.L%d" % L] + ["lz4.len.M%d" % M for M in LZ4_LEN_M]))
    # periods and overlap: every (D, M) pair behind a 0-byte and behind a short literal run, one case per D
    for D in LZ4_PERIOD_D:
        w = _Lz4("lz4.period.D%d" % D)
        w.seq(70, 9, 4)
        for M in LZ4_PERIOD_M:
            w.seq(0, D, M)
            w.seq(w.small(1, 3), D, M)
        cases.append(_case(w, ["lz4.period.D%d" % D, "lz4.period.lit0", "lz4.period.litshort"] +
                           ["lz4.period.M%d" % M for M in LZ4_PERIOD_M]))
    # window base and far sources
    for D in FAR_D:
        w = _Lz4("lz4.far.D%d.pairs" % D)
        w.seq(D, D, 4)
        for M in FAR_M:
            w.seq(w.small(0, 3), D, M)
        cases.append(_case(w, ["lz4.far.D%d" % D] + ["lz4.far.M%d" % M for M in FAR_M]))
        w = _Lz4("lz4.far.D%d.run" % D)
        w.seq(D, D, 4)
        for _ in range(FAR_RUN):
            w.seq(w.small(0, 3), D, w.small(4, 12))
        cases.append(_case(w, ["lz4.far.D%d" % D, "lz4.far.run"]))
        w = _Lz4("lz4.far.D%d.run255" % D)
        w.seq(D, D, 4)
        for _ in range(FAR_RUN):
            w.seq(w.small(0, 3), D, w.small(274, 290))  # the match length carries a 255-chain: the byte-wise emitter
        cases.append(_case(w, ["lz4.far.D%d" % D, "lz4.far.run255"]))
    w = _Lz4("lz4.far.straddle")  # long matches whose source starts in front of the window base and ends inside the window
    w.seq(2400, 2400, 4)
    for D in LZ4_STRADDLE_D:
        for M in (300, 5000):
            w.seq(w.small(0, 3), D, M)
    cases.append(_case(w, ["lz4.far.straddle"]))
    # redirection chains
    lists, big = _chain_lists()
    for k, seqs in enumerate(lists + [big]):
        w = _Lz4("lz4.chain.%02d" % k if k < len(lists) else "lz4.chain.big")
        for lit, off, ml in seqs:
            w.seq(lit, off, ml)
        cases.append(_case(w, ["lz4.chain" if k < len(lists) else "lz4.chain.big"]))
    assert 55_000 <= len(cases[-1].expected) <= 65_000
    # block shapes
    for n in (1, 5, 300):
        w = _Lz4("lz4.block.litonly.%d" % n)
        cases.append(_case(w, ["lz4.block.litonly.%d" % n], w.done(last=n)))
    for size, per_seq in ((32768, 300), (65536, 600), (262144, 3000)):
        w = _Lz4("lz4.block.%d" % size)
        w.seq(100, 100, 4)
        while len(w.out) < size - 2 * per_seq - 300:
            lit = w.small(0, per_seq // 10)
            reach = min(len(w.out) + lit, 65535)
            dist = reach if w.small(0, 7) == 0 else w.small(1, reach)  # the largest distance the position allows, now and then
            w.seq(lit, dist, w.small(4, per_seq))
        cases.append(_case(w, ["lz4.block.%d" % size], w.done(fill_to=size)))
        assert size < 65536 or 65535 in DISTANCES[LZ4]
    units = []
    for k in range(3):
        if k == 1:
            raw = _rng("lz4.block.raw_between.raw").integers(0, 256, 300, dtype=np.uint8).tobytes()
            units.append((True, raw, raw))
        else:
            w = _Lz4("lz4.block.raw_between.%d" % k)
            w.seq(40, 40, 100)
            w.seq(3, 7, 33)
            units.append((False,) + w.done())
    cases.append(_multi("lz4.block.raw_between", LZ4, ["lz4.block.raw_between"], units))
    return cases


# ---- Snappy ---------------------------------------------------------------------------------------------------------------
SN_LIT = [1, 59, 60, 61, 62, 255, 256, 257, 258, 4095, 32768]
SN_BIG_LIT_A = [895, 896, 897]
SN_BIG_LIT_B = [65535, 65536, 65537]
SN_COPY1_D = [1, 2, 3, 4, 255, 256, 257, 2047]
SN_COPY2_D = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4543, 4544, 4545, 65535]
SN_COPY4_LEN = [1, 4, 11, 12, 63, 64]
SN_COPY4_D = [1, 2048, 65535, 65536, 70000]


def snappy_cases() -> List[Case]:
    cases = []
    # literal forms
    for n in SN_LIT:
        w = _Snappy("snappy.lit.%d" % n)
        w.lit(n)
        if n < 32768:
            w.copy(1, 5)
            w.lit(n)
        cases.append(_case(w, ["snappy.lit.%d" % n]))
    for nb in (3, 4):  # the 3- and 4-byte length forms for lengths that would fit in fewer
        w = _Snappy("snappy.lit.form%d" % nb, force_len_bytes=nb)
        for n in (1, 10, 60, 61, 300, 5000):
            w.lit(n)
            w.copy(w.small(1, n), 9)
        cases.append(_case(w, ["snappy.lit.form%d" % nb]))
    w = _Snappy("snappy.lit.big.record")  # a chunk above 32 KiB: literals around the batch record's longest
    w.lit(33000)
    for n in SN_BIG_LIT_A:
        w.copy(10, 20)
        w.lit(n)
    w.copy(4000, 30)
    cases.append(_case(w, ["snappy.lit.big.%d" % n for n in SN_BIG_LIT_A]))
    for n in SN_BIG_LIT_B:
        w = _Snappy("snappy.lit.big.%d" % n)
        w.lit(n)
        w.copy(n, 40)
        w.lit(3)
        cases.append(_case(w, ["snappy.lit.big.%d" % n]))
    # copy forms
    for D in SN_COPY1_D:
        w = _Snappy("snappy.copy1.D%d" % D)
        w.lit(D + 3)
        for n in range(4, 12):
            w.copy(D, n, 1)
            if n & 1:
                w.lit(w.small(1, 3))
        cases.append(_case(w, ["snappy.copy1.D%d" % D] + ["snappy.copy1.len%d" % n for n in range(4, 12)]))
    for D in SN_COPY2_D:
        w = _Snappy("snappy.copy2.D%d" % D)
        w.lit(D + 3)
        for n in range(1, 65):
            w.copy(D, n, 2)
            if n % 3 == 0:
                w.lit(w.small(1, 3))
        cases.append(_case(w, ["snappy.copy2.D%d" % D] + ["snappy.copy2.len%d" % n for n in range(1, 65)]))
    for D in SN_COPY4_D:
        w = _Snappy("snappy.copy4.D%d" % D)
        w.lit(D + 3)
        for n in SN_COPY4_LEN:
            w.copy(D, n, 4)
            w.lit(w.small(0, 1) + 1)
        cases.append(_case(w, ["snappy.copy4.D%d" % D] + ["snappy.copy4.len%d" % n for n in SN_COPY4_LEN]))
    # a literal directly followed by a copy and a copy directly followed by a literal, at every literal length 1 .. 20
    w = _Snappy("snappy.join")
    w.lit(40)
    for n in range(1, 21):
        w.copy(w.small(1, 30), w.small(4, 20))
        w.lit(n)
        w.copy(w.small(1, n), w.small(1, 40))
    cases.append(_case(w, ["snappy.join.%d" % n for n in range(1, 21)]))
    # the far-source runs as copy-2 and as copy-4 elements (copy-4 is byte-wise in the kernel)
    for kind in (2, 4):
        for D in FAR_D:
            w = _Snappy("snappy.far%d.D%d" % (kind, D))
            w.lit(D)
            for M in FAR_M:
                if w.small(0, 1):
                    w.lit(w.small(1, 3))
                w.copy(D, M, kind)
            for _ in range(FAR_RUN):
                n = w.small(0, 3)
                if n:
                    w.lit(n)
                w.copy(D, w.small(4, 12), kind)
            cases.append(_case(w, ["snappy.far%d.D%d" % (kind, D), "snappy.far%d.run" % kind] +
                               ["snappy.far%d.M%d" % (kind, M) for M in FAR_M]))
    # the chain generator's blocks as Snappy elements
    lists, _ = _chain_lists()
    for k, seqs in enumerate(lists):
        w = _Snappy("snappy.chain.%02d" % k)
        for lit, off, ml in seqs:
            if lit:
                w.lit(lit)
            while ml > 0:
                n = min(ml, 64)
                w.copy(off, n, 1 if (off < 2048 and 4 <= n <= 11 and w.small(0, 1)) else 2)
                ml -= n
        cases.append(_case(w, ["snappy.chain"]))
    # preambles: minimal (one byte up to 127 decoded bytes, two up to 16383, three above), literal tags padded through
    # force_len_bytes (1 and 2 extra length bytes for lengths the tag itself holds), and an empty block
    for n, label in ((100, "snappy.preamble.1byte"), (127, "snappy.preamble.1byte"), (128, "snappy.preamble.2byte"),
                     (16383, "snappy.preamble.2byte"), (16384, "snappy.preamble.3byte")):
        w = _Snappy("snappy.preamble.%d" % n)
        w.lit(20)
        w.copy(20, n - 23)
        w.lit(3)
        cases.append(_case(w, [label]))
    for nb in (1, 2):
        w = _Snappy("snappy.preamble.padded%d" % nb, force_len_bytes=nb)
        for n in (1, 7, 33, 60):
            w.lit(n)
            w.copy(w.small(1, n), 12)
        cases.append(_case(w, ["snappy.preamble.padded"]))
    w = _Snappy("snappy.block.empty")
    cases.append(_case(w, ["snappy.block.empty"]))
    return cases


# ---- LZF ------------------------------------------------------------------------------------------------------------------
LZF_REF_LEN = [3, 4, 5, 6, 7, 8, 9, 10, 263, 264]
LZF_REF_D = [1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 255, 256, 257, 2047, 2048, 2049, 4543, 4544, 4545, 8191, 8192]
LZF_FAR_D = [2049, 4545, 8192]


def lzf_cases() -> List[Case]:
    cases = []
    # literal runs of every length, with a reference between them ...
    w = _Lzf("lzf.lit.separated")
    for n in range(1, 33):
        w.els.append(("lit", w._lit(n)))
        w.ref(w.small(1, n), w.small(3, 12))
    cases.append(_case(w, ["lzf.lit.%d" % n for n in range(1, 33)]))
    # ... and following one another with none
    w = _Lzf("lzf.lit.consecutive")
    for n in list(range(1, 33)) + [32, 32, 1, 1, 31]:
        w.els.append(("lit", w._lit(n)))
    w.ref(500, 20)
    cases.append(_case(w, ["lzf.lit.consecutive"] + ["lzf.lit.%d" % n for n in range(1, 33)]))
    # references
    for D in LZF_REF_D:
        w = _Lzf("lzf.ref.D%d" % D)
        w.lit(D + 2)
        for n in LZF_REF_LEN:
            w.ref(D, n)
            if n & 1:
                w.lit(w.small(1, 3))
        for n in LZF_REF_LEN:  # ... once more back to back
            w.ref(D, n)
        cases.append(_case(w, ["lzf.ref.D%d" % D] + ["lzf.ref.len%d" % n for n in LZF_REF_LEN]))
    # the far-source run, short and long form
    for D in LZF_FAR_D:
        for form, lo, hi in (("short", 3, 8), ("long", 9, 40)):
            w = _Lzf("lzf.far.D%d.%s" % (D, form))
            w.lit(D)
            for _ in range(FAR_RUN):
                n = w.small(0, 3)
                if n:
                    w.lit(n)
                w.ref(D, w.small(lo, hi))
            cases.append(_case(w, ["lzf.far.D%d" % D, "lzf.far.run.%s" % form]))
    # chunk shapes
    w = _Lzf("lzf.chunk.65535")
    w.lit(64)
    while len(w.out) < 65535 - 600:
        if w.small(0, 3) == 0:
            w.lit(w.small(1, 40))
        w.ref(w.small(1, min(len(w.out), 8192)), w.small(3, 264))
    w.lit(65535 - len(w.out))
    cases.append(_case(w, ["lzf.chunk.65535"]))
    assert len(cases[-1].expected) == 65535 and len(cases[-1].block) <= 65535

    def small_chunk(name):
        w = _Lzf(name)
        w.lit(50)
        w.ref(50, 100)
        w.lit(2)
        w.ref(3, 9)
        return (False,) + w.done()

    raw = _rng("lzf.chunk.stored_between.raw").integers(0, 256, 300, dtype=np.uint8).tobytes()
    cases.append(_multi("lzf.chunk.stored_between", LZF, ["lzf.chunk.stored_between"],
                        [small_chunk("lzf.chunk.stored_between.0"), (True, raw, raw), small_chunk("lzf.chunk.stored_between.2")]))
    w = _Lzf("lzf.chunk.onebyte")
    w.lit(1)
    cases.append(_case(w, ["lzf.chunk.onebyte"]))
    cases.append(_multi("lzf.chunk.five", LZF, ["lzf.chunk.five"], [small_chunk("lzf.chunk.five.%d" % k) for k in range(5)]))
    return cases


# ---- the class labels every corpus has to cover ---------------------------------------------------------------------------
LABELS = {
    LZ4: (["lz4.len.L%d" % v for v in LZ4_LEN_L] + ["lz4.len.M%d" % v for v in LZ4_LEN_M] +
          ["lz4.period.D%d" % v for v in LZ4_PERIOD_D] + ["lz4.period.M%d" % v for v in LZ4_PERIOD_M] +
          ["lz4.period.lit0", "lz4.period.litshort"] +
          ["lz4.far.D%d" % v for v in FAR_D] + ["lz4.far.M%d" % v for v in FAR_M] +
          ["lz4.far.run", "lz4.far.run255", "lz4.far.straddle", "lz4.chain", "lz4.chain.big"] +
          ["lz4.block.litonly.%d" % v for v in (1, 5, 300)] + ["lz4.block.%d" % v for v in (32768, 65536, 262144)] +
          ["lz4.block.raw_between"]),
    SNAPPY: (["snappy.lit.%d" % v for v in SN_LIT] + ["snappy.lit.form3", "snappy.lit.form4"] +
             ["snappy.lit.big.%d" % v for v in SN_BIG_LIT_A + SN_BIG_LIT_B] +
             ["snappy.copy1.D%d" % v for v in SN_COPY1_D] + ["snappy.copy1.len%d" % v for v in range(4, 12)] +
             ["snappy.copy2.D%d" % v for v in SN_COPY2_D] + ["snappy.copy2.len%d" % v for v in range(1, 65)] +
             ["snappy.copy4.D%d" % v for v in SN_COPY4_D] + ["snappy.copy4.len%d" % v for v in SN_COPY4_LEN] +
             ["snappy.join.%d" % v for v in range(1, 21)] +
             ["snappy.far%d.D%d" % (k, v) for k in (2, 4) for v in FAR_D] +
             ["snappy.far%d.M%d" % (k, v) for k in (2, 4) for v in FAR_M] + ["snappy.far2.run", "snappy.far4.run"] +
             ["snappy.chain", "snappy.preamble.1byte", "snappy.preamble.2byte", "snappy.preamble.3byte",
              "snappy.preamble.padded", "snappy.block.empty"]),
    LZF: (["lzf.lit.%d" % v for v in range(1, 33)] + ["lzf.lit.consecutive"] +
          ["lzf.ref.D%d" % v for v in LZF_REF_D] + ["lzf.ref.len%d" % v for v in LZF_REF_LEN] +
          ["lzf.far.D%d" % v for v in LZF_FAR_D] + ["lzf.far.run.short", "lzf.far.run.long"] +
          ["lzf.chunk.65535", "lzf.chunk.stored_between", "lzf.chunk.onebyte", "lzf.chunk.five"]),
}

# the cases whose matches reach behind the staged window or around its base: the narrow alignment sweep of the GPU suite
FAR_PREFIXES = ("lz4.far.", "snappy.far2.", "snappy.far4.", "lzf.far.")

_BUILDERS = {LZ4: lz4_cases, SNAPPY: snappy_cases, LZF: lzf_cases}
_CACHE = {}


def cases(codec: int) -> List[Case]:
    """The corpus of one codec, built once per process; the cases are immutable."""
    if codec not in _CACHE:
        _CACHE[codec] = _BUILDERS[codec]()
    return _CACHE[codec]


def is_far(case: Case) -> bool:
    return case.name.startswith(FAR_PREFIXES)


def pack_range(case_list):
    """The cases as the partitions of one fetched range, one case per partition ->
    (image uint8, index int64[n + 1], decoded offsets int64[n + 1])."""
    streams = [partition_stream(c) for c in case_list]
    index = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum([len(c.expected) for c in case_list])]).astype(np.int64)
    return np.frombuffer(b"".join(streams), np.uint8), index, offs


def first_difference(case_list, offs, got, what=""):
    """None when `got` (the decoded range) holds every case's expected bytes, else a message that names the first case that
    differs and its first differing byte."""
    for k, c in enumerate(case_list):
        piece = bytes(got[int(offs[k]):int(offs[k + 1])])
        if piece != c.expected:
            at = next((i for i, (a, b) in enumerate(zip(piece, c.expected)) if a != b), min(len(piece), len(c.expected)))
            return "%s: case %s (partition %d, %d bytes) differs first at byte %d: got %s, expected %s" % (
                what, c.name, k, len(c.expected), at, piece[at:at + 8].hex(), c.expected[at:at + 8].hex())
    return None


def smallest_per_label(codec: int) -> List[Case]:
    """For every class label the case with the fewest decoded bytes that covers it (each case once)."""
    chosen = {}
    for label in LABELS[codec]:
        best = min((c for c in cases(codec) if label in c.classes), key=lambda c: (len(c.expected), c.name))
        chosen[best.name] = best
    return list(chosen.values())
