"""A Zstandard frame WRITER at the level of the format specification (RFC 8878) - TEST INFRASTRUCTURE ONLY.

Not a compressor: the caller says, construct by construct, what a frame contains (header fields, block types, the literals
section's type / size format / streams / Huffman code, the sequences with their table modes and distributions), and gets the
bytes together with the content those bytes must decode to.  The writer executes its own sequences against its own output
buffer and repeat-offset history, so the expected content does not come from any decoder.  Written from RFC 8878 alone;
libzstd's DECODER (oracle/zstd_ref.decompress) is the arbiter of every frame built here, see tests/test_zstd_conformance.py.

    f = Frame(window=(0, 3), checksum=True)
    f.raw(b"abcd")
    f.compressed(b"xyz", [(1, 5, 4), (0, 3, -1)], lit="huf", streams=1, modes=("fse", "rle", "predef"))
    frame_bytes, content = f.finish()

A sequence is (literal_length, match_length, offset): offset > 0 is an actual distance (written as Offset_Value = offset + 3),
offset -1 / -2 / -3 is repeat code 1 / 2 / 3 (whose meaning depends on literal_length == 0, RFC 8878 3.1.1.5)."""
import bisect
import heapq

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 1 << 17
LL, OF, ML = 0, 1, 2
MAX_LOG = (9, 8, 9)
MAX_CODE = (35, 31, 52)
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
PREDEF = (
    ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6),
    ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5),
    ([1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
      1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1], 6),
)
MODES = {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}


def ll_code(v):
    return bisect.bisect_right(LL_BASE, v) - 1


def ml_code(v):
    return bisect.bisect_right(ML_BASE, v) - 1


# ---- bit streams ---------------------------------------------------------------------------------------------------------------
class BackBits:
    """A bit stream that is READ backwards (RFC 8878 4.1): the fields are collected in the order the decoder reads them and
    written last-read first from bit 0 up; the first-read field ends below the closing 1-bit of the last byte."""

    def __init__(self):
        self.fields = []

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.fields.append((value, nbits))

    def bytes(self):
        acc = n = 0
        for value, nbits in reversed(self.fields):
            acc |= value << n
            n += nbits
        acc |= 1 << n
        return acc.to_bytes(n // 8 + 1, "little")


class FwdBits:
    def __init__(self):
        self.acc = self.n = 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits)
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- FSE (RFC 8878 4.1) -------------------------------------------------------------------------------------------------------
def fse_table(norm, log):
    """Decoding table of a normalised distribution: per state (symbol, number of bits, baseline)."""
    size = 1 << log
    assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
    sym_at = [None] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym_at[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym_at[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [abs(c) for c in norm]
    table = []
    for s in sym_at:
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


def rle_table(sym):
    return [(sym, 0, 0)]


def write_ncount(norm, log):
    """The table description (RFC 8878 4.1.1): accuracy log, then one variable-width value per symbol up to the last one with
    a probability, a 2-bit zero-run flag after every zero (3 = three more zeros and another flag)."""
    norm = list(norm)
    while norm[-1] == 0:
        norm.pop()
    assert 5 <= log and sum(abs(c) for c in norm) == 1 << log
    w = FwdBits()
    w.put(log - 5, 4)
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    sym, prev0 = 0, False
    while remaining > 1:
        if prev0:
            z = 0
            while norm[sym + z] == 0:
                z += 1
            sym += z
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
        count = norm[sym]
        sym += 1
        value, mx = count + 1, (2 * threshold - 1) - remaining
        if value < mx:
            w.put(value, nbits - 1)
        else:
            w.put(value + mx if value >= threshold else value, nbits)
        remaining -= abs(count)
        prev0 = count == 0
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    assert sym == len(norm)
    return w.bytes()


def read_ncount(b):
    """Inverse of write_ncount (tests/tools/zstd_shapes.py): (norm, log, bytes used, has a zero-run flag, has a -1)."""
    acc = int.from_bytes(b[:80], "little")
    at = 0

    def take(n):
        nonlocal at
        v = (acc >> at) & ((1 << n) - 1)
        at += n
        return v

    log = take(4) + 5
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    norm, prev0, flags = [], False, False
    while remaining > 1:
        if prev0:
            flags = True
            while True:
                f = take(2)
                norm += [0] * f
                if f != 3:
                    break
        mx = (2 * threshold - 1) - remaining
        low = (acc >> at) & (threshold - 1)
        if low < mx:
            value = take(nbits - 1)
        else:
            value = take(nbits)
            if value >= threshold:
                value -= mx
        count = value - 1
        remaining -= abs(count)
        norm.append(count)
        prev0 = count == 0
        while remaining < threshold and threshold > 1:
            nbits -= 1
            threshold >>= 1
        if len(norm) > 255 or at > 8 * len(b) + 8:
            raise ValueError("bad table description")
    return norm, log, (at + 7) // 8, flags, -1 in norm


def normalize(counts, log, less_than_one=False):
    """Some normalised distribution over the symbols with counts > 0 (never a single symbol: a second one gets probability 1);
    less_than_one = the rarest symbols are written as -1."""
    counts = list(counts)
    if sum(1 for c in counts if c) < 2:
        k = next(i for i, c in enumerate(counts) if c)
        if k + 1 < len(counts):
            counts[k + 1] = 1
        else:
            counts[k - 1] = 1
        counts[k] = max(counts[k], 4)
    size, total = 1 << log, sum(counts)
    norm = [max(1, c * size // total) if c else 0 for c in counts]
    while sum(norm) != size:
        d = size - sum(norm)
        k = max(range(len(norm)), key=lambda i: norm[i])
        norm[k] += d if d > 0 else max(d, 1 - norm[k])
    if less_than_one:
        norm = [-1 if c == 1 else c for c in norm]
    return norm


class FseEnc:
    """Symbols -> states of a decoding table, walked from the last symbol back."""

    def __init__(self, table):
        self.table = table
        self.by_sym = {}
        for x, (s, nb, base) in enumerate(table):
            self.by_sym.setdefault(s, []).append(x)
        self.memo = {}

    def last_state(self, sym):
        return max(self.by_sym[sym], key=lambda x: self.table[x][1])

    def state_before(self, sym, nxt):
        """The state that holds `sym` and can move to state `nxt`: (state, bits value, nbits)."""
        key = (sym, nxt)
        if key not in self.memo:
            for x in self.by_sym[sym]:
                _, nb, base = self.table[x]
                if base <= nxt < base + (1 << nb):
                    self.memo[key] = (x, nxt - base, nb)
                    break
            else:
                raise AssertionError("no state")
        return self.memo[key]

    def chain(self, syms):
        """[(state, update value, update nbits)] per symbol; the last one has no update."""
        out = [None] * len(syms)
        out[-1] = (self.last_state(syms[-1]), 0, 0)
        for i in range(len(syms) - 2, -1, -1):
            out[i] = self.state_before(syms[i], out[i + 1][0])
        return out


# ---- Huffman (RFC 8878 4.2) ---------------------------------------------------------------------------------------------------
def huf_lengths(counts, max_depth):
    """Code lengths of a Huffman code for the symbols with counts > 0, at most max_depth deep (counts are flattened until the
    tree fits)."""
    counts = {s: c for s, c in enumerate(counts) if c}
    assert len(counts) >= 2
    while True:
        heap = [(c, s, (s,)) for s, c in counts.items()]
        heapq.heapify(heap)
        depth = dict.fromkeys(counts, 0)
        while len(heap) > 1:
            c1, t1, m1 = heapq.heappop(heap)
            c2, t2, m2 = heapq.heappop(heap)
            for s in m1 + m2:
                depth[s] += 1
            heapq.heappush(heap, (c1 + c2, min(t1, t2), m1 + m2))
        if max(depth.values()) <= max_depth:
            return depth
        counts = {s: (c + 1) // 2 for s, c in counts.items()}


def weights_from_data(data, max_depth=11):
    counts = [0] * 256
    for v in data:
        counts[v] += 1
    if sum(1 for c in counts if c) < 2:
        counts[data[0] ^ 1] = 1
    depth = huf_lengths(counts, max_depth)
    top = max(depth.values())
    return [top + 1 - depth[s] if s in depth else 0 for s in range(max(depth) + 1)]


def huf_codes(weights):
    """{symbol: (code, nbits)}: symbols of one weight take consecutive codes, smaller weights (longer codes) first."""
    total = sum(1 << (w - 1) for w in weights if w)
    log = total.bit_length() - 1
    assert total == 1 << log and weights[-1] and log <= 11, (total, log)
    codes, at = {}, 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (at >> (w - 1), log + 1 - w)
                at += 1 << (w - 1)
    return codes


def huf_stream(codes, data):
    b = BackBits()
    for v in data:
        b.put(*codes[v])
    return b.bytes()


def huf_table_description(weights, kind="auto", log=6, less_than_one=False):
    """Direct (4 bits per weight, at most 128 weights) or FSE-compressed; the last symbol's weight is implied."""
    given = weights[:-1]
    assert 1 <= len(given) <= 255
    if kind == "auto":
        try:
            return huf_table_description(weights, "fse" if len(given) >= 12 else "direct", log, less_than_one)
        except AssertionError:
            return huf_table_description(weights, "direct")
    if kind == "direct":
        assert len(given) <= 128
        padded = given + [0] * (len(given) & 1)
        return bytes([127 + len(given)]) + bytes(padded[i] << 4 | padded[i + 1] for i in range(0, len(padded), 2))
    assert len(given) >= 2
    counts = [0] * 13
    for w in given:
        counts[w] += 1
    norm = normalize(counts, log, less_than_one)
    enc = FseEnc(fse_table(norm, log))
    # two interleaved states: the even weights through one, the odd ones through the other (RFC 8878 4.2.1.2)
    ch = [enc.chain(given[0::2]), enc.chain(given[1::2])]
    b = BackBits()
    b.put(ch[0][0][0], log)
    b.put(ch[1][0][0], log)
    for k in range(2, len(given)):
        _, value, nbits = ch[k & 1][k // 2 - 1]
        b.put(value, nbits)
    assert enc.table[ch[len(given) & 1][-1][0]][1] > 0  # the state that holds the last-but-one weight cannot be updated: the stream is dry
    body = write_ncount(norm, log) + b.bytes()
    assert len(body) < 128, "weights do not fit an FSE-compressed description"
    return bytes([len(body)]) + body


# ---- XXH64 (the published algorithm, for the optional content checksum) ---------------------------------------------------------
def xxh64(b, seed=0):
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & M

    def rnd(acc, v):
        return rotl((acc + v * P2) & M, 31) * P1 & M

    def u(i, n):
        return int.from_bytes(b[i:i + n], "little")

    n, i = len(b), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], u(i + 8 * k, 8))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, u(i, 8)), 27) * P1 + P4) & M
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (u(i, 4) * P1 & M), 23) * P2 + P3) & M
        i += 4
    while i < n:
        h = rotl(h ^ (b[i] * P5 & M), 11) * P1 & M
        i += 1
    h = (h ^ (h >> 33)) * P2 & M
    h = (h ^ (h >> 29)) * P3 & M
    return h ^ (h >> 32)


def resolve_offset(reps, ll, off):
    """(offset, new repeat history) of a sequence with literal length ll: off > 0 an actual offset, -1 / -2 / -3 a repeat code
    (RFC 8878 3.1.1.5: with ll == 0 the codes mean rep1, rep2, rep0 - 1)."""
    if off > 0:
        return off, [off, reps[0], reps[1]]
    idx = -off - (1 if ll else 0)
    if idx == 0:
        return reps[0], list(reps)
    offset = reps[idx] if idx < 3 else reps[0] - 1
    return offset, [offset, reps[0], reps[2]] if idx == 1 else [offset, reps[0], reps[1]]


def skippable(payload=b"", nibble=0):
    return (0x184D2A50 + nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + bytes(payload)


# ---- frames --------------------------------------------------------------------------------------------------------------------
class Frame:
    """window: (exponent, mantissa) of the window descriptor, None = the smallest power of two that holds the content (at
    least 1 KiB).  fcs_bytes: width of Frame_Content_Size (single-segment frames need at least 1); fcs_value overrides what is
    declared.  did_bytes / did: the Dictionary_ID field.  strict = False lets a test build frames that break the rules the
    writer otherwise keeps (offsets within history and window, blocks within min(window, 128 KiB), the Block_Size of a
    compressed block below 128 KiB)."""

    def __init__(self, single=False, fcs_bytes=0, window=None, did_bytes=0, did=0, checksum=False, reserved=False,
                 fcs_value=None, strict=True):
        assert fcs_bytes in (0, 1, 2, 4, 8) and did_bytes in (0, 1, 2, 4) and not (single and fcs_bytes == 0) and (single or fcs_bytes != 1)
        self.single, self.fcs_bytes, self.window, self.did_bytes, self.did = single, fcs_bytes, window, did_bytes, did
        self.checksum, self.reserved, self.fcs_value, self.strict = checksum, reserved, fcs_value, strict
        self.blocks = []            # (type, payload, Block_Size field)
        self.out = bytearray()
        self.reps = [1, 4, 8]
        self.huf = None             # codes of the last Huffman table
        self.tabs = [None, None, None]  # (decoding table, log) of the last LL / OF / ML table
        self.nseq = self.max_offset = self.max_block = 0

    # -- blocks
    def raw(self, data):
        data = bytes(data)
        self.blocks.append((0, data, len(data)))
        self.out += data
        self.max_block = max(self.max_block, len(data))
        return self

    def rle(self, byte, n):
        self.blocks.append((1, bytes([byte]), n))
        self.max_block = max(self.max_block, n)
        self.out += bytes([byte]) * n
        return self

    def compressed(self, lits=b"", seqs=(), lit="raw", lit_sf=None, streams=1, weights=None, max_depth=11, weight_header="auto",
                   weight_log=6, modes=("predef", "predef", "predef"), dists=None, nseq_bytes=None, less_than_one=False):
        """lits: all literals of the block.  lit: raw / rle / huf / treeless; lit_sf: header bytes 1 / 2 / 3 (raw, rle) or size
        format 0..3 (huf, treeless; 0 = the 1-stream form).  weights: the Huffman weights of symbols 0..last (else built from
        lits, at most max_depth deep).  modes: per LL / OF / ML predef / rle / fse / repeat; dists: {field: (norm, log)} for
        fse (else built from the block's codes at the field's maximum accuracy log)."""
        lits = bytes(lits)
        body = self._literals(lits, lit, lit_sf, streams, weights, max_depth, weight_header, weight_log, less_than_one)
        body += self._sequences(lits, list(seqs), modes, dists or {}, nseq_bytes, less_than_one)
        assert len(body) < BLOCK_MAX or not self.strict  # (libzstd refuses Block_Size == 128 KiB in a compressed block)
        self.max_block = max(self.max_block, len(body))
        self.blocks.append((2, body, len(body)))
        return self

    def _literals(self, lits, lit, sf, streams, weights, max_depth, weight_header, weight_log, less_than_one):
        n = len(lits)
        if lit in ("raw", "rle"):
            t = 0 if lit == "raw" else 1
            if lit == "rle":
                assert n >= 1 and lits == lits[:1] * n
            if sf is None:
                sf = 1 if n < 32 else 2 if n < 4096 else 3
            assert n < (32, 4096, 1 << 20)[sf - 1]
            hdr = bytes([t | n << 3]) if sf == 1 else (t | 1 << 2 | n << 4).to_bytes(2, "little") if sf == 2 else \
                (t | 3 << 2 | n << 4).to_bytes(3, "little")
            return hdr + (lits if lit == "raw" else lits[:1])
        table = b""
        if lit == "huf":
            if weights is None:
                weights = weights_from_data(lits, max_depth)
            self.huf = huf_codes(list(weights))
            table = huf_table_description(list(weights), weight_header, weight_log, less_than_one)
        else:
            assert lit == "treeless" and (self.huf is not None or not self.strict)
        codes = self.huf or {v: (0, 1) for v in set(lits)}
        if sf is None:
            sf = 0 if streams == 1 else 1
        assert (streams == 1) == (sf == 0)
        if streams == 1:
            payload = huf_stream(codes, lits)
        else:
            q = (n + 3) // 4
            parts = [huf_stream(codes, lits[k * q:(k + 1) * q] if k < 3 else lits[3 * q:]) for k in range(4)]
            assert n - 3 * q >= 0
            payload = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
        comp = len(table) + len(payload)
        bits = (10, 10, 14, 18)[sf]
        assert n < 1 << bits and comp < 1 << bits, (n, comp, sf)
        t = 2 if lit == "huf" else 3
        hdr = (t | sf << 2 | n << 4 | comp << (4 + bits)).to_bytes((3, 3, 4, 5)[sf], "little")
        return hdr + table + payload

    def _sequences(self, lits, seqs, modes, dists, nseq_bytes, less_than_one):
        n = len(seqs)
        if nseq_bytes is None:
            nseq_bytes = 1 if n < 128 else 2 if n < 0x7F00 else 3
        if n == 0:
            self._emit(lits, seqs)
            return b"\x00"
        if nseq_bytes == 1:
            assert n < 128
            head = bytes([n])
        elif nseq_bytes == 2:
            assert n < 0x7F00
            head = bytes([128 + (n >> 8), n & 255])
        else:
            assert n >= 0x7F00
            head = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
        # codes and extra bits
        codes, extra = ([], [], []), ([], [], [])
        for ll, ml, off in seqs:
            ov = off + 3 if off > 0 else -off
            assert ov >= 1 and (off > 0 or ov <= 3) and ml >= 3
            for f, c, v, nb in ((LL, ll_code(ll), ll - LL_BASE[ll_code(ll)], LL_BITS[ll_code(ll)]),
                                (OF, ov.bit_length() - 1, ov - (1 << (ov.bit_length() - 1)), ov.bit_length() - 1),
                                (ML, ml_code(ml), ml - ML_BASE[ml_code(ml)], ML_BITS[ml_code(ml)])):
                codes[f].append(c)
                extra[f].append((v, nb))
        head += bytes([MODES[modes[LL]] << 6 | MODES[modes[OF]] << 4 | MODES[modes[ML]] << 2])
        chains, logs = [None] * 3, [0] * 3
        for f in (LL, OF, ML):
            mode = modes[f]
            if mode == "predef":
                self.tabs[f] = (fse_table(*PREDEF[f]), PREDEF[f][1])
            elif mode == "rle":
                assert len(set(codes[f])) == 1
                self.tabs[f] = (rle_table(codes[f][0]), 0)
                head += bytes([codes[f][0]])
            elif mode == "fse":
                if f in dists:
                    norm, log = dists[f]
                else:
                    log = MAX_LOG[f]
                    counts = [0] * (MAX_CODE[f] + 1)
                    for c in codes[f]:
                        counts[c] += 1
                    norm = normalize(counts, log, less_than_one)
                assert 5 <= log <= MAX_LOG[f] and len(norm) <= MAX_CODE[f] + 1
                self.tabs[f] = (fse_table(norm, log), log)
                head += write_ncount(norm, log)
            else:
                assert mode == "repeat"
                if self.tabs[f] is None:  # (invalid on purpose: nothing to repeat)
                    assert not self.strict
                    self.tabs[f] = (rle_table(codes[f][0]), 0)
            chains[f] = FseEnc(self.tabs[f][0]).chain(codes[f])
            logs[f] = self.tabs[f][1]
        b = BackBits()
        for f in (LL, OF, ML):
            b.put(chains[f][0][0], logs[f])
        for i in range(n):
            for f in (OF, ML, LL):
                b.put(*extra[f][i])
            if i + 1 < n:
                for f in (LL, ML, OF):
                    b.put(chains[f][i][1], chains[f][i][2])
        self._emit(lits, seqs)
        return head + b.bytes()

    def _emit(self, lits, seqs):
        """Executes the block on the writer's own buffer and repeat history (RFC 8878 3.1.1.4, 3.1.1.5)."""
        out, reps, lp, start = self.out, self.reps, 0, len(self.out)
        for ll, ml, off in seqs:
            assert lp + ll <= len(lits)
            out += lits[lp:lp + ll]
            lp += ll
            offset, reps[:] = resolve_offset(reps, ll, off)
            self.max_offset = max(self.max_offset, offset)
            if self.strict:
                assert 0 < offset <= len(out), ("offset outside the history", offset, len(out))
            elif not 0 < offset <= len(out):
                out += b"?" * ml  # (an invalid frame: its content is never compared)
                continue
            at = len(out) - offset
            if offset >= ml:
                out += out[at:at + ml]
            else:
                pat = bytes(out[at:])
                out += (pat * (ml // offset + 1))[:ml]
        out += lits[lp:]
        self.nseq += len(seqs)
        self.max_block = max(self.max_block, len(out) - start)
        assert len(out) - start <= BLOCK_MAX or not self.strict

    # -- the frame
    def window_size(self):
        if self.single:
            return len(self.out) if self.fcs_value is None else self.fcs_value
        e, m = self.window
        return (1 << (10 + e)) + ((1 << (10 + e)) >> 3) * m

    def finish(self):
        if not self.blocks:
            self.raw(b"")
        content = bytes(self.out)
        if self.window is None and not self.single:
            self.window = (max(len(content) - 1, self.max_block - 1, 1023).bit_length() - 10, 0)
        if self.strict:  # what libzstd enforces and the product documents it does not
            assert self.max_offset <= self.window_size() and self.max_block <= min(max(self.window_size(), 1), BLOCK_MAX) or not content
        fcs_flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[self.fcs_bytes]
        fhd = fcs_flag << 6 | self.single << 5 | self.reserved << 3 | self.checksum << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[self.did_bytes]
        hdr = MAGIC + bytes([fhd])
        if not self.single:
            hdr += bytes([self.window[0] << 3 | self.window[1]])
        hdr += self.did.to_bytes(self.did_bytes, "little")
        if self.fcs_bytes:
            v = len(content) if self.fcs_value is None else self.fcs_value
            hdr += (v - 256 if self.fcs_bytes == 2 else v).to_bytes(self.fcs_bytes, "little")
        body = b""
        for k, (t, payload, size) in enumerate(self.blocks):
            body += ((k == len(self.blocks) - 1) | t << 1 | size << 3).to_bytes(3, "little") + payload
        if self.checksum:
            body += (xxh64(content) & 0xFFFFFFFF).to_bytes(4, "little")
        return hdr + body, content
