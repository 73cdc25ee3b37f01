"""Which shapes of the Zstandard format does a set of frames contain?  (TEST INFRASTRUCTURE)

`shapes(data)` walks the frames of a partition - frame headers, block headers, literals section headers, Huffman table
descriptions, sequence counts, table modes, FSE table descriptions, and the sequences themselves (decoded, not executed) - and
returns a Counter of what it met, plus the widest sequence in bits.  MATRIX is the list of shapes the conformance corpus
(tests/zstd_conformance.py) has to contain; tests/test_zstd_conformance.py asserts it.

    python tests/tools/zstd_shapes.py        # the tally of the libzstd-written corpora of tests/test_zstd_model.py, then of the
                                             # conformance corpus, and what of MATRIX each one lacks
"""
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, "spark-s3-shuffle_amd")) if p not in sys.path]
import zstd_writer as zw  # noqa: E402

FIELDS = ("LL", "OF", "ML")
MODE = ("predef", "rle", "fse", "repeat")
LIT = ("raw", "rle", "huf", "treeless")
EDGES = (1, 31, 32, 4095, 4096, 131072)

MATRIX = (
    ["block:raw", "block:rle", "block:compressed", "block:raw:0", "block:rle:0", "block:raw:131072", "block:rle:131072",
     "last:raw", "last:rle", "last:compressed", "last:raw:0"]
    + ["lit:%s:sf%d" % (t, sf) for t in ("raw", "rle") for sf in (1, 2, 3)] + ["lit:%s:sf%d" % (t, sf) for t in ("huf", "treeless") for sf in range(4)]
    + ["lit:rle:n%d" % n for n in EDGES] + ["lit:raw:n%d" % n for n in EDGES[:-1]]
    + ["weights:direct", "weights:fse", "weights:direct:128", "huf:depth11", "huf:one_weight", "huf:256_symbols", "huf:symbol_255",
       "huf:streams_unequal", "huf:last_stream_1_byte", "treeless:after:compressed", "treeless:after:raw", "treeless:after:rle",
       "treeless:after:other_literals"]
    + ["nseq:0", "nseq:1", "nseq:1byte", "nseq:2bytes", "nseq:3bytes", "nseq:127:1byte", "nseq:127:2bytes", "nseq:128", "nseq:0x7EFF", "nseq:0x7F00",
       "nseq:above_0x7F00", "trailing_literals", "no_trailing_literals"]
    + ["modes:%s,%s,%s" % (a, b, c) for a in MODE[:3] for b in MODE[:3] for c in MODE[:3]]
    + ["repeat:%s:after_%s" % (f, m) for f in FIELDS for m in MODE[:3]] + ["repeat:%s:across_raw_or_rle_block" % f for f in FIELDS]
    + ["rle_code:LL:35", "rle_code:ML:52", "rle_code:OF:27"]
    + ["fse:%s:log%d" % (f, g) for f, mx in zip(FIELDS, (9, 8, 9)) for g in (5, mx)] + ["fse:less_than_one", "fse:zero_run", "fse:zero_run_flag_3"]
    + ["seq:wider_than_57_bits", "seq:plain_next_to_wide", "seq:ll_code_35", "seq:ml_code_52", "seq:wide:of_code_26", "seq:wide:of_code_27",
       "litrun:above_1024"]
    + ["rep:code%d:ll%s" % (c, z) for c in (1, 2, 3) for z in ("0", ">0")]
    + ["offset:%d:overlapping_above_64" % k for k in range(1, 9)]
    + ["fcs:%d" % w for w in (0, 1, 2, 4, 8)] + ["fcs:2:256", "fcs:2:65791", "single_segment", "window:mantissa", "did:1", "did:2", "did:4", "checksum",
                                                   "skippable:first", "skippable:between", "skippable:last"]
)


class _Back:
    """Reads a backward bit stream (RFC 8878 4.1)."""

    def __init__(self, b):
        self.v = int.from_bytes(b, "little")
        self.pos = self.v.bit_length() - 1  # below the closing 1-bit
        if self.pos < 0:
            raise ValueError("no end mark")

    def take(self, n):
        self.pos -= n
        if self.pos < 0:
            return (self.v << -self.pos) & ((1 << n) - 1)
        return (self.v >> self.pos) & ((1 << n) - 1)


def _huffman_weights(b):
    """(weights incl. the implied one, bytes used, kind) of a Huffman tree description."""
    hb = b[0]
    if hb >= 128:
        n = hb - 127
        w = [(b[1 + i // 2] >> 4) if i % 2 == 0 else (b[1 + i // 2] & 15) for i in range(n)]
        used, kind = 1 + (n + 1) // 2, "direct"
    else:
        norm, log, hdr, _, _ = zw.read_ncount(b[1:1 + hb])
        tab = zw.fse_table(norm, log)
        r = _Back(b[1 + hdr:1 + hb])
        s = [r.take(log), r.take(log)]
        w, k = [], 0
        while True:
            sym, nb, base = tab[s[k]]
            w.append(sym)
            if r.pos < nb:
                w.append(tab[s[k ^ 1]][0])
                break
            s[k] = base + r.take(nb)
            k ^= 1
        used, kind = 1 + hb, "fse"
    total = sum(1 << (x - 1) for x in w if x)
    log = total.bit_length()
    rest = (1 << log) - total
    w.append(rest.bit_length())
    return w, used, kind


def shapes(data, tally=None):
    """Counter of the shapes in the frames of `data` (valid frames: no checks beyond what parsing needs); key "max_seq_bits"
    holds the widest sequence (extra bits plus state updates)."""
    t = Counter() if tally is None else tally
    data = bytes(data)
    ip, nframes = 0, 0
    while ip < len(data):
        magic = int.from_bytes(data[ip:ip + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            t["skippable"] += 1
            t["skippable:first" if nframes == 0 else "skippable:between"] += 1
            ip += 8 + int.from_bytes(data[ip + 4:ip + 8], "little")
            if ip >= len(data) and nframes:
                t["skippable:between"] -= 1
                t["skippable:last"] += 1
            continue
        assert magic == 0xFD2FB528, "not a frame"
        nframes += 1
        fhd = data[ip + 4]
        ip += 5
        single, fcs_flag, did_flag = fhd >> 5 & 1, fhd >> 6, fhd & 3
        if single:
            t["single_segment"] += 1
        else:
            t["window:exp%d" % (data[ip] >> 3)] += 1
            if data[ip] & 7:
                t["window:mantissa"] += 1
            ip += 1
        if did_flag:
            t["did:%d" % (0, 1, 2, 4)[did_flag]] += 1
        ip += (0, 1, 2, 4)[did_flag]
        fcs_bytes = (1 if single else 0, 2, 4, 8)[fcs_flag]
        t["fcs:%d" % fcs_bytes] += 1
        if fcs_bytes == 2:
            t["fcs:2:%d" % (int.from_bytes(data[ip:ip + 2], "little") + 256)] += 1
        ip += fcs_bytes
        if fhd & 4:
            t["checksum"] += 1
        # blocks
        huf_seen_in = None   # kinds of blocks / literals met since the last Huffman table
        tabs = [None, None, None]   # (table, log, mode that defined it, non-compressed block met since)
        while True:
            bh = int.from_bytes(data[ip:ip + 3], "little")
            ip += 3
            last, btype, bsize = bh & 1, bh >> 1 & 3, bh >> 3
            name = ("raw", "rle", "compressed")[btype]
            t["block:" + name] += 1
            if last:
                t["last:" + name] += 1
            if btype < 2:
                if bsize in (0, 131072):
                    t["block:%s:%d" % (name, bsize)] += 1
                    if last:
                        t["last:%s:%d" % (name, bsize)] += 1
                ip += bsize if btype == 0 else 1
                if huf_seen_in is not None:
                    huf_seen_in.add(name)
                tabs = [x and x[:3] + (True,) for x in tabs]
            else:
                _compressed_block(data[ip:ip + bsize], t, tabs, huf_seen_in)
                ltype = data[ip] & 3
                if ltype == 2:
                    huf_seen_in = set()
                elif huf_seen_in is not None:
                    huf_seen_in.add("compressed" if ltype == 3 else "other_literals")
                ip += bsize
            if last:
                break
        if fhd & 4:
            ip += 4
    return t


def _compressed_block(b, t, tabs, huf_seen_in):
    ltype, sf = b[0] & 3, b[0] >> 2 & 3
    if ltype < 2:
        lh = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = int.from_bytes(b[:lh], "little") >> (3 if lh == 1 else 4)
        t["lit:%s:sf%d" % (LIT[ltype], lh)] += 1
        at = lh + (regen if ltype == 0 else 1)
    else:
        lh, bits = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
        v = int.from_bytes(b[:lh], "little")
        regen, comp = v >> 4 & ((1 << bits) - 1), v >> (4 + bits)
        t["lit:%s:sf%d" % (LIT[ltype], sf)] += 1
        at = lh + comp
        hp = lh
        if ltype == 2:
            w, used, kind = _huffman_weights(b[lh:lh + comp])
            hp += used
            t["weights:" + kind] += 1
            if kind == "direct" and len(w) - 1 == 128:
                t["weights:direct:128"] += 1
            depth = max(w)
            if depth == 11:
                t["huf:depth11"] += 1
            if len({x for x in w if x}) == 1:
                t["huf:one_weight"] += 1
            if sum(1 for x in w if x) == 256:
                t["huf:256_symbols"] += 1
            if len(w) == 256:
                t["huf:symbol_255"] += 1
        else:
            for k in sorted(huf_seen_in or ()):
                t["treeless:after:" + k] += 1
            if not huf_seen_in:
                t["treeless:after:compressed"] += 1
        if sf:
            sizes = [int.from_bytes(b[hp + 2 * k:hp + 2 * k + 2], "little") for k in range(3)]
            sizes.append(lh + comp - hp - 6 - sum(sizes))
            if len(set(sizes)) > 1:
                t["huf:streams_unequal"] += 1
            if sizes[3] == 1:
                t["huf:last_stream_1_byte"] += 1
    if regen in EDGES:
        t["lit:%s:n%d" % (LIT[ltype], regen)] += 1
    # sequences
    n = b[at]
    if n == 0:
        t["nseq:0"] += 1
        return
    if n < 128:
        form, at = "1byte", at + 1
    elif n < 255:
        n, form, at = ((n - 128) << 8) + b[at + 1], "2bytes", at + 2
    else:
        n, form, at = b[at + 1] + (b[at + 2] << 8) + 0x7F00, "3bytes", at + 3
    t["nseq:" + form] += 1
    for key, hit in (("nseq:1", n == 1), ("nseq:127:" + form, n == 127), ("nseq:128", n == 128), ("nseq:0x7EFF", n == 0x7EFF), ("nseq:0x7F00", n == 0x7F00),
                     ("nseq:above_0x7F00", n > 0x7F00)):
        if hit:
            t[key] += 1
    modes = [MODE[b[at] >> s & 3] for s in (6, 4, 2)]
    at += 1
    t["modes:" + ",".join(modes)] += 1
    for f in range(3):
        mode = modes[f]
        t["mode:%s:%s" % (FIELDS[f], mode)] += 1
        if mode == "predef":
            tabs[f] = (zw.fse_table(*zw.PREDEF[f]), zw.PREDEF[f][1], mode, False)
        elif mode == "rle":
            t["rle_code:%s:%d" % (FIELDS[f], b[at])] += 1
            tabs[f] = (zw.rle_table(b[at]), 0, mode, False)
            at += 1
        elif mode == "fse":
            norm, log, used, flags, lt1 = zw.read_ncount(b[at:])
            t["fse:%s:log%d" % (FIELDS[f], log)] += 1
            if lt1:
                t["fse:less_than_one"] += 1
            if flags:
                t["fse:zero_run"] += 1
            if any(norm[i:i + 4] == [0, 0, 0, 0] for i in range(len(norm))):
                t["fse:zero_run_flag_3"] += 1
            tabs[f] = (zw.fse_table(norm, log), log, mode, False)
            at += used
        else:
            t["repeat:%s:after_%s" % (FIELDS[f], tabs[f][2])] += 1
            if tabs[f][3]:
                t["repeat:%s:across_raw_or_rle_block" % FIELDS[f]] += 1
    r = _Back(b[at:])
    st = [r.take(tabs[f][1]) for f in range(3)]
    lit_used, widest, plain, wide = 0, 0, 0, 0
    for i in range(n):
        (lc, lnb, lbase), (oc, onb, obase), (mc, mnb, mbase) = (tabs[f][0][st[f]] for f in range(3))
        ov = (1 << oc) + r.take(oc)
        ml = zw.ML_BASE[mc] + r.take(zw.ML_BITS[mc])
        ll = zw.LL_BASE[lc] + r.take(zw.LL_BITS[lc])
        bits = oc + zw.ML_BITS[mc] + zw.LL_BITS[lc]
        if i + 1 < n:
            st[0] = lbase + r.take(lnb)
            st[2] = mbase + r.take(mnb)
            st[1] = obase + r.take(onb)
            bits += lnb + mnb + onb
        widest = max(widest, bits)
        if bits > 57:
            wide += 1
            if oc >= 26:
                t["seq:wide:of_code_%d" % oc] += 1
        else:
            plain += 1
        lit_used += ll
        if ov <= 3:
            t["rep:code%d:ll%s" % (ov, "0" if ll == 0 else ">0")] += 1
        elif ov - 3 <= 8 and ml > 64:
            t["offset:%d:overlapping_above_64" % (ov - 3)] += 1
        if lc == 35:
            t["seq:ll_code_35"] += 1
        if mc == 52:
            t["seq:ml_code_52"] += 1
        if ll > 1024:
            t["litrun:above_1024"] += 1
        t["of_code:%d" % oc] += 1
    assert r.pos == 0, "sequence stream not consumed exactly"
    if wide:
        t["seq:wider_than_57_bits"] += wide
        if plain:
            t["seq:plain_next_to_wide"] += 1
    t["max_seq_bits"] = max(t["max_seq_bits"], widest)
    t["trailing_literals" if lit_used < regen else "no_trailing_literals"] += 1


def missing(tally):
    return [k for k in MATRIX if not tally[k]]


def legacy_tally():
    """Every valid frame tests/test_zstd_model.py builds (written by libzstd's compressor)."""
    import zstd_model_lib
    from oracle import zstd_ref as z

    t = Counter()
    for _, data in zstd_model_lib.corpora():
        for level in (1, 3, 9, 19, -5):
            shapes(z.compress_stream(data, level), t)
        for comp in (z.compress(data, 1), z.compress(data, 6), z.compress_stream(data, 1, checksum=True), z.compress_stream(data, 3, chunk=5000, window_log=10)):
            shapes(comp, t)
    return t


def conformance_tally(generated=0):
    import zstd_conformance as zc

    t = Counter()
    for c in zc.fixed_corpus() + [zc.generated_case(s) for s in range(generated)]:
        if c.content is not None:
            shapes(c.data, t)
    return t


def _summary(t):
    keys = ("block:compressed", "lit:rle:sf1", "lit:rle:sf2", "lit:rle:sf3", "lit:treeless:sf0", "mode:LL:rle", "mode:LL:repeat", "mode:OF:repeat", "mode:ML:repeat",
            "nseq:3bytes", "window:mantissa", "fcs:8", "fcs:2", "did:1", "did:2", "did:4", "max_seq_bits", "huf:depth11", "seq:wider_than_57_bits")
    print("  " + ", ".join("%s=%d" % (k, t[k]) for k in keys))
    print("  mode triples: %d of 64;  rle literals: %d;  repeat codes with ll == 0: %s" % (
        sum(1 for k in t if k.startswith("modes:") and t[k]), sum(t["lit:rle:sf%d" % s] for s in (1, 2, 3)),
        [t["rep:code%d:ll0" % c] for c in (1, 2, 3)]))
    miss = missing(t)
    print("  %d of %d shapes of the matrix missing%s" % (len(miss), len(MATRIX), ": " + " ".join(miss) if miss else ""))


if __name__ == "__main__":
    print("libzstd-written corpora of tests/test_zstd_model.py:")
    _summary(legacy_tally())
    print("conformance corpus (tests/zstd_conformance.py, fixed list):")
    _summary(conformance_tally())
