"""The Zstandard conformance corpus (TEST INFRASTRUCTURE): small frames built construct by construct with tests/zstd_writer.py,
each aimed at one thing the format allows and libzstd 1.4.8's compressor does not happen to emit for the project's data
generators, plus a seeded generator that draws random combinations of the same controls (valid frames only).

A Case is one PARTITION (one or more frames, skippable ones among them): `data` its bytes, `content` what it must decode to
(None: it must be refused, with status `rc`), `emu`: small enough for the ISA interpreter.  tests/tools/zstd_shapes.py tallies
the shapes in here, and tests/test_zstd_conformance.py asserts that none of the matrix is missing."""
import itertools
from collections import namedtuple

import numpy as np

from zstd_writer import (BLOCK_MAX, LL, LL_BASE, LL_BITS, MAX_CODE, MAX_LOG, ML, ML_BASE, ML_BITS, OF, Frame, ll_code, ml_code, normalize, resolve_offset,
                         skippable)

Case = namedtuple("Case", "name data content rc emu")
BAD, UNSUPPORTED = -3, -6
EMU_BYTES, EMU_SEQS = 40_000, 400  # what the interpreter takes in a few seconds


def arbiter(case):
    """libzstd's decoder decodes a valid partition to the writer's content and refuses an invalid one - or the WRITER is wrong.
    Every leg (host model, interpreter, GPU) asks it before the product sees a frame."""
    from oracle import zstd_ref as z

    comp = np.frombuffer(case.data, np.uint8)
    if case.content is None:
        assert z.decompress(comp, 1 << 20) is None, "libzstd accepts %s" % case.name
    else:
        ref = z.decompress(comp, len(case.content) + 64)
        assert ref is not None and ref.tobytes() == case.content, "libzstd does not decode %s to the writer's content" % case.name


def _text(n, seed, nsym=40, skew=7):
    """n bytes over nsym symbols with very unequal frequencies (so a Huffman code has several lengths)."""
    rng = np.random.default_rng([seed, 77])
    p = np.array([2.0 ** (i * 5 % skew) for i in range(nsym)])
    return bytes(rng.choice(nsym, n, p=p / p.sum()).astype(np.uint8))


def _hist(n=200, seed=1):
    return bytes(np.random.default_rng([seed, 5]).integers(0, 256, n, dtype=np.uint8))


def _case(name, *frames, rc=0, emu=None):
    """frames: Frame objects (finished here) or bytes (skippable frames)."""
    data, content, nseq = b"", b"", 0
    for f in frames:
        if isinstance(f, Frame):
            b, c = f.finish()
            data += b
            content += c
            nseq += f.nseq
        else:
            data += f
    if emu is None:
        emu = len(content) <= EMU_BYTES and nseq <= EMU_SEQS
    return Case(name, data, content if rc == 0 else None, rc, emu)


# fixed sequences for a block whose fields use the given modes: a field in RLE mode keeps one code
def _mode_seqs(modes):
    lls = [5, 5, 5, 5] if modes[LL] == "rle" else [0, 3, 17, 40]
    mls = [7, 7, 7, 7] if modes[ML] == "rle" else [3, 10, 36, 70]
    offs = [5, 7, 9, 12] if modes[OF] == "rle" else [1, 30, -1, 60]
    return list(zip(lls, mls, offs))


def fixed_corpus():
    C = []
    add = C.append
    # ---- literals: type x size format x streams, at the edges of the size fields --------------------------------------------
    for n in (1, 31, 32, 4095, 4096, 131072):
        for sf in (1, 2, 3):
            if n < (32, 4096, 1 << 20)[sf - 1]:
                add(_case("lit_rle_%d_sf%d" % (n, sf), Frame().compressed(b"\x5a" * n, lit="rle", lit_sf=sf), emu=n <= 4096 or sf == 3))
                m = min(n, 131067)  # (a compressed block stays below 128 KiB: header + raw literals + sequence count)
                add(_case("lit_raw_%d_sf%d" % (m, sf), Frame().compressed(_hist(m, n), lit="raw", lit_sf=sf), emu=n <= 4096))
    t = _text(900, 3)
    for sf, streams in ((0, 1), (1, 4), (2, 4), (3, 4)):
        add(_case("lit_huf_sf%d" % sf, Frame().compressed(t[:40 if sf else 900], lit="huf", lit_sf=sf, streams=streams)))
        add(_case("lit_treeless_sf%d" % sf, Frame().compressed(t, lit="huf", streams=4, lit_sf=1)
                  .compressed(t[100:160 if sf else 800], lit="treeless", lit_sf=sf, streams=streams)))
    add(_case("lit_huf_big_sf2", Frame().compressed(_text(16000, 4), lit="huf", lit_sf=2, streams=4)))
    add(_case("lit_huf_big_sf3", Frame().compressed(_text(131072, 5, nsym=2, skew=1), lit="huf", lit_sf=3, streams=4), emu=False))
    # four streams of unequal lengths; the last one a single byte (13 literals: 4 + 4 + 4 + 1)
    w = [1, 1, 2, 3, 4]  # symbol 4: one bit
    add(_case("huf_streams_unequal_last_1_byte", Frame().compressed(bytes([0, 1, 2, 3, 0, 0, 1, 1, 4, 4, 4, 4, 4]), lit="huf", streams=4, weights=w)))
    add(_case("huf_streams_unequal", Frame().compressed(bytes([0, 1] * 50 + [4] * 100 + [3, 2] * 50 + [4] * 97), lit="huf", streams=4, weights=w, lit_sf=2)))
    # Huffman codes: depth 11, one weight for everybody, 256 symbols, both kinds of weight header
    deep = [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    add(_case("huf_depth11_direct", Frame().compressed(bytes(range(12)) * 9 + bytes([0, 1, 0, 1, 11, 0]), lit="huf", weights=deep, weight_header="direct")))
    add(_case("huf_depth11_fse_4streams", Frame().compressed((bytes(range(12)) + bytes([0, 1, 1, 0, 2])) * 40, lit="huf", weights=deep, weight_header="fse",
                                                     streams=4, lit_sf=1)))
    add(_case("huf_depth11_from_data", Frame().compressed(b"".join(bytes([k]) * (1 << k) for k in range(12)) + bytes(range(12)), lit="huf", max_depth=11,
                                                  streams=4, lit_sf=2)))
    add(_case("huf_single_weight_2", Frame().compressed(bytes([0, 1, 1, 0, 1, 1, 1, 0, 0]), lit="huf", weights=[1, 1])))
    add(_case("huf_single_weight_16", Frame().compressed(bytes(range(16)) * 5, lit="huf", weights=[1] * 16, weight_header="direct")))
    add(_case("huf_256_symbols_one_weight", Frame().compressed(bytes(range(256)) * 3, lit="huf", streams=4, lit_sf=2)))
    add(_case("huf_256_symbols", Frame().compressed(_text(6000, 6, nsym=256, skew=13), lit="huf", streams=4, lit_sf=2)))
    add(_case("huf_256_symbols_lt1_log5", Frame().compressed(_text(6000, 7, nsym=256, skew=11), lit="huf", streams=4, lit_sf=2, less_than_one=True, weight_log=5)))
    add(_case("huf_direct_128_weights", Frame().compressed(bytes(range(129)) * 2, lit="huf", weights=[1] * 128 + [8], weight_header="direct", streams=4, lit_sf=1)))
    add(_case("huf_symbol_255_sparse", Frame().compressed(bytes([255, 0, 255, 255, 7, 0, 255]) * 9, lit="huf", weights=[2] + [0] * 6 + [1] + [0] * 246 + [1, 3])))
    # treeless literals reuse the table across blocks
    for streams, sf in ((1, 0), (4, 1)):
        s = "1s" if streams == 1 else "4s"
        seq = [(5, 4, 3), (20, 9, -1)]
        add(_case("treeless_%s_next_block" % s, Frame().compressed(t, seq, lit="huf").compressed(t[50:300], seq, lit="treeless", streams=streams, lit_sf=sf)))
        add(_case("treeless_%s_across_raw_literals" % s, Frame().compressed(t, seq, lit="huf").compressed(_hist(100), seq, lit="raw")
                  .compressed(b"\x07" * 77, seq, lit="rle").compressed(t[50:300], seq, lit="treeless", streams=streams, lit_sf=sf)))
        add(_case("treeless_%s_across_raw_and_rle_blocks" % s, Frame().compressed(t, seq, lit="huf").raw(_hist(90)).rle(9, 300)
                  .compressed(t[50:300], seq, lit="treeless", streams=streams, lit_sf=sf).rle(1, 10).compressed(t[:99], lit="treeless", streams=streams, lit_sf=sf)))
        add(_case("treeless_%s_first_block_invalid" % s, Frame(strict=False).compressed(t[:60], lit="treeless", streams=streams, lit_sf=sf), rc=BAD))
        add(_case("treeless_%s_first_block_of_second_frame_invalid" % s, Frame().compressed(t, seq, lit="huf"),
                  Frame(strict=False).compressed(t[:60], lit="treeless", streams=streams, lit_sf=sf), rc=BAD))
    # ---- literal runs and the 1 KiB literal window --------------------------------------------------------------------------
    big = _text(9000, 8)
    for lit in ("raw", "huf"):
        kw = dict(lit=lit, streams=4 if lit == "huf" else 1, lit_sf=2 if lit == "huf" else None)
        add(_case("litrun_above_window_%s" % lit, Frame().compressed(big, [(10, 5, 3), (1500, 8, 100), (1024, 4, -1), (1025, 4, 2000), (3000, 70, 1)], **kw)))
        add(_case("litrun_straddles_refill_%s" % lit, Frame().compressed(big, [(60, 4, 7)] * 16 + [(64, 3, 9), (1, 3, 1), (63, 5, 900)] * 5 + [(1000, 3, -2), (24, 3, 4), (1, 3, 1024)]
                                                                      + [(65, 6, 33), (500, 4, -1)] * 4, **kw)))
    add(_case("block_literals_only", Frame().compressed(t, lit="huf").compressed(b"tail")))
    add(_case("block_one_sequence", Frame().compressed(b"abcdef", [(6, 10, 2)])))
    add(_case("block_one_sequence_no_trailing_literals", Frame().raw(b"0123456789").compressed(b"", [(0, 4, 10)])))
    add(_case("block_trailing_literals", Frame().compressed(t[:300], [(6, 10, 2), (0, 3, 1)], lit="huf")))
    # ---- sequence tables: every mode of every field --------------------------------------------------------------------------
    names = ("predef", "rle", "fse")
    for modes in itertools.product(names, repeat=3):
        add(_case("modes_" + "_".join(modes), Frame().raw(_hist(64)).compressed(t[:80], _mode_seqs(modes), modes=modes)))
    for first in names:
        m = (first,) * 3
        add(_case("repeat_after_" + first, Frame().raw(_hist(64)).compressed(t[:80], _mode_seqs(m), modes=m)
                  .compressed(t[80:160], _mode_seqs(m)[::-1], modes=("repeat",) * 3)
                  .compressed(t[:70], _mode_seqs(m), modes=("repeat", first, "repeat")).compressed(t[:70], _mode_seqs(m)[1:], modes=("repeat",) * 3)))
    add(_case("repeat_across_raw_and_rle_blocks", Frame().raw(_hist(64)).compressed(t[:80], _mode_seqs(("fse", "rle", "fse")), modes=("fse", "rle", "fse"))
              .raw(_hist(50)).rle(3, 40).compressed(t[:80], _mode_seqs(("fse", "rle", "fse")), modes=("repeat",) * 3)))
    add(_case("repeat_across_block_without_sequences", Frame().raw(_hist(64)).compressed(t[:80], _mode_seqs(("rle",) * 3), modes=("rle",) * 3)
              .compressed(b"no sequences").compressed(t[:80], _mode_seqs(("rle",) * 3), modes=("repeat",) * 3)))
    for f, nm in ((LL, "ll"), (OF, "of"), (ML, "ml")):
        m = ["predef"] * 3
        m[f] = "repeat"
        add(_case("repeat_%s_first_block_invalid" % nm, Frame(strict=False).compressed(t[:80], [(5, 7, 3)] * 3, modes=tuple(m)), rc=BAD))
        add(_case("repeat_%s_first_block_of_second_frame_invalid" % nm, Frame().compressed(t[:80], [(5, 7, 3)] * 3, modes=("fse",) * 3),
                  Frame(strict=False).compressed(t[:80], [(5, 7, 3)] * 3, modes=tuple(m)), rc=BAD))
    # RLE mode with the largest legal code of each field.  The format lets an offset code reach 31; a valid frame needs that much
    # history inside its window, and the arbiter takes windows up to 2^27 bytes: an offset of at most 2^27 is Offset_Value
    # 2^27 + 3 at most, code 27 (128 MiB of RLE blocks are 4 KB of frame).
    add(_case("rle_mode_ll_code_35", Frame().compressed(b"\x11" * 70000, [(65536 + 4000, 3, 9)], lit="rle", modes=("rle", "predef", "predef")), emu=True))
    add(_case("rle_mode_ml_code_52", Frame().raw(b"ab").compressed(b"", [(0, 65539 + 999, 2)], modes=("predef", "predef", "rle")), emu=True))
    add(_case("rle_mode_of_code_17", Frame().rle(0, BLOCK_MAX).raw(b"tail").compressed(b"xy", [(1, 9, BLOCK_MAX + 5)], modes=("predef", "rle", "predef")), emu=False))
    add(_case("rle_mode_of_code_20", Frame().raw(b"head").rle(0, BLOCK_MAX).rle(1, BLOCK_MAX).rle(2, BLOCK_MAX).rle(3, BLOCK_MAX).rle(4, BLOCK_MAX).rle(5, BLOCK_MAX)
              .rle(6, BLOCK_MAX).rle(7, BLOCK_MAX).compressed(b"xy", [(1, 4, 8 * BLOCK_MAX + 5), (0, 40, (1 << 20) - 3)], modes=("predef", "rle", "predef")), emu=False))
    add(_case("rle_mode_of_code_27", _rle_history(Frame(window=(17, 0)), 1024).compressed(b"xy", [(1, 40, 1 << 27), (0, 3, (1 << 27) - 1), (1, 70000, (1 << 27) - 3)],
              modes=("predef", "rle", "predef")), emu=False))
    # custom distributions: minimum and maximum accuracy log, "less than 1" probabilities, zero runs (flags 3, 3, 0 and 2)
    ll5 = [10, 0, 0, 0, 0, 0, 0, 6, 0, 0, 8] + [-1] * 8
    of5 = [0, 0, 0, 9, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, -1, -1, -1, -1, -1]
    ml5 = [-1, 0, 0, 0, 12, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 16]
    seqs5 = [(0, 7, 5), (7, 3, 10), (10, 23, 13), (11, 24, 14), (18, 7, 9), (15, 24, 30000 - 3 + 16384), (0, 3, 32768 + 7)]
    add(_case("fse_min_log_lt1_zero_runs", Frame().rle(0, 40000).raw(_hist(30000)).compressed(_hist(61, 2), seqs5, modes=("fse",) * 3,
              dists={LL: (ll5, 5), OF: (of5, 5), ML: (ml5, 5)}), emu=False))
    ll9 = [100, 50, 25, 13] + [10] * 28 + [9, 9, 13, 13]
    ll9[0] += 512 - sum(ll9)
    of8 = [40, 30, 20, 10] + [6] * 20 + [-1] * 4 + [0, 0, 0, 32]
    of8[0] += 256 - sum(abs(c) for c in of8)
    ml9 = [60] + [9] * 48 + [-1] * 3 + [17]
    ml9[0] += 512 - sum(abs(c) for c in ml9)
    seqs9 = [(k, 3 + k, 1 + k) for k in range(30)] + [(0, 3, -1), (0, 3, -2), (300, 900, 5000), (64, 34, 128), (2, 3, -3)]
    add(_case("fse_max_log_all_symbols", Frame().raw(_hist(6000)).compressed(_text(3000, 9), seqs9, lit="huf", streams=4, lit_sf=2, modes=("fse",) * 3,
              dists={LL: (ll9, 9), OF: (of8, 8), ML: (ml9, 9)})))
    add(_case("fse_auto_max_log_lt1", Frame().raw(_hist(6000)).compressed(_text(3000, 9), seqs9[:33], modes=("fse",) * 3, less_than_one=True)))
    # ---- sequence counts in every form ------------------------------------------------------------------------------------------
    tiny = [(0, 3, -1)]
    for n, nb in ((127, 1), (127, 2), (1, 2), (128, 2), (0x7EFF, 2), (0x7F00, 3), (0x7F00 + 300, 3), (0x7F00 + 255 + 256 * 40, 3)):
        add(_case("nseq_%d_in_%d_bytes" % (n, nb), Frame().raw(b"abcd").compressed(b"", tiny * n, modes=("rle",) * 3, nseq_bytes=nb)))
    add(_case("nseq_0x7EFF_predef", Frame().raw(b"abcd").compressed(b"q" * 10900, ([(0, 3, 3), (1, 3, -1), (0, 4, -2)] * 11000)[:0x7EFF], lit="rle", nseq_bytes=2)))
    add(_case("nseq_0x7F00_fse", Frame().raw(b"abcd").compressed(_text(10900, 1), ([(0, 3, 3), (1, 3, -1), (0, 4, -2)] * 11000)[:0x7F00], lit="huf", streams=4, lit_sf=2, modes=("fse",) * 3)))
    # ---- sequences wider than 57 bits next to minimal ones --------------------------------------------------------------------
    two = _text(BLOCK_MAX, 11, nsym=2, skew=1)
    wide1 = tiny * 5 + [(3, 3, 1), (65536 + 321, 16387 + 1000, 65000), (0, 3, -1), (1, 3, 2)] + tiny * 3
    wide2 = tiny * 3 + [(16384 + 77, 65539 + 5, 100000), (0, 3, -2), (32768 + 5, 3, 70001)] + tiny * 3
    for lit in ("rle", "huf"):
        kw = dict(lit="rle") if lit == "rle" else dict(lit="huf", streams=4, lit_sf=3)
        src1, src2 = (b"\x33" * 70000, b"\x34" * 50000) if lit == "rle" else (two[:70000], two[:50000])
        for modes in (("predef",) * 3, ("fse",) * 3):
            add(_case("wide_sequences_%s_literals_%s" % (lit, modes[0]), Frame().raw(_hist(500)).compressed(src1, wide1, modes=modes, **kw)
                      .compressed(src2, wide2, modes=modes, **kw), emu=lit == "rle" and modes[0] == "fse"))
    # (and with the largest offset codes: 16 + 14 + 26 extra bits, 15 + 16 + 26, 16 + 13 + 27 - Predefined tables hold offset codes up to 28)
    far1 = tiny * 3 + [(65536 + 9, 16387 + 11, (1 << 26) + 12345), (0, 3, -1), (1, 3, 2)] + tiny * 2
    far2 = tiny * 2 + [(32768 + 7, 65539 + 5, (1 << 26) - 3), (0, 3, -2), (1, 4, (1 << 27) - 4)] + tiny * 3
    far3 = tiny * 2 + [(65536 + 77, 8195 + 100, (1 << 27) - 3), (0, 3, 1 << 27)] + tiny * 2
    for modes in (("predef",) * 3, ("fse",) * 3):
        add(_case("wide_sequences_offset_codes_26_27_" + modes[0], _rle_history(Frame(window=(17, 0)), 1024).compressed(b"\x35" * 66000, far1, lit="rle", modes=modes)
                  .compressed(two[:33000], far2, lit="huf", streams=4, lit_sf=3, modes=modes).compressed(b"\x36" * 66000, far3, lit="rle", modes=modes), emu=False))
    # (the same switch in a frame of a few KB: codes of probability 1 in tables of the maximum accuracy log make the state updates
    #  9 + 8 + 9 bits, on top of 12 + 11 + 11 extra bits)
    small_wide = tiny * 5 + [(3, 3, 1), (2048 + 77, 2051 + 100, 4100), (0, 3, -1), (1, 3, 2)] + tiny * 3 + [(2048, 2051, 4101)] + tiny * 2
    add(_case("wide_sequences_small_fse", Frame().raw(_hist(4200)).compressed(_text(4300, 12), small_wide, lit="huf", streams=4, lit_sf=2, modes=("fse",) * 3,
              dists={LL: ([411, 50, 0, 50] + [0] * 26 + [1], 9), OF: ([200, 0, 55] + [0] * 9 + [1], 8), ML: ([511] + [0] * 46 + [1], 9)})))
    # ---- offsets -----------------------------------------------------------------------------------------------------------------
    add(_case("offsets_1_to_8_overlapping", Frame().raw(b"abcdefgh").compressed(b"XY", [(1 if k == 3 else 0, 100 + 37 * k, k) for k in range(1, 9)]
                                                                                  + [(1, 5000, 1), (0, 4200, 7), (0, 4097, 2), (0, 70, 4096), (0, 64, 4033), (0, 65, 4032)])))
    add(_case("offset_exactly_the_history", Frame().raw(b"0123456789").compressed(b"ab", [(2, 5, 12), (0, 3, 17), (0, 30, 20)])))
    add(_case("offset_one_beyond_the_history_invalid", Frame(strict=False).raw(b"0123456789").compressed(b"ab", [(2, 5, 13)]), rc=BAD))
    add(_case("offset_one_beyond_the_history_first_block_invalid", Frame(strict=False).compressed(b"ab", [(2, 5, 3)]), rc=BAD))
    add(_case("offset_one_beyond_the_history_second_frame_invalid", Frame().raw(_hist(100)), Frame(strict=False).raw(b"0123456789").compressed(b"ab", [(2, 5, 13)]), rc=BAD))
    add(_case("offsets_into_earlier_blocks", Frame().compressed(_hist(300), [(200, 8, 150)]).raw(_hist(100, 2)).rle(0x41, 5000).compressed(
        b"lmnop", [(1, 9, 5000 + 50), (0, 40, 5000 + 100 + 9 + 200), (1, 20, 4096), (1, 7, 3), (1, 600, 5488), (0, 5000, 4800)])))
    # ---- repeat offsets -----------------------------------------------------------------------------------------------------------
    est = [(1, 4, 11), (1, 4, 22), (1, 4, 33)]  # history 33, 22, 11
    for code in (1, 2, 3):
        for ll in (1, 0):
            add(_case("repeat_code_%d_ll_%d" % (code, ll), Frame().raw(_hist(60)).compressed(_hist(30, 3), est + [(ll, 5, -code), (1, 6, -1), (0, 3, -code), (ll, 4, -3), (ll, 4, -2)])))
    add(_case("repeat_codes_on_the_initial_history", Frame().raw(_hist(60)).compressed(b"xyz", [(1, 5, -1), (1, 5, -2), (1, 5, -3), (0, 5, -1), (0, 9, -3), (0, 3, -3), (0, 5, -2)])))
    add(_case("repeat_code_3_ll_0_rep0_2", Frame().raw(_hist(60)).compressed(b"xyz", [(1, 5, 2), (0, 70, -3), (1, 3, 1)])))
    # (repeat code 3 with ll == 0 and rep0 == 1 gives offset 0: the product refuses it, libzstd 1.4.8 quietly decodes it as offset 1 -
    #  no frame of this list can hold it, the arbiter accepts it)
    add(_case("repeat_history_across_blocks", Frame().raw(_hist(60)).compressed(_hist(30, 3), est).raw(b"raw").compressed(b"k", [(0, 5, -1), (1, 5, -2)])
              .rle(7, 20).compressed(b"k", [(0, 5, -2), (1, 5, -2)]).compressed(b"literals only").compressed(b"", [(0, 5, -3), (0, 5, -2)])
              .compressed(t[:90], [(0, 5, -1)], lit="huf").compressed(b"k" * 9, [(0, 5, -2), (9, 3, -3)], lit="rle")))
    # ---- frame headers ------------------------------------------------------------------------------------------------------------
    for n, fb in ((0, 1), (255, 1), (256, 2), (65791, 2), (300, 2), (70000, 4), (5, 4), (5, 8), (200000, 8), (5, 0)):
        for single in (True, False):
            if (single and fb == 0) or (fb == 1 and not single):
                continue
            f = Frame(single=single, fcs_bytes=fb)
            for at in range(0, n, 60000):
                f.raw(_hist(min(60000, n - at), at))
            add(_case("fcs_%d_in_%d_bytes%s" % (n, fb, "_single" if single else ""), f))
    add(_case("fcs_too_large_invalid", Frame(fcs_bytes=4, fcs_value=101).raw(_hist(100)), rc=BAD))
    add(_case("fcs_too_small_invalid", Frame(single=True, fcs_bytes=1, fcs_value=99, strict=False).raw(_hist(100)), rc=BAD))
    add(_case("fcs_2_bytes_wrong_bias_invalid", Frame(fcs_bytes=2, fcs_value=256 + 300).raw(_hist(300)), rc=BAD))
    for e, m in ((0, 1), (0, 7), (3, 5), (7, 2), (10, 3), (16, 7), (17, 0)):
        add(_case("window_exp%d_mantissa%d" % (e, m), Frame(window=(e, m)).raw(_hist(1024 + 128 * m)).compressed(b"w", [(1, 30, 1024 + 128 * m)])))
    for db in (1, 2, 4):
        add(_case("dictionary_id_0_in_%d_bytes" % db, Frame(did_bytes=db, fcs_bytes=2 if db == 2 else 0).raw(_hist(300)).compressed(b"d", [(1, 5, 7)])))
        add(_case("dictionary_id_nonzero_in_%d_bytes_unsupported" % db, Frame(did_bytes=db, did=1 << (8 * db - 1)).raw(_hist(300)), rc=UNSUPPORTED))
    add(_case("reserved_bit_invalid", Frame(reserved=True).raw(_hist(30)), rc=BAD))
    add(_case("reserved_bit_second_frame_invalid", Frame().raw(_hist(30)), Frame(reserved=True).raw(_hist(30)), rc=BAD))
    add(_case("skippable_before_between_after", skippable(b"first", 0), Frame().raw(_hist(100)).compressed(t[:50], [(3, 9, 2)], lit="huf"), skippable(b"", 7),
              skippable(b"x" * 300, 15), Frame(checksum=True).compressed(t[:50], [(3, 9, 2)], lit="huf"), skippable(b"last", 1)))
    add(_case("skippable_only", skippable(b"nothing else")))
    add(_case("checksum_on_mixed_blocks", Frame(checksum=True, fcs_bytes=4).compressed(t, [(5, 4, 3), (20, 9, -1)], lit="huf", streams=4, lit_sf=1, modes=("fse", "predef", "fse"))
              .raw(_hist(90)).rle(9, 300).compressed(t[50:300], [(5, 4, 3), (20, 9, -1)], lit="treeless", modes=("repeat",) * 3).compressed(b"\x01" * 40, [(4, 4000, 1)], lit="rle")))
    add(Case("checksum_wrong_invalid", _flip_last(Frame(checksum=True).raw(_hist(90)).compressed(b"c", [(1, 5, 7)]).finish()[0]), None, BAD, True))
    # ---- blocks ------------------------------------------------------------------------------------------------------------------
    add(_case("block_sizes_0_and_128k", Frame(window=(7, 1)).rle(7, BLOCK_MAX).raw(b"").rle(1, 0).raw(_hist(BLOCK_MAX)).compressed(b"e", [(1, 9, 147456)]).raw(b""), emu=False))
    add(_case("empty_last_raw_block", Frame().compressed(t[:50], [(3, 9, 2)]).raw(b"")))
    add(_case("empty_frame_single_empty_raw_block", Frame().raw(b"")))
    add(_case("empty_frame_empty_rle_block", Frame().rle(0, 0)))
    add(_case("last_block_rle", Frame().raw(b"r").rle(0x55, 1000)))
    add(_case("compressed_block_of_128k", Frame().raw(b"ab").compressed(b"", [(0, BLOCK_MAX, 2)]), emu=True))
    add(_case("compressed_block_above_128k_invalid", Frame(strict=False).raw(b"ab").compressed(b"", [(0, BLOCK_MAX + 1, 2)]), rc=BAD))
    add(_case("block_type_3_invalid", _reserved_block_type(), rc=BAD))
    assert len({c.name for c in C}) == len(C)
    return C


def _rle_history(frame, nblocks):
    """nblocks RLE blocks of 128 KiB with changing bytes: history for the largest offset codes at three bytes a block."""
    for k in range(nblocks):
        frame.rle(k * 7 & 255, BLOCK_MAX)
    return frame


def _flip_last(b):
    return b[:-1] + bytes([b[-1] ^ 0x80])


def _reserved_block_type():
    b = bytearray(Frame().raw(b"abc").finish()[0])
    b[6] |= 6  # Block_Type 3 (reserved); header: magic, descriptor, window
    return bytes(b)


# ---- the seeded structured generator (valid frames only) ------------------------------------------------------------------------
def _support(frame, f):
    return sorted({s for s, _, _ in frame.tabs[f][0]}) if frame.tabs[f] else []


GIVEN_WEIGHTS = ([1, 1, 2, 3, 4], [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [1] * 16, [2, 0, 0, 1, 1], [3, 1, 1, 2, 0, 0, 0, 3] + [0] * 120 + [3])


def _gen_block(rng, frame):
    hist = len(frame.out)
    modes, allowed = [], []
    for f in (LL, OF, ML):
        mode = str(rng.choice(["predef", "rle", "fse", "repeat"]))
        if mode == "repeat":
            sup = _support(frame, f)
            small = [c for c in sup if (f == LL and LL_BASE[c] <= 600) or (f == ML and ML_BASE[c] <= 600) or (f == OF and c >= 2 and (1 << c) - 3 <= hist)]
            if not small:
                mode = "predef"
            else:
                allow = small + ([c for c in sup if c < 2] if f == OF else [])
        if mode == "rle":
            allow = [int(rng.integers(0, 24))] if f == LL else [int(rng.integers(0, 40))] if f == ML else [int(rng.integers(2, max(3, min(hist + 3, 1 << 20).bit_length() - 1)))]
            if f == OF and (1 << allow[0]) - 3 > hist:
                mode = "predef"
        if mode in ("predef", "fse"):
            allow = list(range((36, 29, 53)[f])) if mode == "predef" else list(range(MAX_CODE[f] + 1))
        modes.append(mode)
        allowed.append(allow)
    nseq = int(rng.choice([1, 2, 5, 20, 130, 300]))
    seqs, reps, produced, lits_n = [], list(frame.reps), 0, 0
    for _ in range(nseq):
        if produced > 20000:
            break
        c = int(rng.choice([x for x in allowed[LL] if LL_BASE[x] <= 1500] or allowed[LL][:1]))
        ll = LL_BASE[c] + (int(rng.integers(0, 1 << LL_BITS[c])) if LL_BITS[c] else 0)
        if c >= 25 and rng.random() < 0.8:
            ll = LL_BASE[c] + int(rng.integers(0, 16))
        c = int(rng.choice([x for x in allowed[ML] if ML_BASE[x] <= (2100 if rng.random() < 0.1 else 80)] or allowed[ML][:1]))
        ml = ML_BASE[c] + (int(rng.integers(0, 1 << ML_BITS[c])) if ML_BITS[c] else 0)
        here = hist + produced + ll
        cands = []
        for code in allowed[OF]:
            if code >= 2:
                lo, hi = (1 << code) - 3, min(here, (2 << code) - 4)
                if lo <= hi:
                    cands.append(int(rng.integers(lo, hi + 1)) if rng.random() < 0.7 else (lo if rng.random() < 0.5 else hi))
            else:
                for rc in ((1,) if code == 0 else (2, 3)):
                    o, _ = resolve_offset(reps, ll, -rc)
                    if 0 < o <= here:
                        cands.append(-rc)
        if not cands:
            break
        reps_like = [x for x in cands if x < 0]
        off = int(rng.choice(reps_like)) if reps_like and rng.random() < 0.4 else int(rng.choice(cands))
        _, reps = resolve_offset(reps, ll, off)
        seqs.append((ll, ml, off))
        produced += ll + ml
        lits_n += ll
    if not seqs:
        modes = ["predef"] * 3
    kw = {}
    # the sequence count in a forced form (the 3-byte form needs 0x7F00 sequences: the fixed list has it)
    if seqs:
        kw["nseq_bytes"] = int(rng.choice([1, 2])) if len(seqs) < 128 else 2
    # an explicit distribution for some FSE_Compressed tables: any accuracy log that holds the block's codes, and codes of
    # probability 1 or "less than 1" that the block never uses
    dists = {}
    for f in (LL, OF, ML):
        if modes[f] == "fse" and rng.random() < 0.5:
            counts = [0] * (MAX_CODE[f] + 1)
            for ll, ml, off in seqs:
                counts[ll_code(ll) if f == LL else ml_code(ml) if f == ML else (off + 3 if off > 0 else -off).bit_length() - 1] += 4
            for c in rng.integers(0, len(counts), int(rng.integers(0, 6))):
                counts[int(c)] += 1
            lo = max(5, (2 * sum(1 for c in counts if c)).bit_length())
            if lo <= MAX_LOG[f]:
                log = int(rng.integers(lo, MAX_LOG[f] + 1))
                dists[f] = (normalize(counts, log, bool(rng.random() < 0.5)), log)
    kw["dists"] = dists
    lits_n += int(rng.choice([0, 0, 1, 30, 700]))
    lit = str(rng.choice(["raw", "rle", "huf", "treeless"]))
    if lit == "treeless" and frame.huf is None:
        lit = "huf"
    given = None
    if lit == "huf" and rng.random() < 0.25:  # given weights instead of a code built from the data
        given = GIVEN_WEIGHTS[int(rng.integers(len(GIVEN_WEIGHTS)))]
    if lit == "rle":
        lits = bytes([int(rng.integers(0, 256))]) * max(lits_n, 1)
    elif given:
        lits = bytes(rng.choice([k for k, w in enumerate(given) if w], max(lits_n, 1)).astype(np.uint8))
    elif lit == "treeless":
        sym = sorted(frame.huf)
        lits = bytes(rng.choice(sym, max(lits_n, 1)).astype(np.uint8))
    else:
        lits = _text(max(lits_n, 1), int(rng.integers(1 << 30)), nsym=int(rng.choice([2, 3, 17, 40, 129, 256])), skew=int(rng.choice([1, 3, 7, 12])))
    n = len(lits)
    if lit in ("raw", "rle"):
        kw["lit_sf"] = int(rng.choice([s for s in (1, 2, 3) if n < (32, 4096, 1 << 20)[s - 1]]))
    else:
        # (256 equally likely symbols do not compress: a size format has to hold n + a table description of up to 130 bytes)
        kw["streams"] = 1 if n < 16 or (n < 880 and rng.random() < 0.5) else 4
        kw["lit_sf"] = 0 if kw["streams"] == 1 else int(rng.choice([s for s in (1, 2, 3) if n < (0, 880, 14000, 1 << 18)[s]]))
        if given:
            kw["weights"], kw["weight_header"] = given, str(rng.choice(["auto", "direct"]))
        elif lit == "huf":
            kw["max_depth"] = int(rng.choice([11, 11, 8, 5])) if len(set(lits)) <= 32 else 11
            kw["weight_header"] = str(rng.choice(["auto", "fse", "direct"])) if 3 <= max(lits) <= 128 else "auto"
            kw["weight_log"] = int(rng.choice([5, 6]))
    frame.compressed(lits, seqs, lit=lit, modes=tuple(modes), less_than_one=bool(rng.random() < 0.5), **kw)


def generated_case(seed):
    """One partition of 1..3 frames drawn from the writer's controls; valid by construction.  Drawn: skippable frames, every
    frame-header field (single segment, content-size width, window exponent and mantissa, dictionary-id width with value 0,
    checksum), raw / RLE / compressed blocks incl. sizes 0 and 128 KiB and an empty last block, every literals type, size format
    and stream count, Huffman codes from the data (depth limit, weight header kind, accuracy log, "less than 1") or from given
    weights, the four table modes per field, explicit distributions at any accuracy log, the 1- and 2-byte sequence count, actual
    and repeat offsets.  Only the fixed list has what makes a frame invalid, the 3-byte sequence count (0x7F00 sequences), a
    compressed block that DECODES to exactly 128 KiB, and offset codes above 20."""
    rng = np.random.default_rng([seed, 0x2A57])
    parts = []
    for _ in range(int(rng.choice([1, 1, 2, 3]))):
        if rng.random() < 0.2:
            parts.append(skippable(bytes(int(rng.integers(0, 40))), int(rng.integers(0, 16))))
        f = Frame(checksum=bool(rng.random() < 0.4), did_bytes=int(rng.choice([0, 0, 1, 2, 4])))
        first = int(rng.integers(0, 3))
        if first == 0:
            f.raw(_hist(int(rng.integers(16, 400)), int(rng.integers(1 << 30))))
        elif first == 1:
            f.rle(int(rng.integers(0, 256)), int(rng.choice([16, 100, 5000, BLOCK_MAX])))
        else:
            f.compressed(_text(int(rng.integers(16, 900)), int(rng.integers(1 << 30))), lit=str(rng.choice(["raw", "huf"])))
        for _ in range(int(rng.integers(0, 6))):
            k = int(rng.integers(0, 8))
            if k == 0:
                f.raw(_hist(int(rng.choice([0, 1, 50, 3000, BLOCK_MAX], p=[0.24, 0.24, 0.24, 0.24, 0.04])), int(rng.integers(1 << 30))))
            elif k == 1:
                f.rle(int(rng.integers(0, 256)), int(rng.choice([0, 1, 70, 9000, BLOCK_MAX], p=[0.24, 0.24, 0.24, 0.24, 0.04])))
            else:
                _gen_block(rng, f)
        if rng.random() < 0.15:
            f.raw(b"")
        n = len(f.out)
        widths = [w for w in (0, 1, 2, 4, 8) if not (w == 1 and n > 255) and not (w == 2 and not 256 <= n <= 65791)]
        f.single = bool(rng.random() < 0.3 and n >= max(f.max_offset, f.max_block) and n > 0)
        f.fcs_bytes = int(rng.choice([w for w in widths if w or not f.single]))
        if f.fcs_bytes == 1 and not f.single:
            f.fcs_bytes = 0
        if not f.single:
            e = max(n - 1, f.max_offset - 1, f.max_block - 1, 1023).bit_length() - 10 + int(rng.integers(0, 3))
            f.window = (e, int(rng.integers(0, 8)))
        parts.append(f)
        if rng.random() < 0.1:
            parts.append(skippable(b"tail"))
    return _case("generated_%d" % seed, *parts)
