"""The COMPILED compress kernels (hipcc -S output, hand-written gfx950 blocks included) executed on the CPU by
tests/isa/gfx950_emu.py and compared bit for bit with the oracle; plus the wait-state check of the asm blocks.
Needs hipcc (cross-compiles without a GPU) but no device."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))
import corpus  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None,
                                reason="hipcc not available")


def _check(chunks, oracle, **kw):
    import lz4_kernel as lk

    res = lk.compress_chunks(chunks, **kw)
    for c, (payload, hdr, w) in zip(chunks, res):
        ref = oracle.lz4_compress_block(c)
        if payload is None:
            assert len(ref) >= len(c), "kernel stored RAW a chunk the reference compresses"
        else:
            assert np.array_equal(payload, ref), "compiled kernel differs from LZ4_compress_default (len %d)" % len(c)
        assert hdr[:8] == b"LZ4Block"
    return res


def test_compiled_window_paths_without_the_blocks(oracle):
    """the compiled C++ window paths (what the blocks fall back to in mid-window) on their own"""
    import lz4_kernel as lk
    import snappy_kernel as sk

    rng = np.random.default_rng(24)
    chunks = [corpus.chunk_corpus(k, n, rng) for k, n in [(7, 9000), (6, 5000), (2, 2500), (3, 4000), (1, 1500)]]
    _check(chunks, oracle, flags=("-DS3S_NO_WINDOW_ENGINE",))
    for c, (slot, sz, w) in zip(chunks, sk.compress_chunks(chunks, flags=("-DS3S_NO_WINDOW_ENGINE",))):
        assert bytes(slot[32:32 + sz - 4]) == bytes(oracle.snappy_compress_block(c))


@pytest.mark.parametrize("windows", [True, False])
def test_compiled_kernel_matches_oracle(oracle, windows):
    rng = np.random.default_rng(21)
    chunks = [corpus.chunk_corpus(k, n, rng) for k, n in
              [(7, 32768), (6, 9000), (3, 32768), (2, 4000), (5, 6000), (1, 3000), (0, 700), (4, 2500), (7, 13), (7, 12),
               (7, 1), (7, 300)]]
    # the last chunk ends the source allocation: any read past it faults in the interpreter
    _check(chunks, oracle, windows=windows)




def _lz4_sequences(block):
    """(literal length, match length) of every sequence of a raw LZ4 block (the last one has match length 0)"""
    b, i, out = bytes(block), 0, []
    while i < len(b):
        t = b[i]
        i += 1
        lit = t >> 4
        if lit == 15:
            while True:
                x = b[i]
                i += 1
                lit += x
                if x != 255:
                    break
        i += lit
        if i >= len(b):
            out.append((lit, 0))
            break
        i += 2
        ml = t & 15
        if ml == 15:
            while True:
                x = b[i]
                i += 1
                ml += x
                if x != 255:
                    break
        out.append((lit, ml + 4))
    return out


def _snappy_elements(block):
    """(literal length in front, copy length, copy tag bytes) of every copy element of a raw Snappy block"""
    b, i = bytes(block), 0
    while b[i] & 0x80:
        i += 1
    i += 1
    out, lit = [], 0
    while i < len(b):
        t = b[i]
        k = t & 3
        if k == 0:
            n = (t >> 2) + 1
            i += 1
            if n > 60:
                nb = n - 60
                n = int.from_bytes(b[i:i + nb], "little") + 1
                i += nb
            i += n
            lit = n
        else:
            ln, sz = (((t >> 2) & 7) + 4, 2) if k == 1 else ((t >> 2) + 1, 3 if k == 2 else 5)
            i += sz
            out.append((lit, ln, sz))
            lit = 0
    return out


def test_deferred_emission_covers_every_sequence_shape(oracle):
    """The flush of the window blocks (lz4_window_engine.inc S3S_ENGINE_FLUSH, .Ls_flush): every literal length it takes, with and
    without the extra length byte / with the two- and the three-byte copy, i.e. every byte count and every tail position of a lane"""
    import lz4_kernel as lk
    import snappy_kernel as sk

    rng = np.random.default_rng(31)
    # LZ4: literal runs 0 .. 14 (15 leaves the block: long form), match lengths around the one-byte boundary (18 / 19) and up to 273
    chunks = [corpus.planted_sequence_shapes(rng, 32768, range(0, 16), (4, 5, 7, 12, 17, 18, 19, 20, 33, 70, 150, 272, 273, 280)) for _ in range(2)]
    prof = {}
    _check(chunks, oracle, profile=prof)
    shapes = set()
    for c in chunks:
        shapes |= {(a, m >= 19) for a, m in _lz4_sequences(oracle.lz4_compress_block(c)) if m}
    assert {(a, e) for a in range(15) for e in (False, True)} <= shapes, sorted(shapes)
    # (most of these sequences must have gone through the block's record path, and the flush must have run)
    n_rec = sum(v[1] for k, v in prof.items() if k.startswith(".Lw_len"))  # .Lw_len's taken branch = one recorded sequence
    n_seq = sum(len(_lz4_sequences(oracle.lz4_compress_block(c))) for c in chunks)
    assert any(k.startswith(".Lw_flush") for k in prof) and n_rec > 0.5 * n_seq, (n_rec, n_seq)
    # Snappy: literal runs 0 .. 12 wait as records, 13 .. 20 go out at once behind a flush; two-byte copies (length < 12, offset
    # < 2048) and three-byte ones
    chunks = [corpus.planted_sequence_shapes(rng, 32768, range(0, 21), (4, 6, 11, 12, 13, 30, 64, 65, 90)) for _ in range(2)]
    prof = {}
    for c, (slot, sz, w) in zip(chunks, sk.compress_chunks(chunks, profile=prof)):
        ref = oracle.snappy_compress_block(c)
        assert bytes(slot[32:32 + sz - 4]) == bytes(ref)
        shapes |= {("s", min(a, 13), z) for a, ln, z in _snappy_elements(ref)}
    assert {("s", a, z) for a in range(14) for z in (2, 3)} <= shapes, sorted(x for x in shapes if x[0] == "s")
    assert any(k.startswith(".Ls_flush") for k in prof) and any(k.startswith(".Ls_frl") for k in prof)


def test_lds_race_winner_is_irrelevant(oracle):
    """same-address LDS stores of one instruction: any lane may win (tests/model proves it; here on the real code)"""
    rng = np.random.default_rng(22)
    order = np.random.default_rng(5)
    chunks = [corpus.chunk_corpus(k, 12000, rng) for k in (7, 2, 3)]
    prof = {}
    _check(chunks, oracle, lds_order=lambda n: order.permutation(n), profile=prof)
    assert any(k.startswith(".Lw_cfix") for k in prof), "the commit's repair loop must run when a lower lane wins a store"


def test_window_block_runs_most_windows(oracle):
    """the hand-written window block must actually be the path taken (not a silent fallback to the C++ path)"""
    import lz4_kernel as lk

    rng = np.random.default_rng(23)
    chunk = corpus.chunk_corpus(7, 32768, rng)
    prof = {}
    lk.compress_chunks([chunk], profile=prof)
    in_block = sum(v[0] for k, v in prof.items() if k.startswith(".Lw_"))
    total = sum(v[0] for v in prof.values())
    assert in_block > 0.6 * total, (in_block, total)


def test_asm_blocks_keep_their_wait_states():
    import hazards
    import lz4_kernel as lk

    text = lk.compile_asm()
    entry = lk.find_kernel(text, "lz4_compress_l2_kernelILb1E")
    asm_viol, cc_viol, cc_nops, _ = hazards.check_kernel(text, entry)
    assert not asm_viol, asm_viol
    assert not cc_viol, ("rule set stricter than the compiler", cc_viol[:3])


@pytest.mark.parametrize("windows", [True, False])
def test_compiled_snappy_kernel_matches_oracle(oracle, windows):
    """same for the Snappy compressor (its probe schedule lives in a device global: exercises symbol addressing)"""
    import snappy_kernel as sk

    rng = np.random.default_rng(31)
    chunks = [corpus.chunk_corpus(k, n, rng) for k, n in
              [(6, 9000), (7, 12000), (2, 3000), (3, 5000), (5, 2000), (0, 600), (6, 520), (7, 15), (7, 14), (7, 1)]]
    for c, (slot, sz, w) in zip(chunks, sk.compress_chunks(chunks, windows=windows)):
        ref = bytes(oracle.snappy_compress_block(c))
        assert sz - 4 == len(ref) and bytes(slot[32:32 + sz - 4]) == ref, "compiled Snappy kernel differs (len %d)" % len(c)
        assert int.from_bytes(bytes(slot[28:32]), "big") == len(ref)


def test_snappy_window_block_runs_most_windows(oracle):
    import snappy_kernel as sk

    rng = np.random.default_rng(33)
    chunk = corpus.chunk_corpus(7, 32768, rng)
    prof = {}
    (slot, sz, w), = sk.compress_chunks([chunk], profile=prof)
    assert bytes(slot[32:32 + sz - 4]) == bytes(oracle.snappy_compress_block(chunk))
    in_block = sum(v[0] for k, v in prof.items() if k.startswith(".Ls_"))
    assert in_block > 0.6 * sum(v[0] for v in prof.values())


def test_compiled_kernels_on_the_bench_workloads(oracle):
    """one block of each bench.py generator (TeraSort records, TPC-DS-like wide rows) through both compiled compressors"""
    import lz4_kernel as lk
    import snappy_kernel as sk
    from s3shuffle import datagen

    chunks = []
    for gen, seed in ((datagen.terasort_map_output, 2), (datagen.tpcds_wide_map_output, 3)):
        data, offs = gen(1 << 20, 4, seed=seed, map_id=1)
        data = np.asarray(data, dtype=np.uint8)
        p0 = int(offs[1])
        chunks.append(data[p0:p0 + 32768].copy())
    counts = []
    for c in chunks:  # instruction budget per 32 KiB block (all instruction kinds, interpreter count)
        prof = {}
        _check([c], oracle, profile=prof)
        counts.append(sum(v[0] for v in prof.values()))
        prof = {}
        (slot, sz, w), = sk.compress_chunks([c], profile=prof)
        assert bytes(slot[32:32 + sz - 4]) == bytes(oracle.snappy_compress_block(c))
        counts.append(sum(v[0] for v in prof.values()))
    print("instructions per block: lz4 terasort %d, snappy terasort %d, lz4 wide rows %d, snappy wide rows %d" % tuple(counts))
    # end of round 2 (r02k): 163.2k / 161.9k / 330.5k / 319.9k on these four blocks; round 3 (stream bytes through one
    # 80-byte load + ds_bpermute instead of a 64-lane x 16-byte load: + 13 instructions per LZ4 window, - 34 % of the
    # kernel's L1 lookups): 169.3k / 161.9k / 336.6k / 319.9k; round 5 (LZ4: speculative next-window gather, records at
    # the previous window's end, first-extension prefetch — + 46 instructions per window for - 26 % wait cycles, measured:
    # profiles/r05_experiments.md): 192.9k / 161.9k / 363.1k / 319.9k; a change that adds ~3 % shows up here
    assert counts[0] < 198_000 and counts[1] < 167_000 and counts[2] < 372_000 and counts[3] < 330_000, counts


def test_speculative_paths_of_the_window_block_are_taken(oracle):
    """round 5: the sequential entry, the stale-lane repair from the previous window's registers, the repeated gather and
    the prefetched first extension must all occur on ordinary data (a silent fall-back to .Lw_winm would hide a regression)"""
    import lz4_kernel as lk
    from s3shuffle import datagen

    data, offs = datagen.terasort_map_output(1 << 20, 4, seed=2, map_id=1)
    chunk = np.asarray(data[int(offs[1]):int(offs[1]) + 32768], dtype=np.uint8).copy()
    prof = {}
    _check([chunk], oracle, profile=prof)
    n = lambda name: sum(v[0] for k, v in prof.items() if k.startswith(name))  # noqa: E731
    assert n(".Lw_winf") > 20 * n(".Lw_winm") > 0, (n(".Lw_winf"), n(".Lw_winm"))
    assert n(".Lw_fix") > 0 and n(".Lw_exth") > 0 and n(".Lw_nopf") > 0, {k: v[0] for k, v in prof.items() if "fix" in k or "exth" in k}


def test_round4_window_block_still_builds_and_matches(oracle):
    """-DS3S_ENGINE_NO_SPEC = the block as it shipped in round 4 (the A/B baseline of profiles/r05_*): still exact"""
    rng = np.random.default_rng(29)
    chunks = [corpus.chunk_corpus(k, n, rng) for k, n in [(7, 20000), (3, 9000), (2, 3000)]]
    _check(chunks, oracle, flags=("-DS3S_ENGINE_NO_SPEC",))


def test_window_blocks_take_their_rare_paths(oracle):
    """planted copies at window-critical distances / lengths drive the out-of-line cases of both blocks (ip-2 two windows
    ahead or further, same-window re-entry, far dispatch, duplicate-hash groups): bit-exact there too"""
    import re

    import lz4_kernel as lk
    import snappy_kernel as sk

    sys.path.insert(0, os.path.join(HERE, "tools"))
    import isa_fuzz as F

    rng = np.random.default_rng(77)
    prof_l, prof_s = {}, {}
    for _ in range(2):
        chunks = [F.GENS[int(rng.integers(0, len(F.GENS)))](rng, max(1, F.pick_len(rng))) for _ in range(6)]
        _check(chunks, oracle, profile=prof_l)
        for c, (slot, sz, w) in zip(chunks, sk.compress_chunks(chunks, profile=prof_s)):
            assert bytes(slot[32:32 + sz - 4]) == bytes(oracle.snappy_compress_block(c))
    hit_l = {re.sub(r"\d*_\d+$", "", k) for k in prof_l if k.startswith(".Lw_")}
    hit_s = {re.sub(r"\d*_\d+$", "", k) for k in prof_s if k.startswith(".Ls_")}
    # (.Lw_regather / .Lw_winm / .Lw_fix / .Lw_exth = the speculation's paths; the commit's repair loop .Lw_cfix runs
    # only when a LOWER lane wins a same-address store: test_lds_race_winner_is_irrelevant shuffles the winner and requires it)
    # (.Lw_flush = the deferred emission's flush, .Lw_flw = asked for at a window's end, .Lw_frx = at a hand-back)
    assert {".Lw_pendb", ".Lw_dispf", ".Lw_dispx", ".Lw_dup", ".Lw_extb", ".Lw_noev", ".Lw_regather", ".Lw_winm",
            ".Lw_fix", ".Lw_exth", ".Lw_flush", ".Lw_flw", ".Lw_frx"} <= hit_l, hit_l
    # (.Ls_flush / .Ls_flw / .Ls_frx as above; .Ls_long = a literal run above 12 bytes, .Ls_frl = emitted at once behind a flush)
    assert {".Ls_dispf", ".Ls_dispx", ".Ls_dup", ".Ls_ext", ".Ls_cloop", ".Ls_noev", ".Ls_pendset", ".Ls_flush", ".Ls_flw",
            ".Ls_frx", ".Ls_long", ".Ls_frl"} <= hit_s, hit_s


def test_snappy_asm_block_keeps_its_wait_states():
    import hazards
    import lz4_kernel as lk

    text = lk.compile_asm("snappy_compress.hip")
    entry = lk.find_kernel(text, "snappy_compress_kernelILb1E")
    asm_viol, cc_viol, _, _ = hazards.check_kernel(text, entry)
    assert not asm_viol, asm_viol
    assert not cc_viol, ("rule set stricter than the compiler", cc_viol[:3])


# ---- the compiled block decoder (reduce side) under the interpreter: a byte-exact bounds check ---------------------
def _preamble_len(blk: bytes) -> int:
    n = sh = 0
    for b in blk:
        n |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            break
    return n


def test_compiled_decoder_valid_blocks(oracle):
    import decode_kernel as dk
    import framing

    rng = np.random.default_rng(41)
    chunks = [corpus.chunk_corpus(k, n, rng) for k, n in [(7, 20000), (6, 9000), (3, 5000), (1, 4000), (2, 3000), (7, 13)]]
    blocks = [(bytes(oracle.lz4_compress_block(c)), len(c)) for c in chunks]
    blocks.append((framing.lz4_hc(chunks[2], 9), len(chunks[2])))  # a foreign (non-greedy) compressor's block
    res, st, _ = dk.decode_blocks(blocks, fmt=0)
    assert st == 0 and res[:6] == [c.tobytes() for c in chunks] and res[6] == chunks[2].tobytes()
    sblocks = [(bytes(oracle.snappy_compress_block(c)), len(c)) for c in chunks]
    res, st, _ = dk.decode_blocks(sblocks, fmt=1)
    assert st == 0 and res == [c.tobytes() for c in chunks]


def test_decoder_asm_blocks_keep_their_wait_states():
    """round 6: the batch decoder has hand-written blocks too (the exact-length LDS store under v_cmpx, the LZ4 parse
    window) — their v_cmp -> v_cndmask / v_readlane distances are not padded by hipcc, so the checker walks them"""
    import hazards
    import lz4_kernel as lk

    text = lk.compile_asm("lz4_decode_batch.hip")
    for fmt in (0, 1, 2):
        entry = lk.find_kernel(text, "batch_decode_kernelILi%dE" % fmt)
        asm_viol, cc_viol, _, _ = hazards.check_kernel(text, entry)
        assert not asm_viol, asm_viol[:4]
        assert not cc_viol, ("rule set stricter than the compiler", cc_viol[:3])


def test_compiled_lz4_parse_block_takes_the_interior_windows(oracle):
    """the hand-written parse block must be where the windows of an ordinary block are parsed (and the generic front end
    only near the block's end / around byte-wise tokens): a silent fall-back to the compiled loop would keep the tests
    green and lose the point"""
    import decode_kernel as dk
    from s3shuffle import datagen

    d, _ = datagen.terasort_map_output(1 << 20, 1, seed=2, map_id=0)
    blk = d[32768 * 5:32768 * 6]
    c = bytes(oracle.lz4_compress_block(blk))
    prof = {}
    res, st, _ = dk.decode_blocks([(c, 32768)], fmt=0, profile=prof)
    assert st == 0 and res[0] == bytes(blk)
    walk = sum(v[0] for k, v in prof.items() if k.startswith(".Lp_wnext"))          # tokens walked inside the block (x 5)
    generic = sum(v[0] for k, v in prof.items() if k.startswith(".Lwalk_next"))     # ... by the generic front end
    assert walk > 4000 and walk > 20 * generic, (walk, generic)


@pytest.mark.parametrize("fmt", [1, 2], ids=["snappy", "lzf"])
def test_compiled_element_parse_block_takes_the_interior_windows(oracle, fmt):
    """the Snappy / LZF parse block (one asm statement per format: branch-free element decode, doubling or scalar walk, the
    literal-copy join through LDS marks, record stores) must be where ordinary blocks are parsed — match-dense wide rows
    (25 elements per window: the doubling walk) and TeraSort records (the scalar walk) — and the result must be the source"""
    import decode_kernel as dk
    from s3shuffle import datagen

    for gen, seed in ((datagen.tpcds_wide_map_output, 3), (datagen.terasort_map_output, 2)):
        d, _ = gen(1 << 19, 1, seed=seed, map_id=1)
        blk = d[32768 * 4:32768 * 5]
        c = bytes(oracle.snappy_compress_block(blk) if fmt == 1 else oracle.lzf_compress_block(blk))
        prof = {}
        res, st, _ = dk.decode_blocks([(c, 32768)], fmt=fmt, profile=prof)
        assert st == 0 and res[0] == bytes(blk)
        in_block = sum(v[0] for k, v in prof.items() if k.startswith(".Ls_"))
        generic_walk = sum(v[0] for k, v in prof.items() if k.startswith(".Lwalk_next"))
        total = sum(v[0] for v in prof.values())
        assert in_block > 0.25 * total and generic_walk < 0.01 * total, (in_block, generic_walk, total)


def test_compiled_decoder_on_chained_sources(oracle):
    """hand-made sequence lists whose matches copy from inside earlier matches, from literal runs and from periodic
    patterns (the generator of tests/decoder_shapes.py): what the decoder's source redirection, its 16-byte
    pieces and the period splats have to get right — through the COMPILED kernel, both formats, plus TeraSort blocks"""
    import decode_kernel as dk
    import framing
    import decoder_shapes as ds
    from s3shuffle import datagen

    rng = np.random.default_rng(7)
    lz, sn = [], []
    for _ in range(8):
        seqs = ds._chain_sequences(rng, int(rng.integers(50, 400)))
        blk = framing.lz4_block([(rng.integers(0, 256, l).astype(np.uint8).tobytes(), o, m) for l, o, m in seqs], b"abcdefg")
        lz.append((blk, framing.lz4_decode_py(blk)))
        els = []
        for l, o, m in seqs:
            if l:
                els.append(("lit", rng.integers(0, 256, l).astype(np.uint8).tobytes()))
            while m > 0:
                k = min(m, 64)
                els.append(("copy", o, k, 2))
                m -= k
        sblk = framing.snappy_block(els)
        want = framing.snappy_decode_py(sblk)
        if want is not None and 0 < len(want) <= 32768:
            sn.append((sblk, want))
    data, _ = datagen.terasort_map_output(1 << 20, 10, seed=3)
    for b in range(2):
        c = data[b * 32768:(b + 1) * 32768]
        lz.append((bytes(oracle.lz4_compress_block(c)), c.tobytes()))
        sn.append((bytes(oracle.snappy_compress_block(c)), c.tobytes()))
    for fmt, cases in ((0, lz), (1, sn)):
        res, st, _ = dk.decode_blocks([(b, len(w)) for b, w in cases], fmt=fmt)
        assert st == 0 and res == [w for _, w in cases], fmt



def test_compiled_batch_decoder_takes_blocks_above_32k(oracle):
    """round 4: LZ4Block frames of a writer with spark.io.compression.lz4.blockSize above 32k go through
    the BATCH decoder (records relative to the batch's first token / first output byte): a 70 000-byte and a 150 000-byte
    block of liblz4 (fast and HC: offsets up to 65 535 behind, far outside the LDS window), chained sources in a 90 KB block,
    payload and destination of exactly their sizes; a malformed big block is S3S_E_BAD_FRAME without leaving its buffers"""
    import decode_kernel as dk
    import framing
    import decoder_shapes as ds
    from s3shuffle import datagen

    rng = np.random.default_rng(47)
    big1 = datagen.terasort_map_output(70_000, 1, seed=5)[0]
    big2 = np.concatenate([datagen.tpcds_wide_map_output(100_000, 1, seed=6)[0][:100_000], corpus.chunk_corpus(7, 50_000, rng)])
    cases = [(bytes(framing.lz4_fast(big1)), big1.tobytes()), (framing.lz4_hc(big2, 9), big2.tobytes())]
    seqs = ds._chain_sequences(rng, 6000, max_out=60_000)
    b = framing.lz4_block([(rng.integers(0, 256, l).astype(np.uint8).tobytes(), o, m) for l, o, m in seqs], b"abcdefg")
    w = framing.lz4_decode_py(b)
    assert len(w) > 40_000
    cases.append((b, w))
    res, st, _ = dk.decode_blocks([(c, len(x)) for c, x in cases], fmt=0)
    assert st == 0 and res == [x for _, x in cases]
    # malformed: an offset that points in front of the block, 40 KB into a big block
    z = rng.integers(0, 256, 40_000).astype(np.uint8).tobytes()
    bad = framing.lz4_block([(z, 40_001, 8)], b"tail!")
    _, st, _ = dk.decode_blocks([(bad, 40_000 + 8 + 5)], fmt=0)
    assert st == -3


def test_compiled_batch_decoder_lzf_front_end(oracle):
    """round 4: LZF chunks (Spark's LZFCompressionCodec) through the batch decoder's third front end: blocks written by liblzf
    itself (tests/golden/lzf_liblzf.npz, up to the 65 535-byte chunk limit), blocks of the oracle's encoder over the corpora,
    a stored chunk; payload and destination of exactly their sizes; malformed blocks - a reference in front of the block, a
    literal run and a reference cut off by the end of the block, a block that decodes to more than its chunk header says -
    end in S3S_E_BAD_FRAME without an access outside the buffers"""
    import decode_kernel as dk

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lzf_liblzf.npz"))
    names = sorted(k[4:] for k in g.files if k.startswith("raw_"))
    cases = [(g["lzf_" + n].tobytes(), g["raw_" + n].tobytes()) for n in names]
    rng = np.random.default_rng(61)
    for kind, n in [(7, 20000), (3, 5000), (6, 6000), (1, 4000), (2, 40000), (7, 13)]:
        c = corpus.chunk_corpus(kind, n, rng)
        cases.append((bytes(oracle.lzf_compress_block(c)), c.tobytes()))
    blocks = [(b, len(w)) for b, w in cases]
    res, st, _ = dk.decode_blocks(blocks, fmt=2, methods=[2] * len(blocks))
    assert st == 0 and res == [w for _, w in cases]
    raw = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    res, st, _ = dk.decode_blocks([(raw, len(raw)), blocks[0]], fmt=2, methods=[0x10, 2])
    assert st == 0 and res == [raw, cases[0][1]]
    for bad, olen in ((bytes([0x20, 0x05]), 16), (bytes([0x03, 1, 2]), 16), (bytes([0x00, 7, 0xE0]), 16), (bytes([0x00, 7, 0x20, 0x00]), 2),
                      (bytes([0x00, 7, 0x20, 0x00]), 9), (cases[0][0][:-3], len(cases[0][1]))):
        _, st, _ = dk.decode_blocks([(bad, olen)], fmt=2, methods=[2])
        assert st == -3, (bad[:8], olen)


def test_compiled_ring_decoders(oracle):
    """the ring decoders (lz4_decompress_valu_kernel / snappy_decompress_valu_kernel: decode variant 3, and where LZ4 frames
    above 32 KiB go) as hipcc compiles them, payload buffer and destination of exactly their sizes (the payload rounded up to
    the dword its last byte sits in: these kernels read aligned dwords): oracle-compressed corpora, chained / periodic sources,
    a 100 000-byte frame of a foreign writer (far matches beyond the LDS ring), a wrong frame check, malformed blocks"""
    import decode_kernel as dk
    import framing
    import decoder_shapes as ds
    import xxhash

    def chk(b):
        return xxhash.xxh32(bytes(b), seed=0x9747B28C).intdigest() & 0x0FFFFFFF

    rng = np.random.default_rng(45)
    chunks = [corpus.chunk_corpus(k, n, rng) for k, n in [(7, 20000), (6, 9000), (3, 5000), (1, 4000), (2, 32768), (7, 13)]]
    blocks = [(bytes(oracle.lz4_compress_block(c)), len(c)) for c in chunks]
    res, st, _ = dk.decode_blocks(blocks, fmt=0, kernel="ring", checks=[chk(c) for c in chunks])
    assert st == 0 and res == [c.tobytes() for c in chunks]
    sblocks = [(bytes(oracle.snappy_compress_block(c)), len(c)) for c in chunks]
    res, st, _ = dk.decode_blocks(sblocks, fmt=1, kernel="ring")
    assert st == 0 and res == [c.tobytes() for c in chunks]
    # a frame above 32 KiB (lz4.blockSize = 128k on the writer): TeraSort-like records match far behind the ring
    from s3shuffle import datagen

    big = datagen.terasort_map_output(100_000, 1, seed=5)[0]
    blk = framing.lz4_hc(big, 9)
    res, st, _ = dk.decode_blocks([(blk, big.size)], fmt=0, kernel="ring", checks=[chk(big)])
    assert st == 0 and res[0] == big.tobytes()
    # chained sources
    cases = []
    for _ in range(4):
        seqs = ds._chain_sequences(rng, int(rng.integers(50, 300)))
        b = framing.lz4_block([(rng.integers(0, 256, l).astype(np.uint8).tobytes(), o, m) for l, o, m in seqs], b"abcdefg")
        cases.append((b, framing.lz4_decode_py(b)))
    res, st, _ = dk.decode_blocks([(b, len(w)) for b, w in cases], fmt=0, kernel="ring", checks=[chk(w) for _, w in cases])
    assert st == 0 and res == [w for _, w in cases]
    # the LZ4 ring kernel verifies the frame check itself; malformed payloads end in S3S_E_BAD_FRAME inside the buffers
    _, st, _ = dk.decode_blocks(blocks[:1], fmt=0, kernel="ring", checks=[chk(chunks[0]) ^ 1])
    assert st == -3
    z = b"abcdefgh"
    good = framing.lz4_block([(z, 8, 40)], z)
    orig = framing.lz4_decode_py(good)
    for bad in (framing.lz4_block([(z, 9, 4)], z), framing.lz4_block([(z, 8, 4)], z)[:-3], bytes([0xF0]) + b"\xff" * 40,
                framing.lz4_block([(z * 4, 8, 30000)], z)):
        _, st, _ = dk.decode_blocks([(bad, len(orig))], fmt=0, kernel="ring", checks=[chk(orig)])
        assert st == -3
    for bad in (framing.snappy_block([("lit", z), ("copy", 9, 4, 2)]), framing.snappy_block([("lit", z * 10)])[:-5],
                framing.snappy_block([("lit", z), ("copy", 4, 64, 2)] * 3, ulen=100)):
        _, st, _ = dk.decode_blocks([(bad, _preamble_len(bad))], fmt=1, kernel="ring")
        assert st == -3


def test_compiled_decoder_rejects_malformed_blocks_without_leaving_its_buffers():
    """the payload buffer ends with the block's last byte and the destination has exactly the declared size: any
    access outside either faults in the interpreter (MemFault), whatever the bytes say"""
    import decode_kernel as dk
    import framing

    z = b"abcdefgh"
    good = framing.lz4_block([(z, 8, 40)], z)
    orig = framing.lz4_decode_py(good)
    bad = [framing.lz4_block([(z, 9, 4)], z), framing.lz4_block([(z, 0, 4)], z), framing.lz4_block([(z, 8, 4)], z)[:-3],
           bytes([0xF0]) + b"\xff" * 40, framing.lz4_block([(z, 4, 19)], z)[:13] + b"\xff" * 9,
           framing.lz4_block([(z * 4, 8, 30000)], z), framing.lz4_block([(z, 8, 40)], z * 3)]
    for blk in bad:
        res, st, _ = dk.decode_blocks([(good, len(orig)), (blk, len(orig))], fmt=0)
        assert st == -3 and res[0] == orig
    rng = np.random.default_rng(42)
    d = corpus.chunk_corpus(2, 8192, rng)
    payload = framing.lz4_hc(d, 9)
    for _ in range(12):
        p = bytearray(payload)
        for _ in range(int(rng.integers(1, 6))):
            p[int(rng.integers(0, len(p)))] = int(rng.integers(0, 256))
        _, st, _ = dk.decode_blocks([(bytes(p), d.size)], fmt=0)
        assert st in (0, -3)
    sbad = [framing.snappy_block([("lit", z), ("copy", 9, 4, 2)]), framing.snappy_block([("lit", z), ("copy", 0, 4, 2)]),
            framing.snappy_block([("lit", z), ("copy", 4, 8, 2)], ulen=12), framing.snappy_block([("lit", z)], ulen=9),
            framing.snappy_block([("lit", z * 10)])[:-5], framing.snappy_block([("lit", z), ("copy", 4, 8, 4)])[:-2],
            framing.snappy_block([("lit", z), ("copy", 4, 64, 2)] * 3, ulen=100)]
    for blk in sbad:
        _, st, _ = dk.decode_blocks([(blk, _preamble_len(blk))], fmt=1)
        assert st == -3


# ---- one whole map-side call through the compiled kernels ------------------------------------------------------------------
def test_whole_map_side_call_through_the_compiled_kernels(oracle):
    """tests/isa/map_side.py: frame-check pre-pass, LZ4 blocks and end frames (persistent grid) — or the Snappy kernel —, item
    scan, gather into the .data image, per-partition checksums — the kernels of compress_core in its order, the item plan built like the host code
    builds it, every buffer of exactly its size.  Image, index and checksums equal the oracle's; a destination that is one
    byte short is S3S_E_CAPACITY and nothing is written behind it (the buffer ends there)."""
    import map_side as ms

    rng = np.random.default_rng(52)
    parts = [corpus.chunk_corpus(7, 70_000, rng).tobytes(), b"", corpus.chunk_corpus(3, 5, rng).tobytes(),
             rng.integers(0, 256, 33_000, dtype=np.uint8).tobytes(),  # incompressible: RAW frames, payload gathered from the source
             corpus.chunk_corpus(6, 9000, rng).tobytes(), b"", corpus.chunk_corpus(2, 32768, rng).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    for codec, algo in ((1, 1), (1, 2), (2, 2)):  # LZ4 + Adler32, LZ4 + CRC32, Snappy (own slot stride: a raw block may grow) + CRC32
        img, idx, sums = oracle.compress_map_output(codec, algo, data, offs)
        st, got, gi, gs = ms.compress_map_output(parts, algo, img.size, codec=codec)
        assert st == 0 and got == img.tobytes() and gi == list(idx) and gs == [int(x) for x in sums], (codec, algo)
    img, idx, sums = oracle.compress_map_output(1, 0, data, offs)
    st, got, gi, _ = ms.compress_map_output(parts, 0, img.size - 1)
    assert st == -2 and gi == list(idx)  # (the index says what it would have taken)
    st, got, gi, gs = ms.compress_map_output([b"", b"", b""], 1, 0)
    assert st == 0 and gi == [0, 0, 0, 0] and gs == [1, 1, 1]
    one = [bytes([7])]
    img, idx, sums = oracle.compress_map_output(1, 1, np.frombuffer(one[0], np.uint8), np.array([0, 1], np.int64))
    st, got, gi, gs = ms.compress_map_output(one, 1, img.size)
    assert st == 0 and got == img.tobytes() and gs == [int(sums[0])]


def test_batched_map_side_call_runs_its_tail_kernels_once(oracle):
    """round 6: a batched call launches scan / gather / checksum segments / checksum combine ONCE, every kernel finding its task
    through a TaskTail descriptor (tests/isa/map_side.py::compress_map_outputs_batch).  Three tasks of different shapes — one
    with empty partitions and a multi-block partition, one of a single tiny partition, one with no bytes at all — must each
    come out as the oracle's image, index and checksums in its OWN exactly-sized destination; a destination one byte short
    fails that task alone."""
    import map_side as ms
    from s3shuffle import datagen

    rng = np.random.default_rng(606)
    d, offs = datagen.terasort_map_output(150_000, 5, seed=2, map_id=3)
    t0 = [bytes(d[offs[p]:offs[p + 1]]) for p in range(5)]
    t0[1] = b""
    t0.append(bytes(corpus.chunk_corpus(2, 70_000, rng)))
    t1 = [bytes(rng.integers(0, 4, 37, dtype=np.uint8))]
    t2 = [b"", b""]
    tasks = [t0, t1, t2]
    for algo in (1, 2):
        want = []
        for parts in tasks:
            data = np.frombuffer(b"".join(parts), np.uint8)
            o = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
            want.append(oracle.compress_map_output(oracle.CODEC_LZ4, algo, data, o))
        res = ms.compress_map_outputs_batch(tasks, algo, [w[0].size for w in want])
        for (st, img, idx, sums), (wimg, widx, wsums) in zip(res, want):
            assert st == 0 and img == wimg.tobytes() and idx == [int(x) for x in widx]
            assert sums == [int(x) for x in wsums]
    caps = [w[0].size for w in want]
    caps[0] -= 1
    res = ms.compress_map_outputs_batch(tasks, 0, caps)
    assert res[0][0] == -2 and res[1][0] == 0 and res[2][0] == 0
    assert res[1][1] == want[1][0].tobytes()


def test_lz4_blocks_up_to_64k_on_the_map_side(oracle):
    """Round 4: spark.io.compression.lz4.blockSize up to 64k.  liblz4 parses every input below 65 547 bytes with the same
    8192 x u16 table (byU16), so the compiled window engine and the general parse take 64 KiB blocks as they are - positions
    use all 16 bits, the slot stride follows the block size (a kernel argument now).  Blocks of 65 536 / 60 000 / 40 000 bytes
    through both parses against the oracle's restatement of LZ4_compress_default (pinned to liblz4 1.9.3 up to 65 536 bytes);
    then a whole map-side call with 64 KiB blocks (frames' token level 6, stored frames of incompressible blocks,
    scan, gather, checksums) against the oracle's image."""
    import lz4_kernel as lk
    import map_side as ms

    rng = np.random.default_rng(64)
    from s3shuffle import datagen

    tera, _ = datagen.terasort_map_output(1 << 20, 2, seed=3)
    cases = [tera[:65536], corpus.chunk_corpus(3, 65536, rng), corpus.chunk_corpus(2, 40000, rng),
             rng.integers(0, 256, 65536, dtype=np.uint8), np.zeros(65536, np.uint8)]
    for windows in (True, False):  # (the general parse on two of them: it shares the engine's table code, the interpreter is slow)
        cases = cases if windows else cases[:2]
        got = lk.compress_chunks(cases, windows=windows, block=65536)
        for c, (payload, hdr, _) in zip(cases, got):
            want = oracle.lz4_compress_block(c)
            if want.size >= c.size:
                assert payload is None, (windows, c.size)  # stored frame
            else:
                assert payload is not None and payload.tobytes() == want.tobytes(), (windows, c.size, want.size)
    parts = [tera[:100_000].tobytes(), b"", rng.integers(0, 256, 66_000, dtype=np.uint8).tobytes(), corpus.chunk_corpus(7, 65537, rng).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    for block in (65536,):  # (49 152 and 40 000 bytes per block: on the GPU, tests/test_gpu_compress.py)
        img, idx, sums = oracle.compress_map_output(1, 1, data, offs, block)
        st, image, gi, gs = ms.compress_map_output(parts, 1, img.size, codec=1, block=block)
        assert st == 0 and image == img.tobytes() and gi == list(idx) and gs == [int(x) for x in sums], block


def test_whole_reduce_side_call_through_the_compiled_kernels(oracle):
    """the other direction: the .data image of a map output (written by the oracle) as one fetched batch range — per-partition
    checksums (compiled checksum kernels) equal the stored ones, the compiled frame discovery finds every LZ4Block frame, the
    compiled batch decoder + frame-check kernel turn them back into the partitions.  One flipped payload byte: the partition's
    checksum differs; with the checksum left aside, the frame check refuses the block."""
    import checksum_kernel as ck
    import decode_kernel as dk
    import discover_kernel as dsc

    rng = np.random.default_rng(53)
    parts = [corpus.chunk_corpus(7, 50_000, rng).tobytes(), b"", rng.integers(0, 256, 33_000, dtype=np.uint8).tobytes(),
             corpus.chunk_corpus(6, 9000, rng).tobytes(), corpus.chunk_corpus(3, 11, rng).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    img, idx, sums = oracle.compress_map_output(1, 1, data, offs)
    image = img.tobytes()
    assert ck.checksum_ranges(1, image, [int(x) for x in idx]) == [int(x) for x in sums]
    st, recs, outs = dsc.discover(image)
    assert st == 0 and outs[-1] == data.size
    st, back = dk.decode_range(image, recs, outs)
    assert st == 0 and back == data.tobytes()
    bad = bytearray(image)
    victim = next(r for r in recs if r[1] > 100 and r[4] == 0x20)  # an LZ4-coded block: damage a byte in its literals / tokens
    bad[victim[0] + 40] ^= 0x04
    p = max(k for k in range(len(parts)) if idx[k] <= victim[0])
    got = ck.checksum_ranges(1, bytes(bad), [int(x) for x in idx])
    assert [k for k in range(len(parts)) if got[k] != int(sums[k])] == [p]
    st, recs2, outs2 = dsc.discover(bytes(bad))
    assert st == 0 and recs2 == recs  # (the headers are intact)
    st, _ = dk.decode_range(bytes(bad), recs2, outs2)
    assert st == -3


def test_batched_reduce_side_call_through_the_compiled_kernels(oracle):
    """s3s_decompress_ranges_batch_device's launches for LZ4 (tests/isa/discover_kernel.py: decode_ranges_batch): several fetched
    ranges in one call — the batched discovery kernels walk their LzRange descriptors, frames_finish_batch rebases the records to
    absolute addresses, ONE decode launch (comp = dst = nullptr) and one frame-check launch cover every range.  A range with a
    broken chain, one whose destination is too small and one the host marked beforehand leave the others untouched; their
    frames become empty records and nothing is written to their destinations."""
    import discover_kernel as dsc

    rng = np.random.default_rng(55)
    srcs = [corpus.chunk_corpus(7, 90_000, rng).tobytes(), corpus.chunk_corpus(6, 9000, rng).tobytes(), b"",
            rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(), corpus.chunk_corpus(2, 40_000, rng).tobytes()]
    streams = [oracle.compress_stream(1, np.frombuffer(b, np.uint8)).tobytes() if b else b"" for b in srcs]
    res, dec_status = dsc.decode_ranges_batch(streams, [len(b) for b in srcs])
    assert dec_status == 0 and [st for st, _ in res] == [0] * 5 and [out for _, out in res] == srcs
    broken = bytearray(streams[3])
    broken[21 + 32768 + 9] ^= 0x40  # the second frame's compressedLen: the chain leaves the range
    res, dec_status = dsc.decode_ranges_batch([streams[0], bytes(broken), streams[4], streams[1], streams[1]],
                                              [len(srcs[0]), len(srcs[3]), len(srcs[4]) - 1, len(srcs[1]), len(srcs[1])], skip=(4,))
    assert dec_status == 0
    assert [st for st, _ in res] == [0, -3, -2, 0, -4]
    assert res[0][1] == srcs[0] and res[3][1] == srcs[1]



def test_wide_finish_rebases_any_frame_count(oracle):
    """frames_finish_batch_kernel rebases four records per lane and iteration (round 4: measured and shipped): the batched
    reduce-side call gives the right bytes and verdicts for frame counts that are not a multiple of four"""
    import discover_kernel as dsc

    rng = np.random.default_rng(56)
    srcs = [corpus.chunk_corpus(7, 300_000, rng).tobytes(), corpus.chunk_corpus(6, 9000, rng).tobytes(), b"",
            corpus.chunk_corpus(2, 40_000, rng).tobytes()]
    streams = [oracle.compress_stream(1, np.frombuffer(b, np.uint8)).tobytes() if b else b"" for b in srcs]
    res, dec_status = dsc.decode_ranges_batch(streams, [len(b) for b in srcs])
    assert dec_status == 0 and [st for st, _ in res] == [0] * 4 and [out for _, out in res] == srcs
    res, _ = dsc.decode_ranges_batch([streams[0], streams[3], streams[1]], [len(srcs[0]), len(srcs[3]) - 1, len(srcs[1])], skip=(2,))
    assert [st for st, _ in res] == [0, -2, -4] and res[0][1] == srcs[0]


def test_whole_snappy_reduce_side_call_through_the_compiled_kernels(oracle):
    """SnappyOutputStream images: snappy_count / snappy_emit (chunk chains of every partition, concatenated streams) feed the
    compiled batch decoder; chains that end early or run over their partition are S3S_E_BAD_FRAME without leaving the range"""
    import decode_kernel as dk
    import discover_kernel as dsc

    rng = np.random.default_rng(54)
    parts = [corpus.chunk_corpus(7, 50_000, rng).tobytes(), b"", rng.integers(0, 256, 33_000, dtype=np.uint8).tobytes(),
             corpus.chunk_corpus(6, 9000, rng).tobytes(), corpus.chunk_corpus(3, 11, rng).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    img, idx, _ = oracle.compress_map_output(2, 0, data, offs)
    image = img.tobytes()
    st, recs, outs = dsc.discover_snappy(image, idx)
    assert st == 0 and outs[-1] == data.size and len(recs) == 2 + 2 + 1 + 1
    st, back = dk.decode_range(image, recs, outs, fmt=1)
    assert st == 0 and back == data.tobytes()
    # two streams in one partition (a multi-spill merge): the second header is stepped over
    twice = image[: int(idx[1])] * 2
    st, recs, outs = dsc.discover_snappy(twice, [0, len(twice)])
    assert st == 0 and len(recs) == 4 and outs[-1] == 2 * len(parts[0])
    for cut in (1, 3, 4, 5, 17, 100, int(idx[1]) - 1):  # ends inside the header / a length word / a chunk
        assert dsc.discover_snappy(image[:cut], [0, cut])[0] == -3, cut
    bad = bytearray(image)
    bad[16:20] = (1 << 30).to_bytes(4, "big")  # a chunk length that runs over the partition
    assert dsc.discover_snappy(bytes(bad), idx)[0] == -3
    bad = bytearray(image)
    bad[3] ^= 1  # header magic
    assert dsc.discover_snappy(bytes(bad), idx)[0] == -3


def test_whole_lzf_reduce_side_call_through_the_compiled_kernels(oracle):
    """round 4: LZFInputStream images: the chunk walk of walk_partition_lzf (count -> scan -> emit; compressed and stored chunks,
    chunks of the 65 535-byte maximum, an empty partition, two streams in one partition) feeds the compiled batch decoder's LZF
    front end (stored chunks are copied); chains that end inside a header / a chunk, a wrong magic, a chunk type above 1 are
    S3S_E_BAD_FRAME without leaving the range"""
    import decode_kernel as dk
    import discover_kernel as dsc

    rng = np.random.default_rng(57)
    parts = [corpus.chunk_corpus(7, 150_000, rng).tobytes(), b"", rng.integers(0, 256, 70_000, dtype=np.uint8).tobytes(),
             corpus.chunk_corpus(6, 9000, rng).tobytes(), corpus.chunk_corpus(3, 11, rng).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    img, idx, _ = oracle.compress_map_output(4, 0, data, offs)
    image = img.tobytes()
    st, recs, outs = dsc.discover_snappy(image, idx, chunk_format=1)
    assert st == 0 and outs[-1] == data.size and len(recs) == 3 + 2 + 1 + 1
    assert {r[4] for r in recs} == {2, 0x10}  # compressed chunks and stored ones (the random partition)
    st, back = dk.decode_range(image, recs, outs, fmt=2)
    assert st == 0 and back == data.tobytes()
    twice = image[: int(idx[1])] * 2  # a multi-spill merge: simply more chunks
    st, recs, outs = dsc.discover_snappy(twice, [0, len(twice)], chunk_format=1)
    assert st == 0 and len(recs) == 6 and outs[-1] == 2 * len(parts[0])
    for cut in (1, 3, 4, 6, 17, 100, int(idx[1]) - 1):
        assert dsc.discover_snappy(image[:cut], [0, cut], chunk_format=1)[0] == -3, cut
    for at, v in ((0, ord("X")), (1, ord("W")), (2, 2)):
        bad = bytearray(image)
        bad[at] = v
        assert dsc.discover_snappy(bytes(bad), idx, chunk_format=1)[0] == -3, at


# ---- the compiled checksum kernels under the interpreter ----------------------------------------------------------------------
@pytest.mark.parametrize("algo", [1, 2, 3], ids=["adler32", "crc32", "crc32c"])
def test_compiled_checksum_kernels(algo, oracle):
    """checksum_segments_kernel (256-thread workgroups, four wavefronts that do not talk to each other) + checksum_combine_kernel
    as hipcc compiles them, against zlib: ragged ranges at every alignment, empty ranges, ranges of several 16 KiB segments,
    one-byte ranges — the data buffer ends with its last byte.  And the capacity-overflow rule: offsets that point behind
    `data_len` are not followed (tests/isa/checksum_kernel.py maps exactly data_len bytes)."""
    import zlib

    import checksum_kernel as ck

    f = zlib.adler32 if algo == 1 else zlib.crc32 if algo == 2 else (lambda b: oracle.crc32c(np.frombuffer(b, np.uint8)) if len(b) else 0)
    rng = np.random.default_rng(50 + algo)
    data = rng.integers(0, 256, 120_000, dtype=np.uint8).tobytes()
    cuts = sorted({0, 0, 1, 2, 63, 64, 65, 127, 4096, 16383, 16384, 16385, 16384 * 3 + 7, 70_001, 70_001, 119_999, 120_000})
    offs = [0] + cuts + [120_000]
    assert ck.checksum_ranges(algo, data, offs) == [f(data[a:b]) for a, b in zip(offs, offs[1:])]
    offs = sorted(int(x) for x in rng.integers(0, 120_001, 40)) + [120_000]
    offs = [0] + offs
    assert ck.checksum_ranges(algo, data, offs) == [f(data[a:b]) for a, b in zip(offs, offs[1:])]
    zeros = bytes(40_000)  # Adler32's worst case for the modulus is 0xff bytes, CRC's for leading zeros is zeros
    assert ck.checksum_ranges(algo, zeros, [0, 40_000]) == [f(zeros)]
    ff = b"\xff" * 100_000
    assert ck.checksum_ranges(algo, ff, [0, 100_000]) == [f(ff)]
    # the two-level form of very large ranges (checksum_fold_kernel), with groups of 3 segments instead of the product's 256
    offs = [0, 5, 5, 16384 * 3, 16384 * 7 + 100, 120_000]
    assert ck.checksum_ranges(algo, data, offs, fold_group=3) == [f(data[a:b]) for a, b in zip(offs, offs[1:])]
    assert ck.checksum_ranges(algo, ff, [0, 100_000], fold_group=2) == [f(ff)]
    # offsets computed on the device after a capacity overflow exceed the caller's buffer: those ranges are skipped, not read
    got = ck.checksum_ranges(algo, data[:50_000], [0, 20_000, 50_000, 90_000, 120_000], data_len=50_000)
    assert got[:2] == [f(data[:20_000]), f(data[20_000:50_000])]


# ---- the compiled LZ4Block frame discovery (reduce side) under the interpreter ------------------------------------------------
def _lz4block_stream(oracle, rng, n_chunks, fake_at=()):
    """LZ4Block frames of 32 KiB chunks (compressible ones and random ones that are stored RAW), one end mark; `fake_at` = chunk
    numbers whose RAW payload carries a complete, plausible frame header (what the tile speculation must not believe)"""
    import framing

    out = bytearray()
    for i in range(n_chunks):
        if i % 3 == 0:
            c = corpus.chunk_corpus(7, 32768, rng).tobytes()
        else:
            c = bytearray(rng.integers(0, 256, 32768, dtype=np.uint8).tobytes())
            if i in fake_at:  # a header that passes every field check and whose chain stays inside the range
                for at in (5, 9000, 20000):
                    c[at:at + 21] = b"LZ4Block" + bytes([0x25]) + (700).to_bytes(4, "little") + (900).to_bytes(4, "little") + bytes(4)
            c = bytes(c)
        pay = bytes(oracle.lz4_compress_block(np.frombuffer(c, np.uint8)))
        raw = len(pay) >= len(c)
        out += framing.lz4_frame(c if raw else pay, c, raw=raw)
    out += framing.lz4_end_frame()
    return bytes(out)


def test_compiled_frame_discovery(oracle):
    """tile_speculate -> tile_resolve -> scan -> tile_emit -> scan as hipcc compiles them, every buffer of exactly its size
    (tests/isa/discover_kernel.py): multi-tile streams, concatenated streams, fake headers inside stored payloads right behind
    tile boundaries, and every way a range can end early — the answer is LZ4BlockInputStream.refill()'s, frame by frame, or
    S3S_E_BAD_FRAME, and no access leaves a buffer."""
    import discover_kernel as dsc
    import framing

    rng = np.random.default_rng(47)
    s1 = _lz4block_stream(oracle, rng, 9, fake_at=(1, 2, 4, 5, 7))  # 3.4 tiles; tiles 1..3 start inside chunks 2, 4 / 5, 7
    s2 = _lz4block_stream(oracle, rng, 2)
    for stream in (s1, s1 + s2 + s2, framing.lz4_end_frame(), framing.lz4_end_frame() * 3, s2[:21 + 5] and s2):
        st, recs, outs = dsc.discover(stream)
        want = dsc.reference_frames(stream)
        assert want is not None and st == 0 and recs == want
        assert outs == list(np.concatenate([[0], np.cumsum([r[2] for r in want])]))
    # a range that ends early: inside the last header, inside a payload, one byte short, inside the magic, at tile boundaries
    cuts = [len(s1) - k for k in (1, 2, 8, 20, 21, 22, 30, 42, 43)] + [65536 + d for d in (-1, 0, 1, 8, 20, 21)] + [1, 7, 8, 20]
    for cut in cuts:
        stream = s1[:cut]
        st, recs, _ = dsc.discover(stream)
        want = dsc.reference_frames(stream)
        if want is None:
            assert st == -3, cut
        else:
            assert st == 0 and recs == want, cut
    # "LZ4Block" in the last bytes of the range (a header that cannot be complete) and damaged header fields
    tail = s2 + b"LZ4Block"[: 8]
    assert dsc.discover(tail)[0] == -3
    assert dsc.discover(s2 + b"LZ4Block" + bytes(12))[0] == -3
    for at, val in ((8, 0x35), (8, 0x2F), (9 + 3, 0x7F), (13 + 3, 0x80), (0, 0x4D)):
        m = bytearray(s1)
        m[at] = val
        st, recs, _ = dsc.discover(bytes(m))
        want = dsc.reference_frames(bytes(m))
        assert (st == -3) if want is None else (st == 0 and recs == want), (at, val)
    # random damage: the reference's verdict, never a fault
    for _ in range(25):
        m = bytearray(s1 if rng.integers(0, 2) else s2)
        for _ in range(int(rng.integers(1, 4))):
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256))
        if rng.integers(0, 3) == 0:
            m = m[: int(rng.integers(1, len(m)))]
        st, recs, _ = dsc.discover(bytes(m))
        want = dsc.reference_frames(bytes(m))
        assert (st == -3) if want is None else (st == 0 and recs == want)


# ---- the compiled Zstandard decoder (reduce side, zstd only) under the interpreter -------------------------------------
def test_compiled_zstd_decoder(oracle):
    """zstd_partitions_kernel as hipcc compiles it, both passes of the product (sizes, then decode through the literal
    scratch), on frames written by libzstd the way zstd-jni writes them: TeraSort records and wide rows (Huffman literals,
    FSE sequence tables, repeat offsets), zeros (RLE blocks), random bytes (raw blocks), two partitions in one launch, a
    partition of several concatenated frames, an empty partition.  Source, destination and scratch buffers have exactly
    their sizes: an access outside faults."""
    import zstd_kernel as zk
    from oracle import zstd_ref
    from s3shuffle import datagen

    rng = np.random.default_rng(5)
    tera, _ = datagen.terasort_map_output(1 << 20, 10, seed=3)
    wide, _ = datagen.tpcds_wide_map_output(1 << 20, 10, seed=3)
    pieces = [tera[:9000], wide[:7000], np.zeros(5000, np.uint8), rng.integers(0, 256, 3000).astype(np.uint8),
              tera[20000:20700]]
    parts = [(bytes(zstd_ref.compress_stream(p, level=1)), p.size) for p in pieces]
    # one partition made of three complete frames (a writer that was flushed in pieces), and an empty one
    multi = b"".join(bytes(zstd_ref.compress_stream(p, level=1)) for p in (tera[:1500], wide[:1200], tera[3000:3300]))
    parts.append((multi, 1500 + 1200 + 300))
    parts.append((b"", 0))
    want = [p.tobytes() for p in pieces] + [tera[:1500].tobytes() + wide[:1200].tobytes() + tera[3000:3300].tobytes(), b""]
    out, rcs, _ = zk.decode_partitions(parts)
    assert rcs == [0] * len(parts), rcs
    assert out == want
    # a truncated and a corrupted stream end in "bad frame" (or a size that does not match), never outside the buffers
    good = parts[0][0]
    for bad in (good[:len(good) // 2], good[:40] + bytes([good[40] ^ 0x5A]) + good[41:]):
        out, rcs, _ = zk.decode_partitions([(bad, parts[0][1])])
        assert out[0] is None or out[0] == want[0]


def test_compiled_zstd_content_checksum(oracle):
    """Round 4: frames written with a content checksum end with XXH64's low 32 bits; the compiled decoder hashes what it
    decoded - an out-of-line device function (hipcc: s_getpc_b64 + rel32 + s_swappc_b64; the interpreter appends the callee's
    instructions, Program.callees) whose four accumulators run on lanes 0..3 - and refuses a frame whose content was damaged
    where it still decodes (a byte of a stored block), as libzstd does."""
    import zstd_kernel as zk
    from oracle import zstd_ref
    from s3shuffle import datagen

    rng = np.random.default_rng(4)
    tera, _ = datagen.terasort_map_output(1 << 20, 2, seed=3)
    cases = [tera[:5000], rng.integers(0, 256, 3000, dtype=np.uint8), tera[:37], np.zeros(0, np.uint8), tera[:20], tera[:64]]
    parts = [(bytes(zstd_ref.compress_stream(d, level=1, checksum=True)), d.size) for d in cases]
    out, rcs, _ = zk.decode_partitions(parts)
    assert rcs == [0] * len(cases) and out == [d.tobytes() for d in cases]
    bad = bytearray(parts[1][0])
    bad[len(bad) // 2] ^= 0x40
    assert zstd_ref.decompress(np.frombuffer(bytes(bad), np.uint8), 4096) is None
    out, rcs, _ = zk.decode_partitions([(bytes(bad), 3000), parts[0]])
    assert rcs[0] == -3 and out[0] is None and out[1] == cases[0].tobytes()


def test_compiled_zstd_literal_wavefront_over_several_blocks(oracle):
    """Round 4: a workgroup of zstd_partitions_kernel is two sequence wavefronts and one literal wavefront that regenerates the
    Huffman literals of each partition's NEXT block (LitPipe counters in LDS, two literal buffers per partition).  The
    interpreter runs the three wavefronts as co-operating threads (gfx950_emu._WaveGroup: the baton moves at s_barrier, at
    s_sleep and when a wavefront ends).  A partition of six Huffman-coded blocks beside one of four: the literal side runs
    ahead, waits for a buffer to be given back, and serves both partitions; then the same pair with a damaged Huffman stream in
    the SECOND block of one partition - that partition is refused (or decodes to something of another size), its neighbour
    still decodes, and nobody waits forever."""
    import zstd_kernel as zk
    from oracle import zstd_ref
    from s3shuffle import datagen

    tera, _ = datagen.terasort_map_output(1 << 20, 2, seed=31)
    wide, _ = datagen.tpcds_wide_map_output(1 << 20, 2, seed=32)
    # (window_log 12: libzstd cuts 4 KiB blocks, so a few dozen KB are many blocks and the interpreter stays quick)
    a, b = tera[:22_000], wide[:13_000]
    ca, cb = bytes(zstd_ref.compress_stream(a, level=1, window_log=12)), bytes(zstd_ref.compress_stream(b, level=1, window_log=12))
    out, rcs, waves = zk.decode_partitions([(ca, a.size), (cb, b.size)])
    assert rcs == [0, 0] and out[0] == a.tobytes() and out[1] == b.tobytes()
    def blocks(c):  # (offset of the block content, size, literals type) of a single frame without dictionary id
        fhd = c[4]
        pos = 5 + (0 if fhd & 0x20 else 1) + [0, 1, 2, 4][fhd & 3] + ([1, 2, 4, 8][fhd >> 6] if (fhd >> 6) or (fhd & 0x20) else 0)
        found = []
        while True:
            bh = int.from_bytes(c[pos:pos + 3], "little")
            size = 1 if (bh >> 1) & 3 == 1 else bh >> 3
            found.append((pos + 3, size, c[pos + 3] & 3 if (bh >> 1) & 3 == 2 else -1))
            pos += 3 + size
            if bh & 1:
                return found

    ba, bb = blocks(ca), blocks(cb)
    assert sum(1 for _, _, t in ba if t >= 2) >= 4 and sum(1 for _, _, t in bb if t >= 2) >= 3  # Huffman-coded literals
    second = [o for o, _, t in ba if t >= 2][1] - 3
    hit = second + 3 + 40  # inside its literals section (table or first stream)
    bad = ca[:hit] + bytes([ca[hit] ^ 0x77]) + ca[hit + 1:]
    out, rcs, _ = zk.decode_partitions([(bad, a.size), (cb, b.size)])
    assert out[1] == b.tobytes() and rcs[1] == 0
    assert out[0] is None or out[0] == a.tobytes()
