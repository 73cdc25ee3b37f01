"""LZ4 blocks above 64 KiB on the map side, run on the CPU: the COMPILED kernels (lz4_compress_u32_kernel - the byU32 parse of
chunks of 65 547 bytes and more -, today's lz4_compress_l2_kernel on the lengths 65 537 .. 65 546 it had never been handed, and a
whole map-side call at block size 131 072) through the interpreter of tests/isa/gfx950_emu.py, compared with liblz4 itself
(tests/lz4_u32_ref.py).  Every source buffer ends with its chunk: a read past the end faults."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "spark-s3-shuffle_amd"))
import corpus  # noqa: E402
import lz4_u32_ref as R  # noqa: E402
from test_lz4_u32_ref import inputs  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None,
                                reason="hipcc not available")

CHECK0 = 3 * 0x01010101  # the frame check compress_chunks_u32 hands the first item


def _kernel(d):
    """one chunk through the compiled byU32 kernel, in a source buffer of exactly its size -> (payload or None, frame header)"""
    import lz4_big_blocks as bb

    (payload, header, _), = bb.compress_chunks_u32([d])
    return payload, header


def _kernel_all(chunks):
    """the interpreter runs one wavefront at a time (8 - 60 s per chunk here): the chunks are dealt out to a few forked workers"""
    import multiprocessing

    import lz4_big_blocks as bb

    bb._prog("lz4_compress.hip", "lz4_compress_u32_kernel")  # compiled and parsed once, inherited by the workers
    with multiprocessing.get_context("fork").Pool(max(1, min(4, os.cpu_count() or 1))) as pool:
        return pool.map(_kernel, chunks, chunksize=1)


def test_u32_kernel_matches_liblz4():
    """chunks of 65 547, 65 548, 70 000 and 131 072 bytes of TeraSort, wide rows, chunk_corpus, zeros and random, the far-motif
    input and both boundary inputs: payload and frame header equal to liblz4's"""
    import lz4_big_blocks as bb

    b0, b1 = R.boundary_pair()
    cases = inputs(lengths=(65_547, 65_548, 70_000, 131_072)) + [("boundary_65535", b0), ("boundary_65536", b1),
                                                                ("long_literals", R.long_literals(np.random.default_rng(8)))]
    seen = {"raw": 0, "compressed": 0, "refusals": 0}
    results = _kernel_all([d for _, d in cases])
    for (name, d), (payload, header) in zip(cases, results):
        want = R.liblz4_block(d)
        _, refused = R.compress_u32(d.tobytes())
        is_raw = len(want) >= d.size
        assert header == bb.expected_header(d, want, d.size, CHECK0), (name, d.size)
        if is_raw:
            assert payload is None, (name, d.size)
        else:
            assert payload == want, (name, d.size, _first_diff(payload, want))
        seen["raw"] += is_raw
        seen["compressed"] += not is_raw
        seen["refusals"] += refused > 0
        # what the hand-built inputs are, asserted from liblz4's own stream before the kernel is compared with it (above)
        if name == "boundary_65535":
            assert max(R.block_offsets(want)) == 65_535 and refused == 0
        if name == "boundary_65536":
            assert max(R.block_offsets(want)) < 65_535 and refused >= 1
        if name == "far_motif":
            assert d.size == 146_500 and refused >= 100
        if name == "long_literals":  # a literal run above 64 KiB in front of a match
            k = 1
            while want[k] == 255:
                k += 1
            assert not is_raw and want[0] >> 4 == 15 and 15 + 255 * (k - 1) + want[k] > 100_000
    assert seen["raw"] >= 1 and seen["compressed"] >= 1 and seen["refusals"] >= 4, seen


def _first_diff(a, b):
    n = min(len(a), len(b))
    return next((i for i in range(n) if a[i] != b[i]), n), len(a), len(b)


def test_u32_kernel_keeps_its_wait_states():
    import hazards
    import lz4_kernel as lk

    text = lk.compile_asm()
    entry = lk.find_kernel(text, "lz4_compress_u32_kernel")
    asm_viol, cc_viol, _, _ = hazards.check_kernel(text, entry)
    assert not asm_viol, asm_viol
    assert not cc_viol, ("rule set stricter than the compiler", cc_viol[:3])


def test_u16_kernel_on_chunks_of_65537_to_65546_bytes():
    """liblz4 parses inputs below 65 547 bytes with its 16-bit table whatever the block size: a tail of 65 537 .. 65 546 bytes goes
    through today's kernel (window block included), which no block size could hand such a chunk before"""
    import lz4_kernel as lk
    from s3shuffle import datagen

    rng = np.random.default_rng(11)
    tera = datagen.terasort_map_output(1 << 18, 1, seed=3)[0]
    wide = datagen.tpcds_wide_map_output(1 << 18, 1, seed=4)[0]
    for n in range(65_537, 65_547):
        d = np.ascontiguousarray([tera[:n], wide[:n], corpus.chunk_corpus(7, n, rng)][n % 3])
        want = R.liblz4_block(d)
        assert len(want) < n
        for windows in ((True, False) if n in (65_537, 65_546) else (True,)):
            (payload, header, _), = lk.compress_chunks([d], windows=windows, block=65_546)
            assert payload is not None and bytes(payload) == want, (n, windows)
            assert header[8] == 0x25 and int.from_bytes(header[9:13], "little") == len(want) and int.from_bytes(header[13:17], "little") == n
    # a chunk that ends in a long match (matchlimit, last literals) and a stored one, at the largest byU16 length
    z = np.zeros(65_546, np.uint8)
    (payload, _, _), = lk.compress_chunks([z], block=65_546)
    assert bytes(payload) == R.liblz4_block(z)
    r = rng.integers(0, 256, 65_546, dtype=np.uint8)
    (payload, header, _), = lk.compress_chunks([r], block=65_546)
    assert payload is None and header[8] == 0x15


def test_map_side_image_at_block_size_131072():
    """full blocks, tails of 65 546 (byU16) and 65 547 bytes (byU32), a 100-byte tail, an empty partition, a stored chunk, both
    boundary inputs as whole chunks and the far-motif input's first block (the input itself is 146 500 bytes, more than a block:
    its first 131 072 bytes hold the motif's second copy 73 000 bytes behind the first, so the block has candidates that are
    refused although their bytes match - asserted from the model): image, index and checksums of the compiled kernels equal the
    liblz4-built streams; the destination has exactly the image's size"""
    import lz4_big_blocks as bb
    from s3shuffle import datagen

    bs = 131_072
    rng = np.random.default_rng(12)
    tera = datagen.terasort_map_output(1 << 18, 1, seed=3)[0]
    wide = datagen.tpcds_wide_map_output(1 << 18, 1, seed=4)[0]
    far = R.far_motif(rng)
    b0, b1 = R.boundary_pair()
    parts = [np.ascontiguousarray(tera[:bs + 65_546]), np.zeros(0, np.uint8), np.ascontiguousarray(wide[:bs + 65_547]),
             np.concatenate([far[:bs], corpus.chunk_corpus(7, 100, rng)]), rng.integers(0, 256, 66_000, dtype=np.uint8), b0, b1]
    img, index, sums = R.expected_map_output(parts, bs, 3)
    toks = [t for p in parts for t in R.frame_tokens(R.jvm_stream(p, bs))]
    assert sorted(t[2] for t in toks if t[2]) == [100, 65_546, 65_547, 66_000, 68_599, 68_600, bs, bs, bs]
    assert any(t[0] == 0x17 and t[2] for t in toks) and any(t[0] == 0x27 for t in toks)  # stored and compressed, level 7
    assert R.compress_u32(parts[0][:bs].tobytes())[1] >= 1
    st = {}
    payload, refused = R.compress_u32(far[:bs].tobytes(), stats=st)
    assert payload == R.liblz4_block(far[:bs]) and refused >= 100 and st["refused_equal"] >= 1
    assert max(R.block_offsets(R.liblz4_block(b0))) == 65_535 and R.compress_u32(b0.tobytes())[1] == 0
    assert max(R.block_offsets(R.liblz4_block(b1))) < 65_535 and R.compress_u32(b1.tobytes())[1] >= 1
    status, got, gidx, gsums = bb.compress_map_output([p.tobytes() for p in parts], 3, len(img), bs)
    assert status == 0
    assert gidx == index
    assert got == img
    assert gsums == sums
    # one byte less: S3S_E_CAPACITY, nothing written past the destination (the interpreter would fault)
    status, _, _, _ = bb.compress_map_output([p.tobytes() for p in parts[4:5]], 0, len(R.jvm_stream(parts[4], bs)) - 1, bs)
    assert status == -2
