"""GPU: LZ4 block sizes above 64 KiB on the map side (spark.io.compression.lz4.blockSize 65 537 .. 32m through
S3S_OPT_LZ4_BLOCK_SIZE_LARGE, ABI 10).  Chunks of 65 547 bytes and more are liblz4's byU32 parse (4096 x u32 table, 5-byte hash,
distance test), shorter ones - a partition's tail, whatever the block size - its byU16 parse.

Expected bytes come from liblz4 itself through ctypes (tests/lz4_u32_ref.py: jvm_stream), checksums from zlib (CRC32C: a table
loop), the index from the stream lengths: neither the oracle (byU16 only) nor the product.  What the inputs exercise is asserted
from the Python restatement of the parse (refusals of the distance test) and from the frame tokens (stored RAW / compressed)."""
import time
import zlib

import numpy as np
import pytest

import corpus
import lz4_u32_ref as R
from hipdev import Dev

pytestmark = pytest.mark.gpu

LZ4 = 1
OPT_LZ4_BLOCK_SIZE, OPT_LZ4_VARIANT, OPT_LZ4_BLOCK_SIZE_LARGE = 1, 4, 8
ADLER, CRC, CRC32C = 1, 2, 3
FAR_LEN = 146_500


class _BlockSize:
    """the context's LZ4 block size for the duration of a with-block (the default comes back through key 1)"""

    def __init__(self, codec, bs):
        self.codec, self.bs = codec, bs

    def __enter__(self):
        self.old = self.codec.get_option(OPT_LZ4_BLOCK_SIZE)
        self.codec.set_option(OPT_LZ4_BLOCK_SIZE_LARGE, self.bs)
        return self

    def __exit__(self, *exc):
        self.codec.set_option(OPT_LZ4_BLOCK_SIZE_LARGE, self.old)


def _parts(bs, seed):
    """named partitions: ragged sizes, TeraSort, wide rows, incompressible, empty, exactly one block, one block + 1 byte, tails of
    65 546 and 65 547 bytes (where the block size leaves room for them), the far-motif input and both boundary inputs"""
    from s3shuffle import datagen

    rng = np.random.default_rng(seed)
    b0, b1 = R.boundary_pair()
    parts = [("terasort", datagen.terasort_map_output(3 * bs + 12_345, 1, seed=3)[0]),
             ("empty", np.zeros(0, np.uint8)),
             ("random", rng.integers(0, 256, bs + 77, dtype=np.uint8)),
             ("wide", datagen.tpcds_wide_map_output(2 * bs + 999 + 4096, 1, seed=4)[0][:2 * bs + 999]),
             ("one_block", corpus.chunk_corpus(7, bs, rng)),
             ("one_block_plus_1", corpus.chunk_corpus(7, bs + 1, rng)),
             ("far_motif", R.far_motif(rng)),
             ("boundary_65535", b0),
             ("boundary_65536", b1),
             ("long_literals", R.long_literals(rng)),
             ("tiny", corpus.chunk_corpus(3, 100, rng))]
    if bs > 65_547:
        parts += [("tail_65546", corpus.chunk_corpus(7, bs + 65_546, rng)), ("tail_65547", corpus.chunk_corpus(7, bs + 65_547, rng))]
    for k in range(4):  # ragged
        parts.append(("ragged%d" % k, corpus.chunk_corpus(int(rng.integers(0, corpus.N_KINDS - 2)) if k else 7, int(rng.integers(1, 3 * bs)), rng)))
    return [(n, np.ascontiguousarray(p, dtype=np.uint8)) for n, p in parts]


def _concat(parts):
    data = np.concatenate([p for _, p in parts]) if parts else np.zeros(0, np.uint8)
    offs = np.concatenate([[0], np.cumsum([p.size for _, p in parts])]).astype(np.int64)
    return data, offs


def _expect(parts, bs, algo):
    img, index, sums = R.expected_map_output([p for _, p in parts], bs, algo)
    return np.frombuffer(img, np.uint8), np.array(index, np.int64), np.array(sums, np.int64)


def _special(rng):
    """the partitions every byte-compare set of this file carries: the far-motif input, both boundary inputs, an incompressible
    partition (stored RAW) and a tiny one (a byU16 chunk at any block size)"""
    b0, b1 = R.boundary_pair()
    return [("far_motif", R.far_motif(rng)), ("boundary_65535", b0), ("boundary_65536", b1),
            ("random_70000", rng.integers(0, 256, 70_000, dtype=np.uint8)), ("tiny", corpus.chunk_corpus(3, 100, rng))]


def _check_inputs(parts, bs):
    """What a byte-compare set exercises, asserted from liblz4's own frames (stored RAW / compressed, level) and from the model
    (refusals of the distance test) before the product is compared with anything.  Called for EVERY set of this file:
      * one chunk stored RAW, one compressed, one below 65 547 bytes (the 16-bit-table kernel);
      * block sizes below 65 547 have no byU32 chunk at all - the set is then asserted to be byU16 only, at lengths that kernel
        was never handed before (the distance test does not exist in that parse);
      * the far-motif input's first block (the whole 146 500-byte input from that block size on, else its first bs bytes, which
        hold the motif's second copy 73 000 bytes behind the first from 76 004 bytes on): candidates REFUSED although their four
        bytes match, and no offset above 65 535 in liblz4's stream;
      * both boundary inputs as single chunks (68 599 / 68 600 bytes) from block size 68 600 on: liblz4's stream holds a match of
        offset 65 535 in the first and none in the second, which has refusals instead;
      * the first TeraSort block, where there is one of at most 1 MiB (the model is Python): >= 1 refusal."""
    by = dict(parts)
    toks = [t for _, p in parts for t in R.frame_tokens(R.jvm_stream(p, bs))]
    data_frames = [t for t in toks if t[2] > 0]
    assert any(t[0] & 0xF0 == 0x10 for t in data_frames), "no chunk stored RAW"
    assert any(t[0] & 0xF0 == 0x20 for t in data_frames), "no chunk compressed"
    assert all(t[0] & 0x0F == R.level(bs) for t in toks)
    u32_chunks = [t for t in data_frames if t[2] >= R.U32_FROM]
    assert any(t[2] < R.U32_FROM for t in data_frames), "no chunk for the 16-bit-table kernel"
    if bs < R.U32_FROM:
        assert not u32_chunks
        return
    assert u32_chunks
    fm = np.ascontiguousarray(by["far_motif"][:bs])
    assert by["far_motif"].size == FAR_LEN and fm.size >= R.U32_FROM
    st = {}
    payload, refused = R.compress_u32(fm.tobytes(), stats=st)
    want = R.liblz4_block(fm)
    assert payload == want and max(R.block_offsets(want)) <= 65_535
    if bs >= 76_004:
        assert refused >= 100 and st["refused_equal"] >= 1, "no candidate with matching bytes refused by the distance test"
    if bs >= 68_600:
        b0, b1 = by["boundary_65535"], by["boundary_65536"]
        assert (b0.size, b1.size) == (68_599, 68_600)
        assert max(R.block_offsets(R.liblz4_block(b0))) == 65_535 and max(R.block_offsets(R.liblz4_block(b1))) < 65_535
        assert R.compress_u32(b0.tobytes())[1] == 0 and R.compress_u32(b1.tobytes())[1] >= 1
    first = by["terasort"][:bs] if "terasort" in by else None
    if first is not None and R.U32_FROM <= first.size <= 1 << 20:
        payload, refused = R.compress_u32(first.tobytes())
        assert payload == R.liblz4_block(first) and refused >= 1, "no candidate refused by the distance test"


@pytest.mark.parametrize("bs", [65_537, 100_000, 131_072, 262_144, 1 << 20])
def test_map_side_matches_liblz4(gpu_codec, bs):
    parts = _parts(bs, bs % 1000)
    _check_inputs(parts, bs)
    if bs == 131_072:  # the figure of the issue: this TeraSort block is the one it counted
        assert R.compress_u32(dict(parts)["terasort"][:bs].tobytes())[1] == 840
    data, offs = _concat(parts)
    with _BlockSize(gpu_codec, bs):
        assert gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE_LARGE) == bs and gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE) == bs
        for algo in (ADLER, CRC, CRC32C):
            img, index, sums = gpu_codec.compress_map_output(LZ4, algo, data, offs)
            r_img, r_index, r_sums = _expect(parts, bs, algo)
            assert np.array_equal(index, r_index), algo
            assert np.array_equal(img, r_img), (algo, _first_diff(img, r_img, r_index, parts))
            assert np.array_equal(sums, r_sums), algo
        back = gpu_codec.decompress_range(LZ4, CRC32C, img, index, sums)
        assert np.array_equal(back, data)


def _first_diff(img, want, index, parts):
    n = min(img.size, want.size)
    d = np.nonzero(img[:n] != want[:n])[0]
    if d.size == 0:
        return ("sizes", img.size, want.size)
    p = int(np.searchsorted(index, d[0], side="right") - 1)
    return ("partition", parts[p][0], "image byte", int(d[0]), "byte of the partition's stream", int(d[0] - index[p]))


def test_32_mib_blocks_and_option_bounds(gpu_codec):
    from s3shuffle import datagen

    lib, h = gpu_codec._lib, gpu_codec._h
    old = gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE)
    try:
        assert lib.s3s_set_option(h, OPT_LZ4_BLOCK_SIZE_LARGE, 64) == 0
        assert gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE) == 64 and gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE_LARGE) == 64
        assert lib.s3s_set_option(h, OPT_LZ4_BLOCK_SIZE_LARGE, 63) == -1
        assert lib.s3s_set_option(h, OPT_LZ4_BLOCK_SIZE_LARGE, (1 << 25) + 1) == -6
        assert gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE_LARGE) == 64  # (refused values leave the option alone)
        assert lib.s3s_set_option(h, OPT_LZ4_BLOCK_SIZE_LARGE, 1 << 25) == 0
        assert gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE) == 1 << 25 and gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE_LARGE) == 1 << 25
        assert lib.s3s_set_option(h, OPT_LZ4_BLOCK_SIZE, 65_537) == -6  # key 1 keeps its range and its answer
        assert gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE) == 1 << 25
        assert lib.s3s_set_option(h, OPT_LZ4_BLOCK_SIZE, 65_536) == 0 and gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE_LARGE) == 65_536
        # one full 32 MiB block + a short tail; the far-motif, boundary, stored and tiny partitions as whole chunks
        bs = 1 << 25
        rng = np.random.default_rng(32)
        parts = [("terasort", np.ascontiguousarray(datagen.terasort_map_output(bs + 2000, 1, seed=6)[0][:bs + 1000]))] + _special(rng)
        parts = [(n, np.ascontiguousarray(p, dtype=np.uint8)) for n, p in parts]
        _check_inputs(parts, bs)
        data, offs = _concat(parts)
        gpu_codec.set_option(OPT_LZ4_BLOCK_SIZE_LARGE, bs)
        img, index, sums = gpu_codec.compress_map_output(LZ4, ADLER, data, offs)
        r_img, r_index, r_sums = _expect(parts, bs, ADLER)
        assert [t[2] for t in R.frame_tokens(r_img[:r_index[1]].tobytes())] == [bs, 1000, 0]
        assert np.array_equal(index, r_index) and np.array_equal(sums, r_sums)
        assert np.array_equal(img, r_img), _first_diff(img, r_img, r_index, parts)
        assert np.array_equal(gpu_codec.decompress_range(LZ4, ADLER, img, index, sums), data)
    finally:
        gpu_codec.set_option(OPT_LZ4_BLOCK_SIZE, old)


def test_every_entry_point_at_128k(gpu_codec):
    import s3shuffle

    bs = 131_072
    parts = _parts(bs, 7)
    _check_inputs(parts, bs)
    data, offs = _concat(parts)
    r_img, r_index, r_sums = _expect(parts, bs, CRC)
    dev = Dev()
    old_variant = gpu_codec.get_option(OPT_LZ4_VARIANT)
    try:
        with _BlockSize(gpu_codec, bs):
            cap = gpu_codec.max_compressed_size(LZ4, offs)
            assert cap >= r_img.size
            for variant in (1, 10, 9):  # identical output (chunks of 65 547 bytes and more take the general batch whatever this says)
                gpu_codec.set_option(OPT_LZ4_VARIANT, variant)
                img, index, sums = gpu_codec.compress_map_output(LZ4, CRC, data, offs)
                assert np.array_equal(index, r_index) and np.array_equal(sums, r_sums) and np.array_equal(img, r_img), variant
            gpu_codec.set_option(OPT_LZ4_VARIANT, old_variant)
            # device form, batched device form, batched host form
            d_src, d_dst = dev.upload(data), dev.alloc(cap)
            total, index, sums = gpu_codec.compress_map_output_device(LZ4, CRC, d_src, offs, d_dst, cap)
            assert total == r_img.size and np.array_equal(index, r_index) and np.array_equal(sums, r_sums)
            assert np.array_equal(dev.download(d_dst, total), r_img)
            halves = [parts[:6], parts[6:]]  # (one batched call over two tasks: together the whole set)
            tasks, host_tasks, host_dst, want = [], [], [], []
            for hp in halves:
                hd, ho = _concat(hp)
                hc = gpu_codec.max_compressed_size(LZ4, ho)
                tasks.append((dev.upload(hd), ho, dev.alloc(hc), hc))
                out = np.zeros(hc, np.uint8)
                host_dst.append((hd, out))
                host_tasks.append((hd.ctypes.data, ho, out.ctypes.data, hc))
                want.append(_expect(hp, bs, CRC))
            res = gpu_codec.compress_map_outputs_batch_device(LZ4, CRC, tasks)
            hres = gpu_codec.compress_map_outputs_batch(LZ4, CRC, host_tasks)
            for (w_img, w_index, w_sums), (total, bi, bsums), (_, _, d_out, _), (htotal, hi, hsums), (_, hout) in zip(
                    want, res, tasks, hres, host_dst):
                assert total == w_img.size and np.array_equal(bi, w_index) and np.array_equal(bsums, w_sums)
                assert np.array_equal(dev.download(d_out, total), w_img)
                assert htotal == w_img.size and np.array_equal(hi, w_index) and np.array_equal(hsums, w_sums)
                assert np.array_equal(hout[:htotal], w_img)
            # segments: partition p is made of pieces (spills), every non-empty piece a complete stream
            # (the first six partitions in three pieces, the others - far-motif, boundary inputs ... - in one: the whole set again)
            pieces, pfs = [], [0]
            for k, (_, p) in enumerate(parts):
                cuts = [0, p.size // 3, p.size // 3, p.size] if k < 6 else [0, p.size]  # (an empty piece in the middle)
                pieces += [p[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
                pfs.append(len(pieces))
            seg_offs = np.concatenate([[0], np.cumsum([x.size for x in pieces])]).astype(np.int64)
            sdata = np.concatenate(pieces)
            img, index, sums = gpu_codec.compress_map_output_segments(LZ4, ADLER, sdata, seg_offs, np.array(pfs, np.int32))
            streams = [b"".join(R.jvm_stream(x, bs) for x in pieces[a:b]) for a, b in zip(pfs[:-1], pfs[1:])]
            assert img.tobytes() == b"".join(streams)
            assert [int(x) for x in np.diff(index)] == [len(s) for s in streams]
            assert [int(x) for x in sums] == [zlib.adler32(s) for s in streams]
            # a destination that is too small
            with pytest.raises(s3shuffle.CodecError) as e:
                gpu_codec.compress_map_output(LZ4, CRC, data, offs, dst_capacity=r_img.size - 1)
            assert e.value.code == s3shuffle.codec.E_CAPACITY
            img, index, sums = gpu_codec.compress_map_output(LZ4, CRC, data, offs, dst_capacity=r_img.size)
            assert np.array_equal(img, r_img)
    finally:
        gpu_codec.set_option(OPT_LZ4_VARIANT, old_variant)
        dev.free()


def test_host_mirror_round_trip_at_128k(gpu_codec, oracle, tmp_path):
    from s3shuffle import datagen, host

    root = "file://" + str(tmp_path / "spark-s3-shuffle")
    d = host.Dispatcher(root, codec="lz4", block_size=131072, num_gpus=1)
    try:
        tera = datagen.terasort_map_output(1 << 20, 1, seed=8)[0]
        parts = [("terasort", tera[:700_000])] + _special(np.random.default_rng(8)) + [("terasort_tail", tera[700_000:900_000])]
        parts = [(n, np.ascontiguousarray(p, dtype=np.uint8)) for n, p in parts]
        _check_inputs(parts, 131072)
        data, offs = _concat(parts)
        spill = tmp_path / "spill_0.tmp"
        spill.write_bytes(data.tobytes())
        lengths = host.transfer_map_spill_file(d, 0, 4, str(spill), np.diff(offs))
        img, index, sums = _expect(parts, 131072, ADLER)
        assert np.array_equal(lengths, np.diff(index))
        assert open(d.get_path(host.KIND_DATA, 0, 4), "rb").read() == img.tobytes()
        assert open(d.get_path(host.KIND_INDEX, 0, 4), "rb").read() == oracle.longs_to_be(index)
        assert open(d.get_path(host.KIND_CHECKSUM, 0, 4), "rb").read() == oracle.longs_to_be(sums)
        got = host.read_shuffle(d, 0, 0, len(parts), True)
        assert len(got) == 1 and np.array_equal(got[0][4], data)
        d.remove_root()
    finally:
        d.close()


def test_short_fuzz_at_random_block_sizes(gpu_codec):
    """a few seconds of the adversarial chunk generators (tests/tools/isa_fuzz.py) at random block sizes in 65 537 .. 1 MiB,
    partition lengths around the block size and around LZ4_64Klimit, against liblz4-built streams.  Every round also carries
    the far-motif, boundary, stored and tiny partitions, and what the round exercises is asserted like every other set's; the first
    round's block size is fixed so that those inputs are whole chunks at least once"""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import isa_fuzz as F

    rng = np.random.default_rng(20261)
    old = gpu_codec.get_option(OPT_LZ4_BLOCK_SIZE)
    t0, rounds, u32_chunks = time.time(), 0, 0
    try:
        while time.time() - t0 < 12.0 or rounds < 3:
            bs = 262_144 if rounds == 0 else int(rng.integers(65_537, (1 << 20) + 1))
            gpu_codec.set_option(OPT_LZ4_BLOCK_SIZE_LARGE, bs)
            parts = [(n, np.ascontiguousarray(p, dtype=np.uint8)) for n, p in _special(rng)]
            u32_chunks += sum(1 for _, p in parts for q in range(0, p.size, bs) if min(bs, p.size - q) >= R.U32_FROM)
            for k in range(8):
                r = rng.random()
                n = (int(rng.integers(65_530, 65_560)) if r < 0.25 else bs + int(rng.integers(-3, 20)) if r < 0.45
                     else int(rng.integers(1, 2 * bs + 70_000)))
                gen = F.GENS[int(rng.integers(0, len(F.GENS)))]
                p = np.concatenate([gen(rng, min(n - q, 98_304)) for q in range(0, n, 98_304)])[:n]
                for _ in range(int(rng.integers(0, 4))):  # copies planted around the distance limit
                    ln, dist = int(rng.integers(4, 400)), int(rng.integers(65_400, 65_700))
                    if n > dist + ln + 16:
                        at = int(rng.integers(0, n - dist - ln))
                        p[at + dist:at + dist + ln] = p[at:at + ln]
                parts.append(("g%d" % k, np.ascontiguousarray(p, dtype=np.uint8)))
                u32_chunks += sum(1 for q in range(0, n, bs) if min(bs, n - q) >= R.U32_FROM)
            _check_inputs(parts, bs)
            data, offs = _concat(parts)
            algo = int(rng.integers(1, 3))
            img, index, sums = gpu_codec.compress_map_output(LZ4, algo, data, offs)
            r_img, r_index, r_sums = _expect(parts, bs, algo)
            assert np.array_equal(index, r_index), (rounds, bs)
            assert np.array_equal(img, r_img), (rounds, bs, _first_diff(img, r_img, r_index, parts))
            assert np.array_equal(sums, r_sums), (rounds, bs)
            rounds += 1
        assert u32_chunks > 10
    finally:
        gpu_codec.set_option(OPT_LZ4_BLOCK_SIZE, old)
