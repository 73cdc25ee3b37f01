"""The batched map-side call (s3s_compress_map_outputs_batch_device) with its small arrays packed into ONE arena: one upload
(block counter and status words travel as zeros with it), one download, no memset (PackedPlan, csrc/stream_placement.h).
Outputs, statuses and error behaviour are what they were: every case is bit-exact against the CPU oracle, or round-tripped
through the decoder where the oracle has no writer (Zstandard, LZF)."""
import numpy as np
import pytest

import corpus
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC = 1, 2
BLOCK = 32768


def _map_output(sizes, seed):
    """partitions of the given sizes, kinds of tests/corpus.py in turn"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, n in enumerate(sizes):
        kind = (seed + i) % corpus.N_KINDS
        parts.append(corpus.chunk_corpus(7 if kind == 6 and n > 5000 else kind, n, rng))  # (kind 6 is a Python loop per byte)
    offs = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=offs[1:])
    data = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return data, offs


_SHAPES = {}


def shape(name):
    """the map tasks of a named call, built once: [(data, offsets)]"""
    if name not in _SHAPES:
        if name == "edges":  # no partitions at all | one empty partition | five partitions around the block size
            _SHAPES[name] = [_map_output([], 1), _map_output([0], 2), _map_output([BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1], 3)]
        elif name == "tiny2000":  # an odd number of index entries (2 001): the regions behind it need their alignment
            _SHAPES[name] = [_map_output([7] * 2000, 4)]
        elif name == "three":
            _SHAPES[name] = [_map_output([50_000, 0, 9], 5), _map_output([BLOCK + 1, 40_000, 1], 6), _map_output([3, 70_000], 7)]
        elif name == "large":
            _SHAPES[name] = [_map_output([200_000] * 8, 8)]
        elif name == "small":
            _SHAPES[name] = [_map_output([10], 9)]
    return _SHAPES[name]


_REF = {}


def reference(oracle, name, codec, algo):
    """the oracle's (image, index, checksums) of every task of a named call, computed once"""
    key = (name, codec, algo)
    if key not in _REF:
        _REF[key] = [oracle.compress_map_output(codec, algo, d, o) for d, o in shape(name)]
    return _REF[key]


def run_batch(codec_ctx, dev, codec, algo, host_tasks, caps=None):
    """-> (rc, [(status, total, index, sums, image or None)]) through the C entry point, per-task status included"""
    from s3shuffle.codec import MapTask, _i64, _p64

    arr = (MapTask * len(host_tasks))()
    keep = []
    for i, (data, offs) in enumerate(host_tasks):
        offs = _i64(offs)
        n = len(offs) - 1
        cap = codec_ctx.max_compressed_size(codec, offs) if caps is None or caps[i] is None else caps[i]
        index, sums = np.full(n + 1, -1, np.int64), np.full(max(n, 1), -1, np.int64)
        d_dst = dev.alloc(cap)
        keep.append((offs, index, sums, n, d_dst))
        arr[i].d_src = dev.upload(data)
        arr[i].src_offsets = _p64(offs)
        arr[i].num_partitions = n
        arr[i].d_dst = d_dst
        arr[i].dst_capacity = int(cap)
        arr[i].out_index = _p64(index)
        arr[i].out_checksums = _p64(sums) if algo else None
        arr[i].status = 12345
    rc = codec_ctx._lib.s3s_compress_map_outputs_batch_device(codec_ctx._h, codec, algo, arr, len(host_tasks))
    out = []
    for i, (offs, index, sums, n, d_dst) in enumerate(keep):
        st, total = int(arr[i].status), int(arr[i].out_total)
        out.append((st, total, index, sums[:n], dev.download(d_dst, total) if st == 0 else None))
    return rc, out


def assert_equals_oracle(got, ref, algo):
    for t, ((st, total, index, sums, img), (r_img, r_index, r_sums)) in enumerate(zip(got, ref)):
        assert st == 0, (t, st)
        assert np.array_equal(index, r_index), t
        assert total == r_img.size
        if algo:
            assert np.array_equal(sums, r_sums), t
        assert np.array_equal(img, r_img), t


@pytest.mark.parametrize("algo", [NONE, ADLER, CRC])
@pytest.mark.parametrize("codec", [LZ4, SNAPPY])
@pytest.mark.parametrize("name", ["edges", "tiny2000"])
def test_packed_call_equals_oracle(gpu_codec, oracle, name, codec, algo):
    dev = Dev()
    try:
        rc, got = run_batch(gpu_codec, dev, codec, algo, shape(name))
        assert rc == 0
        assert_equals_oracle(got, reference(oracle, name, codec, algo), algo)
    finally:
        dev.free()


@pytest.mark.parametrize("codec,option", [(ZSTD, 9), (LZF, 10)])
def test_packed_call_round_trips_opt_in_codecs(codec, option):
    """Zstandard and LZF on the map side are decode-compatible writers, not the reference's bytes: the decoder is the check"""
    import s3shuffle

    dev = Dev()
    try:
        with s3shuffle.Codec(0) as c:
            c.set_option(option, 1)
            rc, got = run_batch(c, dev, codec, CRC, shape("edges"))
            assert rc == 0
            for (data, offs), (st, total, index, sums, img) in zip(shape("edges"), got):
                assert st == 0 and index[0] == 0 and index[-1] == total
                if data.size == 0:  # no partitions, or only an empty one: nothing is written
                    assert total == 0
                    continue
                d_out = dev.alloc(data.size)
                n = c.decompress_range_device(codec, CRC, dev.upload(img), total, index, sums, d_out, data.size)
                assert n == data.size
                assert np.array_equal(dev.download(d_out, n), data)
    finally:
        dev.free()


def test_capacity_one_byte_short_on_the_middle_task(gpu_codec, oracle):
    import s3shuffle

    ref = reference(oracle, "three", LZ4, ADLER)
    dev = Dev()
    try:
        rc, got = run_batch(gpu_codec, dev, LZ4, ADLER, shape("three"), caps=[None, ref[1][0].size - 1, None])
        assert rc == s3shuffle.codec.E_CAPACITY
        assert got[1][0] == s3shuffle.codec.E_CAPACITY
        assert_equals_oracle([got[0], got[2]], [ref[0], ref[2]], ADLER)
        # and with exactly the bytes it needs the same call passes (the status words of the last call are gone)
        rc, got = run_batch(gpu_codec, dev, LZ4, ADLER, shape("three"), caps=[None, ref[1][0].size, None])
        assert rc == 0
        assert_equals_oracle(got, ref, ADLER)
    finally:
        dev.free()


def test_arena_reused_at_alternating_sizes(oracle):
    """one context, five calls, large and small in turn: the arenas grow once and are then reused at another size"""
    import s3shuffle

    dev = Dev()
    try:
        with s3shuffle.Codec(0) as c:
            for name in ("large", "small", "large", "small", "large"):
                rc, got = run_batch(c, dev, LZ4, ADLER, shape(name))
                assert rc == 0
                assert_equals_oracle(got, reference(oracle, name, LZ4, ADLER), ADLER)
    finally:
        dev.free()


def test_first_call_of_a_fresh_context_is_the_batched_one(oracle):
    import s3shuffle

    dev = Dev()
    try:
        with s3shuffle.Codec(0) as c:
            rc, got = run_batch(c, dev, SNAPPY, CRC, shape("three"))
            assert rc == 0
            assert_equals_oracle(got, reference(oracle, "three", SNAPPY, CRC), CRC)
    finally:
        dev.free()
