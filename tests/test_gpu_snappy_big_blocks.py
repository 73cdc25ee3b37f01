"""GPU: Snappy block sizes above 32 KiB (spark.io.compression.snappy.blockSize 64k .. 32m, ABI 9).  Map side against the
oracle (SnappyOutputStream over libsnappy 1.1.8's fragment compressor), the batched forms against the single-task call,
JVM-style objects (oracle-written, two spills in one partition) through every reduce-side form, the option's bounds, the C++
host mirror, and a short damage run."""
import time

import numpy as np
import pytest

import corpus
from hipdev import Dev

pytestmark = pytest.mark.gpu

SNAPPY = 2
OPT_SNAPPY_BLOCK_SIZE, OPT_DECODE_VARIANT = 2, 5
ADLER, CRC, CRC32C = 1, 2, 3


class _BlockSize:
    """the context's Snappy block size for the duration of a with-block (reset in finally)"""

    def __init__(self, codec, bs):
        self.codec, self.bs = codec, bs

    def __enter__(self):
        self.old = self.codec.get_option(OPT_SNAPPY_BLOCK_SIZE)
        self.codec.set_option(OPT_SNAPPY_BLOCK_SIZE, self.bs)
        return self

    def __exit__(self, *exc):
        self.codec.set_option(OPT_SNAPPY_BLOCK_SIZE, self.old)


def _inputs(seed):
    from s3shuffle import datagen

    rng = np.random.default_rng(seed)
    ragged = corpus.ragged_map_output(rng, n_parts=14, max_len=1_500_000)
    tera = datagen.terasort_map_output(6 << 20, 7, seed=seed)
    wide = datagen.tpcds_wide_map_output(3 << 20, 5, seed=seed + 1)
    return [("ragged", ragged[0], ragged[1]), ("terasort", tera[0], tera[1]), ("wide", wide[0], wide[1])]


@pytest.mark.parametrize("bs", [32769, 65536, 131072, 1 << 20])
def test_map_side_matches_oracle(gpu_codec, oracle, bs):
    with _BlockSize(gpu_codec, bs):
        assert gpu_codec.get_option(OPT_SNAPPY_BLOCK_SIZE) == bs
        for name, data, offs in _inputs(bs % 1000):
            for algo in (ADLER, CRC, CRC32C):
                img, index, sums = gpu_codec.compress_map_output(SNAPPY, algo, data, offs)
                r_img, r_index, r_sums = oracle.compress_map_output(SNAPPY, algo, data, offs, block_size=bs)
                assert np.array_equal(index, r_index), (name, algo)
                assert np.array_equal(sums, r_sums), (name, algo)
                assert np.array_equal(img, r_img), (name, algo)
            back = gpu_codec.decompress_range(SNAPPY, algo, img, index, sums)
            assert np.array_equal(back, data), name
            assert gpu_codec.get_option(OPT_SNAPPY_BLOCK_SIZE) == bs


def test_batched_forms_equal_single_task_call(gpu_codec, oracle):
    bs = 131072
    inputs = _inputs(4)
    dev = Dev()
    try:
        with _BlockSize(gpu_codec, bs):
            singles = [gpu_codec.compress_map_output(SNAPPY, CRC, d, o) for _, d, o in inputs]
            tasks, host_tasks, host_dst = [], [], []
            for _, d, o in inputs:
                cap = gpu_codec.max_compressed_size(SNAPPY, o)
                tasks.append((dev.upload(d), o, dev.alloc(cap), cap))
                out = np.zeros(cap, np.uint8)
                host_dst.append(out)
                host_tasks.append((d.ctypes.data, o, out.ctypes.data, cap))
            res = gpu_codec.compress_map_outputs_batch_device(SNAPPY, CRC, tasks)
            hres = gpu_codec.compress_map_outputs_batch(SNAPPY, CRC, host_tasks)
            for (img, index, sums), (total, bi, bsums), (_, _, d_dst, _), (htotal, hi, hsums), hd in zip(
                    singles, res, tasks, hres, host_dst):
                assert total == img.size and np.array_equal(bi, index) and np.array_equal(bsums, sums)
                assert np.array_equal(dev.download(d_dst, total), img)
                assert htotal == img.size and np.array_equal(hi, index) and np.array_equal(hsums, sums)
                assert np.array_equal(hd[:htotal], img)
    finally:
        dev.free()


def _two_spill_object(oracle, data, offs, bs, algo):
    """an oracle-written object whose partition 1 is two concatenated streams (two spills merged)"""
    img, index, sums = oracle.compress_map_output(SNAPPY, algo, data, offs, block_size=bs)
    p = data[offs[1]:offs[2]]
    half = p.size // 2
    s1 = oracle.compress_stream(SNAPPY, p[:half], block_size=bs)
    s2 = oracle.compress_stream(SNAPPY, p[half:], block_size=bs)
    parts = [img[index[k]:index[k + 1]] for k in range(len(index) - 1)]
    parts[1] = np.concatenate([s1, s2])
    new_index = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([x.size for x in parts], out=new_index[1:])
    new_img = np.concatenate(parts)
    new_sums = np.array([oracle.checksum(algo, x) for x in parts], np.int64)
    return new_img, new_index, new_sums


@pytest.mark.parametrize("bs", [65536, 262144, 1 << 20])
def test_reduce_side_reads_jvm_style_objects(gpu_codec, oracle, bs):
    import s3shuffle
    from s3shuffle import datagen

    data, offs = datagen.tpcds_wide_map_output(5 << 20, 4, seed=bs % 97)
    img, index, sums = _two_spill_object(oracle, data, offs, bs, CRC)
    assert gpu_codec.decompressed_size(SNAPPY, img) == data.size
    assert np.array_equal(gpu_codec.decompress_range(SNAPPY, CRC, img, index, sums), data)
    dev = Dev()
    try:
        d_comp, d_dst = dev.upload(img), dev.alloc(data.size)
        (st, n, badp), = gpu_codec.decompress_ranges_batch_device(SNAPPY, CRC, [(d_comp, img.size, index, sums, d_dst, data.size)])
        assert st == 0 and n == data.size and np.array_equal(dev.download(d_dst, n), data)
        n1 = gpu_codec.decompress_range_device(SNAPPY, CRC, d_comp, img.size, index, sums, d_dst, data.size)
        assert n1 == data.size and np.array_equal(dev.download(d_dst, n1), data)
    finally:
        dev.free()
    out = np.zeros(data.size, np.uint8)
    (st, n, badp), = gpu_codec.decompress_ranges_batch(SNAPPY, CRC, [(img.ctypes.data, img.size, index, sums, out.ctypes.data, out.size)])
    assert st == 0 and n == data.size and np.array_equal(out, data)
    # a checksum mismatch names its partition
    wrong = sums.copy()
    wrong[2] ^= 1
    with pytest.raises(s3shuffle.CodecError) as e:
        gpu_codec.decompress_range(SNAPPY, CRC, img, index, wrong)
    assert e.value.code == s3shuffle.codec.E_CHECKSUM and e.value.partition == 2
    (st, n, badp), = gpu_codec.decompress_ranges_batch(SNAPPY, CRC, [(img.ctypes.data, img.size, index, wrong, out.ctypes.data, out.size)],
                                                       raise_on_error=False)
    assert st == s3shuffle.codec.E_CHECKSUM and badp == 2


def test_ring_decoder_keeps_its_32k_limit(gpu_codec, oracle):
    """decode variant 3 (the ring decoder) stays at 32 KiB chunks: a larger one is S3S_E_UNSUPPORTED, not a wrong answer"""
    import s3shuffle

    rng = np.random.default_rng(3)
    data = corpus.chunk_corpus(7, 200_000, rng)
    offs = np.array([0, data.size], np.int64)
    img, index, sums = oracle.compress_map_output(SNAPPY, CRC, data, offs, block_size=131072)
    old = gpu_codec.get_option(OPT_DECODE_VARIANT)
    gpu_codec.set_option(OPT_DECODE_VARIANT, 3)
    try:
        with pytest.raises(s3shuffle.CodecError) as e:
            gpu_codec.decompress_range(SNAPPY, CRC, img, index, sums)
        assert e.value.code == s3shuffle.codec.E_UNSUPPORTED
    finally:
        gpu_codec.set_option(OPT_DECODE_VARIANT, old)
    assert np.array_equal(gpu_codec.decompress_range(SNAPPY, CRC, img, index, sums), data)


def test_option_bounds(gpu_codec):
    old = gpu_codec.get_option(OPT_SNAPPY_BLOCK_SIZE)
    lib, h = gpu_codec._lib, gpu_codec._h
    try:
        for v in (1 << 25, 65537, 1 << 20, 1000):
            assert lib.s3s_set_option(h, OPT_SNAPPY_BLOCK_SIZE, v) == 0
            assert gpu_codec.get_option(OPT_SNAPPY_BLOCK_SIZE) == v
        assert lib.s3s_set_option(h, OPT_SNAPPY_BLOCK_SIZE, (1 << 25) + 1) == -6
        assert lib.s3s_set_option(h, OPT_SNAPPY_BLOCK_SIZE, 0) == -1
        assert lib.s3s_set_option(h, OPT_SNAPPY_BLOCK_SIZE, -5) == -1
        assert gpu_codec.get_option(OPT_SNAPPY_BLOCK_SIZE) == 1000  # (refused values leave the option alone)
    finally:
        gpu_codec.set_option(OPT_SNAPPY_BLOCK_SIZE, old)


def test_host_mirror_round_trip_at_128k(gpu_codec, oracle, tmp_path):
    from s3shuffle import datagen, host

    root = "file://" + str(tmp_path / "spark-s3-shuffle")
    d = host.Dispatcher(root, codec="snappy", block_size=131072, num_gpus=1)
    try:
        data, offs = datagen.tpcds_wide_map_output(3 << 20, 6, seed=8)
        spill = tmp_path / "spill_0.tmp"
        spill.write_bytes(data.tobytes())
        lengths = host.transfer_map_spill_file(d, 0, 4, str(spill), np.diff(offs))
        img, index, sums = oracle.compress_map_output(SNAPPY, ADLER, data, offs, block_size=131072)
        assert np.array_equal(lengths, np.diff(index))
        assert open(d.get_path(host.KIND_DATA, 0, 4), "rb").read() == img.tobytes()
        assert open(d.get_path(host.KIND_INDEX, 0, 4), "rb").read() == oracle.longs_to_be(index)
        assert open(d.get_path(host.KIND_CHECKSUM, 0, 4), "rb").read() == oracle.longs_to_be(sums)
        got = host.read_shuffle(d, 0, 0, 6, True)
        assert len(got) == 1 and np.array_equal(got[0][4], data)
        got = host.read_shuffle(d, 0, 2, 5, False, sequential=True)
        assert np.array_equal(np.concatenate([g[4] for g in got]), data[offs[2]:offs[5]])
        d.remove_root()
    finally:
        d.close()


@pytest.mark.parametrize("bs", [131072, 1 << 20])
def test_damaged_big_chunks_fail_cleanly(gpu_codec, oracle, bs):
    """a few seconds of damaged oracle images with checksums off: the data, or -2 / -3 / -6 — never a fault or a hang"""
    import s3shuffle
    from s3shuffle import datagen

    rng = np.random.default_rng(bs)
    data, offs = datagen.tpcds_wide_map_output(3 << 20, 3, seed=5)
    img, index, _ = oracle.compress_map_output(SNAPPY, 0, data, offs, block_size=bs)
    t0, rounds, refused = time.time(), 0, 0
    while time.time() - t0 < 4.0:
        bad = img.copy()
        for _ in range(int(rng.integers(1, 6))):
            p = int(rng.integers(16, bad.size))
            bad[p] = (int(bad[p]) + int(rng.integers(1, 256))) & 0xFF
        try:
            back = gpu_codec.decompress_range(SNAPPY, 0, bad, index, None, dst_capacity=data.size + 65536)
            assert back.size <= data.size + 65536
        except s3shuffle.CodecError as e:
            assert e.code in (-2, -3, -6), e.code
            refused += 1
        rounds += 1
    assert rounds > 3 and refused > 0
    assert np.array_equal(gpu_codec.decompress_range(SNAPPY, 0, img, index, None), data)  # the context still works
