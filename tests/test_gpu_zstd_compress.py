"""GPU: the Zstandard map side (S3S_OPT_ZSTD_COMPRESS = 1, ABI 11).  The frames are not libzstd's bytes; what they owe is
that libzstd 1.4.8 and this library decode every one of them to its source, that index and checksums describe the image, that
the image is a pure function of the source (equal across entry points, batch composition and calls - and equal to the frames
the host build of the same writer produces, parse included), and that they are smaller than what a writer without entropy
coding of the literals could reach (the three size conditions)."""
import os
import sys

import numpy as np
import pytest

import corpus

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_encode_model_lib as E  # noqa: E402

pytestmark = pytest.mark.gpu

ZSTD, LZ4, LZF = 3, 1, 4
ADLER, CRC = 1, 2
OPT_ZSTD_COMPRESS = 9
B = E.BLOCK


@pytest.fixture()
def zc(gpu_codec):
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    try:
        yield gpu_codec
    finally:
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)


_cache = {}


def inputs():
    """name -> (data, offsets): built once, never modified."""
    if not _cache:
        from s3shuffle import datagen

        rng = np.random.default_rng(17)
        words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(200)]
        text = np.frombuffer(b" ".join(words[int(i)] for i in rng.integers(0, 200, 90_000)), dtype=np.uint8)
        sizes = [0, 1, 2, 3, B - 1, 0, B, B + 1]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        _cache["edges"] = (np.ascontiguousarray(text[:offs[-1]]), offs)
        _cache["zeros"] = datagen.skew_block(1 << 20, "zeros", seed=5)
        _cache["random"] = datagen.skew_block(1 << 20, "random", seed=5)
        _cache["terasort"] = datagen.terasort_map_output(4 << 20, 8, seed=2)
        _cache["wide"] = datagen.tpcds_wide_map_output(4 << 20, 8, seed=3)
        _cache["kv"] = datagen.kv_int_map_output(300_000, 7, seed=1)
        for d, _ in _cache.values():
            d.flags.writeable = False
    return _cache


def model_image(data, offs, name=None):
    """The frames the host build of the writer produces (those of the named inputs are kept)."""
    key = ("model", name)
    if name is None or key not in _cache:
        m = E.load()
        frames = [E.encode_frame(m, data[offs[p]:offs[p + 1]]) for p in range(len(offs) - 1)]
        if name is None:
            return frames
        _cache[key] = frames
    return _cache[key]


def check_image(codec, oracle, algo, data, offs, img, index, sums, name=None):
    from oracle import zstd_ref

    n = len(offs) - 1
    assert index[0] == 0 and index[-1] == img.size and np.all(np.diff(index) >= 0)
    for p in range(n):
        part, src = img[index[p]:index[p + 1]], data[offs[p]:offs[p + 1]]
        if src.size == 0:
            assert part.size == 0  # an empty partition is 0 bytes
            continue
        assert bytes(part[:6]) == b"\x28\xb5\x2f\xfd\xc0\x38" and int.from_bytes(bytes(part[6:14]), "little") == src.size
        back = zstd_ref.decompress(part, src.size)
        assert back is not None and np.array_equal(back, src), "libzstd does not decode partition %d to its source" % p
        if algo:
            assert int(sums[p]) == oracle.checksum(algo, part)
    # the index is the cumulative frame lengths - of exactly the frames the host build of the writer produces
    frames = model_image(data, offs, name)
    assert np.array_equal(np.diff(index), [f.size for f in frames])
    assert np.array_equal(img, np.concatenate(frames))
    assert codec.decompressed_size(ZSTD, img) == data.size
    out = codec.decompress_range(ZSTD, algo, img, index, sums, dst_capacity=data.size)
    assert np.array_equal(out, data)
    if n > 3:
        r0, r1 = 1, n - 1
        out = codec.decompress_range(ZSTD, algo, img[index[r0]:index[r1]], index[r0:r1 + 1] - index[r0], None if not algo else sums[r0:r1],
                                     dst_capacity=int(offs[r1] - offs[r0]))
        assert np.array_equal(out, data[offs[r0]:offs[r1]])


@pytest.mark.parametrize("algo", [ADLER, CRC, 0])
@pytest.mark.parametrize("name", ["edges", "zeros", "random", "terasort", "wide", "kv"])
def test_images_decode_everywhere(zc, oracle, name, algo):
    data, offs = inputs()[name]
    img, index, sums = zc.compress_map_output(ZSTD, algo, data, offs)
    check_image(zc, oracle, algo, data, offs, img, index, sums, name)


def test_size_conditions(zc):
    """Conditions, not measurements: a raw-block or raw-literal writer meets none of them.  TeraSort has no condition; its
    figure is printed (-s) next to the others."""
    ins = inputs()
    sizes = {}
    for name in ("wide", "kv", "zeros", "terasort"):
        data, offs = ins[name]
        sizes[name] = (data.size, zc.compress_map_output(ZSTD, ADLER, data, offs)[0].size,
                       zc.compress_map_output(LZ4, ADLER, data, offs)[0].size)
        print("%-9s source %9d  zstd image %9d  lz4 image %9d" % ((name,) + sizes[name]))
    assert sizes["wide"][1] < sizes["wide"][2], "wide rows: not smaller than the LZ4 image of the same call"
    assert sizes["kv"][1] < sizes["kv"][0], "kv: not smaller than its source"
    assert sizes["zeros"][1] * 1000 < sizes["zeros"][0], "zeros: not below 1 / 1000 of the source"


def test_entry_points_give_one_image(zc, oracle):
    from hipdev import Dev

    ins = inputs()
    tasks = [ins["wide"], ins["edges"], ins["kv"]]
    single = [zc.compress_map_output(ZSTD, CRC, d, o) for d, o in tasks]
    again = [zc.compress_map_output(ZSTD, CRC, d, o) for d, o in tasks]
    for a, b in zip(single, again):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "two calls, two images"
    dev = Dev()
    try:
        args, outs = [], []
        for (d, o), (img, _, _) in zip(tasks, single):
            cap = zc.max_compressed_size(ZSTD, o)
            assert cap >= img.size
            d_out = dev.alloc(cap + 16)
            outs.append((d_out, cap))
            args.append((dev.upload(d), o, d_out, cap))
        res = zc.compress_map_outputs_batch_device(ZSTD, CRC, args)
        for (total, index, sums), (d_out, cap), (img, sindex, ssums) in zip(res, outs, single):
            assert total == img.size and np.array_equal(index, sindex) and np.array_equal(sums, ssums)
            assert np.array_equal(dev.download(d_out, total), img)
        # the device form of one task, and the answer one byte short
        d, o = tasks[0]
        total, index, sums = zc.compress_map_output_device(ZSTD, CRC, args[0][0], o, outs[0][0], outs[0][1])
        assert total == single[0][0].size and np.array_equal(index, single[0][1]) and np.array_equal(dev.download(outs[0][0], total), single[0][0])
        import s3shuffle

        with pytest.raises(s3shuffle.CodecError) as ei:
            zc.compress_map_output_device(ZSTD, CRC, args[0][0], o, outs[0][0], total - 1)
        assert ei.value.code == s3shuffle.codec.E_CAPACITY
    finally:
        dev.free()
    # the host-buffer batch (the form the JNI shim binds)
    houts = [np.zeros(zc.max_compressed_size(ZSTD, o), np.uint8) for _, o in tasks]
    hres = zc.compress_map_outputs_batch(ZSTD, CRC, [(d.ctypes.data, o, out.ctypes.data, out.size) for (d, o), out in zip(tasks, houts)])
    for (total, index, sums), out, (img, sindex, ssums) in zip(hres, houts, single):
        assert total == img.size and np.array_equal(out[:total], img) and np.array_equal(index, sindex) and np.array_equal(sums, ssums)


def test_segments_are_concatenated_frames(zc, oracle):
    """A partition of three spill pieces is three frames back to back; an empty piece adds nothing."""
    from oracle import zstd_ref

    data, _ = inputs()["wide"]
    data = data[:700_000]
    segs = np.array([0, 200_000, 200_000, 200_001, 460_000, 700_000], np.int64)
    pfs = np.array([0, 1, 4, 5], np.int32)   # partition 1 = pieces 1 (empty), 2 (1 byte), 3
    for algo in (ADLER, 0):
        img, index, sums = zc.compress_map_output_segments(ZSTD, algo, data, segs, pfs)
        m = E.load()
        frames = [E.encode_frame(m, data[segs[g]:segs[g + 1]]) for g in range(5)]
        assert np.array_equal(img, np.concatenate(frames))
        assert list(index) == [0, frames[0].size, frames[0].size + sum(f.size for f in frames[1:4]), img.size]
        part1 = img[index[1]:index[2]]
        assert np.array_equal(zstd_ref.decompress(part1, 500_000), data[200_000:460_000])
        if algo:
            assert [int(s) for s in sums] == [oracle.checksum(algo, img[index[p]:index[p + 1]]) for p in range(3)]
        assert np.array_equal(zc.decompress_range(ZSTD, algo, img, index, sums, dst_capacity=data.size), data)
        assert zc.decompressed_size(ZSTD, img) == data.size


def test_bound_capacity_and_the_switch(gpu_codec):
    import s3shuffle

    data, offs = inputs()["random"]
    lib, h = gpu_codec._lib, gpu_codec._h
    assert gpu_codec.get_option(OPT_ZSTD_COMPRESS) == 0
    with pytest.raises(s3shuffle.CodecError) as ei:  # off: no bound, no compression
        gpu_codec.max_compressed_size(ZSTD, offs)
    assert ei.value.code == s3shuffle.codec.E_INVALID
    assert lib.s3s_set_option(h, OPT_ZSTD_COMPRESS, 2) == -1 and lib.s3s_set_option(h, OPT_ZSTD_COMPRESS, -1) == -1
    assert gpu_codec.get_option(OPT_ZSTD_COMPRESS) == 0
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    try:
        assert gpu_codec.get_option(OPT_ZSTD_COMPRESS) == 1
        bound = gpu_codec.max_compressed_size(ZSTD, offs)
        img, index, sums = gpu_codec.compress_map_output(ZSTD, ADLER, data, offs)
        assert data.size < img.size <= bound  # random bytes: Raw blocks
        n = len(offs) - 1
        blocks = sum(-(-int(offs[p + 1] - offs[p]) // B) for p in range(n))
        assert img.size == data.size + 3 * blocks + 14 * sum(1 for p in range(n) if offs[p + 1] > offs[p])
        with pytest.raises(s3shuffle.CodecError) as ei:
            gpu_codec.compress_map_output(ZSTD, ADLER, data, offs, dst_capacity=img.size - 1)
        assert ei.value.code == s3shuffle.codec.E_CAPACITY
        # the other decode-only codec stays refused: the host forms size their staging through s3s_max_compressed_size first and
        # answer its S3S_E_INVALID (as they did before ABI 11), the device forms answer S3S_E_UNSUPPORTED
        with pytest.raises(s3shuffle.CodecError) as ei:
            gpu_codec.compress_map_output(LZF, ADLER, data[:1000], [0, 1000], dst_capacity=4096)
        assert ei.value.code == s3shuffle.codec.E_INVALID
        assert device_call_code(gpu_codec, LZF, data) == s3shuffle.codec.E_UNSUPPORTED
        assert max_size_null_ctx(lib, offs) == -1
    finally:
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)
    with pytest.raises(s3shuffle.CodecError) as ei:  # off again: refused again, with the answers of ABI 10
        gpu_codec.compress_map_output(ZSTD, ADLER, data, offs, dst_capacity=data.size + 4096)
    assert ei.value.code == s3shuffle.codec.E_INVALID
    assert device_call_code(gpu_codec, ZSTD, data) == s3shuffle.codec.E_UNSUPPORTED


def device_call_code(codec, codec_id, data):
    """The return code of s3s_compress_map_output_device and of s3s_compress_map_output_segments_device (they must agree)."""
    import ctypes

    from hipdev import Dev

    dev = Dev()
    try:
        d_src, d_dst = dev.upload(data[:4096]), dev.alloc(8192)
        offs, pfs = np.array([0, 4096], np.int64), np.array([0, 1], np.int32)
        index, sums, total = np.zeros(2, np.int64), np.zeros(1, np.int64), ctypes.c_int64(0)
        i64p = ctypes.POINTER(ctypes.c_int64)
        a = codec._lib.s3s_compress_map_output_device(codec._h, codec_id, ADLER, ctypes.c_void_p(d_src), offs.ctypes.data_as(i64p), 1,
                                                      ctypes.c_void_p(d_dst), 8192, index.ctypes.data_as(i64p), sums.ctypes.data_as(i64p),
                                                      ctypes.byref(total))
        b = codec._lib.s3s_compress_map_output_segments_device(codec._h, codec_id, ADLER, ctypes.c_void_p(d_src), offs.ctypes.data_as(i64p), 1,
                                                               pfs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, ctypes.c_void_p(d_dst), 8192,
                                                               index.ctypes.data_as(i64p), sums.ctypes.data_as(i64p), ctypes.byref(total))
        assert a == b
        return a
    finally:
        dev.free()


def test_segments_device_form(zc, oracle):
    """s3s_compress_map_output_segments_device: the eighth entry point, device buffers and spill pieces."""
    import ctypes

    from hipdev import Dev

    data, _ = inputs()["terasort"]
    data = data[:600_000]
    segs = np.array([0, 150_000, 150_000, 420_000, 600_000], np.int64)
    pfs = np.array([0, 3, 3, 4], np.int32)  # partition 0 = three pieces (one empty), partition 1 empty, partition 2 = one piece
    m = E.load()
    frames = [E.encode_frame(m, data[segs[g]:segs[g + 1]]) for g in range(4)]
    want = np.concatenate(frames)
    dev = Dev()
    try:
        cap = int(zc._lib.s3s_max_compressed_size_segments(zc._h, ZSTD, segs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 4))
        assert cap >= want.size
        d_src, d_dst = dev.upload(data), dev.alloc(cap + 16)
        index, sums, total = np.zeros(4, np.int64), np.zeros(3, np.int64), ctypes.c_int64(0)
        i64p = ctypes.POINTER(ctypes.c_int64)
        rc = zc._lib.s3s_compress_map_output_segments_device(zc._h, ZSTD, CRC, ctypes.c_void_p(d_src), segs.ctypes.data_as(i64p), 4,
                                                             pfs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 3, ctypes.c_void_p(d_dst), cap,
                                                             index.ctypes.data_as(i64p), sums.ctypes.data_as(i64p), ctypes.byref(total))
        assert rc == 0 and total.value == want.size
        img = dev.download(d_dst, total.value)
    finally:
        dev.free()
    assert np.array_equal(img, want)
    first = sum(f.size for f in frames[:3])
    assert list(index) == [0, first, first, want.size]
    assert [int(x) for x in sums] == [oracle.checksum(CRC, img[index[p]:index[p + 1]]) for p in range(3)]
    assert np.array_equal(zc.decompress_range(ZSTD, CRC, img, index, sums, dst_capacity=data.size), data)


def test_more_blocks_than_resident_workgroups(zc, oracle):
    """A production-sized call: ~150 MiB in 56 partitions is ~1 150 blocks for a persistent grid of 3 workgroups per compute unit
    (768 on an MI355X), so workgroups take a second and a third block - table, histogram, plan and the sequence / literal
    scratch are reused, after compressed blocks and after the RLE blocks and frame headers that leave the loop early.  The image
    must still be the host build's, byte for byte, and decode under libzstd and on the GPU."""
    from hipdev import Dev
    from oracle import zstd_ref

    ins = inputs()
    rng = np.random.default_rng(77)
    pool = [ins["wide"][0], ins["terasort"][0], ins["kv"][0], ins["random"][0][:300_000]]
    parts = []
    for p in range(56):
        if p % 8 == 5:  # all-equal stretches: RLE blocks between the compressed ones
            parts.append(np.full(int(rng.integers(1, 5)) * B + int(rng.integers(0, 3)), p, np.uint8))
            continue
        pieces, want = [], int(rng.integers(2_000_000, 3_900_000))
        while want > 0:
            src = pool[int(rng.integers(0, len(pool)))]
            at = int(rng.integers(0, src.size - 1000))
            take = min(want, int(rng.integers(1000, 1_500_000)), src.size - at)
            pieces.append(src[at:at + take])
            want -= take
        parts.append(np.concatenate(pieces))
    offs = np.concatenate([[0], np.cumsum([q.size for q in parts])]).astype(np.int64)
    data = np.concatenate(parts)
    n = len(parts)
    n_items = sum(1 + -(-q.size // B) for q in parts)
    assert n_items > 768 + 256, "not enough blocks to make a workgroup take a second one"
    frames = model_image(data, offs)
    want = np.concatenate(frames)
    dev = Dev()
    try:
        cap = zc.max_compressed_size(ZSTD, offs)
        d_src, d_dst = dev.upload(data), dev.alloc(cap + 16)
        total, index, sums = zc.compress_map_output_device(ZSTD, ADLER, d_src, offs, d_dst, cap)
        img = dev.download(d_dst, total)
        total2, index2, sums2 = zc.compress_map_output_device(ZSTD, ADLER, d_src, offs, d_dst, cap)
        assert total2 == total and np.array_equal(dev.download(d_dst, total2), img) and np.array_equal(sums, sums2)
        # the same partitions as two tasks of one batch: another launch shape, other workgroups for every block
        half = n // 2
        d_dst2 = dev.alloc(cap + 16)
        offs_b = offs[half:]
        res = zc.compress_map_outputs_batch_device(ZSTD, ADLER, [(d_src, offs[:half + 1], d_dst, cap), (d_src, offs_b, d_dst2, cap)])
        got = np.concatenate([dev.download(d_dst, res[0][0]), dev.download(d_dst2, res[1][0])])
        assert np.array_equal(got, img), "the bytes depend on the launch shape"
    finally:
        dev.free()
    assert np.array_equal(np.diff(index), [f.size for f in frames])
    assert np.array_equal(img, want), "first difference at byte %d" % int(np.argmax(img[:min(img.size, want.size)] != want[:min(img.size, want.size)]))
    for p in (0, 5, 13, n - 1):
        back = zstd_ref.decompress(img[index[p]:index[p + 1]], parts[p].size)
        assert back is not None and np.array_equal(back, parts[p])
        assert int(sums[p]) == oracle.checksum(ADLER, img[index[p]:index[p + 1]])
    assert np.array_equal(zstd_ref.decompress(img, data.size), data)
    assert np.array_equal(zc.decompress_range(ZSTD, ADLER, img, index, sums, dst_capacity=data.size), data)


def max_size_null_ctx(lib, offs):
    import ctypes

    o = np.ascontiguousarray(offs, dtype=np.int64)
    return int(lib.s3s_max_compressed_size(None, ZSTD, o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(o) - 1))


def test_seeded_shapes_round_trip(zc, oracle):
    """One seeded loop over the corpus shapes (every kind, ragged partition lengths around the block size, empty ones)."""
    rng = np.random.default_rng(2026)
    for round_ in range(4):
        parts = []
        for p in range(14):
            kind = int(rng.integers(0, corpus.N_KINDS))
            n = int(rng.choice([0, 1, 7, 300, 5000, 40_000, B - 3, B, B + 2, 200_000]))
            if kind == 6:
                n = min(n, 5000)
            parts.append(corpus.chunk_corpus(kind, n, rng))
        offs = np.concatenate([[0], np.cumsum([q.size for q in parts])]).astype(np.int64)
        data = np.concatenate(parts)
        algo = (ADLER, CRC, 0, ADLER)[round_]
        img, index, sums = zc.compress_map_output(ZSTD, algo, data, offs)
        check_image(zc, oracle, algo, data, offs, img, index, sums)
