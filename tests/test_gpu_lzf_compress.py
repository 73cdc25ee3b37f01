"""GPU: the LZF map side (S3S_OPT_LZF_COMPRESS = 1, key 10).  The streams are not compress-lzf's bytes; what they owe is that
the oracle's decoder and this library decode every one of them to its source, that index and checksums describe the image,
that the image is a pure function of the source (equal across entry points, batch composition and calls - and equal to the
streams the host build of the same writer produces, parse included, which tests/test_lzf_encode_model.py has liblzf read),
and that the parse is no worse than the size conditions allow (the bound is the oracle's image of the same call, computed here).

The kernel's grid is one workgroup per plan item, not a persistent one: there is no "more chunks than the grid" case."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lzf_encode_model_lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

LZ4, ZSTD, LZF = 1, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
OPT_ZSTD_COMPRESS, OPT_LZF_COMPRESS = 9, 10
E_INVALID, E_CAPACITY, E_UNSUPPORTED, STATUS_NOT_RUN = -1, -2, -6, -100


@pytest.fixture()
def lc(gpu_codec):
    gpu_codec.set_option(OPT_LZF_COMPRESS, 1)
    try:
        yield gpu_codec
    finally:
        gpu_codec.set_option(OPT_LZF_COMPRESS, 0)


def check_image(codec, oracle, algo, data, offs, img, index, sums, name=None):
    n = len(offs) - 1
    assert index[0] == 0 and index[-1] == img.size and np.all(np.diff(index) >= 0)
    # the host build's streams, byte for byte: the index is their cumulative lengths
    streams = L.model_streams(data, offs, name)
    assert np.array_equal(np.diff(index), [s.size for s in streams])
    want = np.concatenate(streams) if streams else np.zeros(0, np.uint8)
    assert np.array_equal(img, want), "first difference at byte %d" % int(np.argmax(img[:want.size] != want[:img.size]))
    for p in range(n):
        part = img[index[p]:index[p + 1]]
        if offs[p + 1] == offs[p]:
            assert part.size == 0  # an empty partition is 0 bytes
        if algo:
            assert int(sums[p]) == oracle.checksum(algo, part)
    # every partition decodes to its source: by the oracle (checksums verified first) ...
    rc, back, bad = oracle.decompress_range(LZF, algo, img, index, sums if algo else None, data.size)
    assert rc == 0 and bad == -1 and np.array_equal(back, data)
    # ... and by this library
    assert codec.decompressed_size(LZF, img) == data.size
    out = codec.decompress_range(LZF, algo, img, index, sums if algo else None, dst_capacity=data.size)
    assert np.array_equal(out, data)
    if n > 3:
        r0, r1 = 1, n - 1
        out = codec.decompress_range(LZF, algo, img[index[r0]:index[r1]], index[r0:r1 + 1] - index[r0], None if not algo else sums[r0:r1],
                                     dst_capacity=int(offs[r1] - offs[r0]))
        assert np.array_equal(out, data[offs[r0]:offs[r1]])


@pytest.mark.parametrize("algo", [ADLER, CRC, CRC32C, 0])
@pytest.mark.parametrize("name", ["edges", "zeros", "random", "terasort", "wide", "kv"])
def test_images_equal_the_host_build_and_decode(lc, oracle, name, algo):
    data, offs = L.inputs()[name]
    img, index, sums = lc.compress_map_output(LZF, algo, data, offs)
    assert img.size <= lc.max_compressed_size(LZF, offs) == sum(L.stream_bound(int(offs[p + 1] - offs[p])) for p in range(len(offs) - 1))
    check_image(lc, oracle, algo, data, offs, img, index, sums, name)


def test_size_conditions(lc, oracle):
    ins = L.inputs()
    sizes = {name: lc.compress_map_output(LZF, ADLER, *ins[name])[0].size for name in L.NAMED}
    L.check_size_conditions(sizes, oracle)


def test_entry_points_give_one_image(lc, oracle):
    from hipdev import Dev

    ins = L.inputs()
    tasks = [ins["wide"], ins["edges"], ins["kv"]]
    single = [lc.compress_map_output(LZF, CRC, d, o) for d, o in tasks]
    again = [lc.compress_map_output(LZF, CRC, d, o) for d, o in tasks]
    for a, b in zip(single, again):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "two calls, two images"
    dev = Dev()
    try:
        args, outs = [], []
        for (d, o), (img, _, _) in zip(tasks, single):
            cap = lc.max_compressed_size(LZF, o)
            assert cap >= img.size
            d_out = dev.alloc(cap + 16)
            outs.append((d_out, cap))
            args.append((dev.upload(d), o, d_out, cap))
        res = lc.compress_map_outputs_batch_device(LZF, CRC, args)  # three tasks in one batch
        for (total, index, sums), (d_out, cap), (img, sindex, ssums) in zip(res, outs, single):
            assert total == img.size and np.array_equal(index, sindex) and np.array_equal(sums, ssums)
            assert np.array_equal(dev.download(d_out, total), img)
        (total, index, sums), = lc.compress_map_outputs_batch_device(LZF, CRC, args[:1])  # a batch of one
        assert total == single[0][0].size and np.array_equal(index, single[0][1]) and np.array_equal(sums, single[0][2])
        assert np.array_equal(dev.download(outs[0][0], total), single[0][0])
        # the device form of one task, and the answer one byte short
        d, o = tasks[0]
        total, index, sums = lc.compress_map_output_device(LZF, CRC, args[0][0], o, outs[0][0], outs[0][1])
        assert total == single[0][0].size and np.array_equal(index, single[0][1]) and np.array_equal(dev.download(outs[0][0], total), single[0][0])
        import s3shuffle

        with pytest.raises(s3shuffle.CodecError) as ei:
            lc.compress_map_output_device(LZF, CRC, args[0][0], o, outs[0][0], total - 1)
        assert ei.value.code == E_CAPACITY
        # one batched device call of the reduce side reads the three images back
        d_imgs = [dev.upload(img) for img, _, _ in single]
        d_back = [dev.upload(np.full(d.size + 16, 0xA5, np.uint8)) for d, _ in tasks]
        dres = lc.decompress_ranges_batch_device(LZF, CRC, [(d_img, img.size, index, sums, d_b, d.size)
                                                           for d_img, (img, index, sums), d_b, (d, _) in zip(d_imgs, single, d_back, tasks)])
        for (st, nbytes, bad), d_b, (d, _) in zip(dres, d_back, tasks):
            back = dev.download(d_b, d.size + 16)
            assert st == 0 and nbytes == d.size and np.array_equal(back[:nbytes], d) and np.all(back[nbytes:] == 0xA5)
    finally:
        dev.free()
    # the host-buffer batch (the form the JNI shim binds)
    houts = [np.zeros(lc.max_compressed_size(LZF, o), np.uint8) for _, o in tasks]
    hres = lc.compress_map_outputs_batch(LZF, CRC, [(d.ctypes.data, o, out.ctypes.data, out.size) for (d, o), out in zip(tasks, houts)])
    for (total, index, sums), out, (img, sindex, ssums) in zip(hres, houts, single):
        assert total == img.size and np.array_equal(out[:total], img) and np.array_equal(index, sindex) and np.array_equal(sums, ssums)


def test_segments_are_concatenated_streams(lc, oracle):
    """A partition of three spill pieces is the chunks of three streams back to back; an empty piece adds nothing.  With one
    piece per partition the segments form gives the image of the plain form."""
    data, _ = L.inputs()["wide"]
    data = data[:700_000]
    segs = np.array([0, 200_000, 200_000, 200_001, 460_000, 700_000], np.int64)
    pfs = np.array([0, 1, 4, 5], np.int32)   # partition 1 = pieces 1 (empty), 2 (1 byte), 3
    m = L.load()
    streams = [L.encode_stream(m, data[segs[g]:segs[g + 1]]) for g in range(5)]
    for algo in (ADLER, 0):
        img, index, sums = lc.compress_map_output_segments(LZF, algo, data, segs, pfs)
        assert np.array_equal(img, np.concatenate(streams))
        assert list(index) == [0, streams[0].size, streams[0].size + sum(s.size for s in streams[1:4]), img.size]
        if algo:
            assert [int(s) for s in sums] == [oracle.checksum(algo, img[index[p]:index[p + 1]]) for p in range(3)]
        rc, back, bad = oracle.decompress_range(LZF, algo, img, index, sums if algo else None, data.size)
        assert rc == 0 and np.array_equal(back, data)
        assert np.array_equal(lc.decompress_range(LZF, algo, img, index, sums if algo else None, dst_capacity=data.size), data)
        assert lc.decompressed_size(LZF, img) == data.size
    plain = lc.compress_map_output(LZF, CRC, data, segs)
    one_each = lc.compress_map_output_segments(LZF, CRC, data, segs, np.arange(6, dtype=np.int32))
    assert all(np.array_equal(a, b) for a, b in zip(plain, one_each))


def test_segments_device_form(lc, oracle):
    """s3s_compress_map_output_segments_device: device buffers and spill pieces, sized by s3s_max_compressed_size_segments."""
    from hipdev import Dev

    data, _ = L.inputs()["terasort"]
    data = data[:600_000]
    segs = np.array([0, 150_000, 150_000, 420_000, 600_000], np.int64)
    pfs = np.array([0, 3, 3, 4], np.int32)  # partition 0 = three pieces (one empty), partition 1 empty, partition 2 = one piece
    m = L.load()
    streams = [L.encode_stream(m, data[segs[g]:segs[g + 1]]) for g in range(4)]
    want = np.concatenate(streams)
    i64p = ctypes.POINTER(ctypes.c_int64)
    dev = Dev()
    try:
        cap = int(lc._lib.s3s_max_compressed_size_segments(lc._h, LZF, segs.ctypes.data_as(i64p), 4))
        assert cap == sum(L.stream_bound(int(segs[g + 1] - segs[g])) for g in range(4)) >= want.size
        d_src, d_dst = dev.upload(data), dev.alloc(cap + 16)
        index, sums, total = np.zeros(4, np.int64), np.zeros(3, np.int64), ctypes.c_int64(0)
        rc = lc._lib.s3s_compress_map_output_segments_device(lc._h, LZF, CRC, ctypes.c_void_p(d_src), segs.ctypes.data_as(i64p), 4,
                                                             pfs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 3, ctypes.c_void_p(d_dst), cap,
                                                             index.ctypes.data_as(i64p), sums.ctypes.data_as(i64p), ctypes.byref(total))
        assert rc == 0 and total.value == want.size
        img = dev.download(d_dst, total.value)
    finally:
        dev.free()
    assert np.array_equal(img, want)
    first = sum(s.size for s in streams[:3])
    assert list(index) == [0, first, first, want.size]
    assert [int(x) for x in sums] == [oracle.checksum(CRC, img[index[p]:index[p + 1]]) for p in range(3)]
    assert np.array_equal(lc.decompress_range(LZF, CRC, img, index, sums, dst_capacity=data.size), data)


def device_call_code(codec, codec_id, data):
    """The return code of s3s_compress_map_output_device and of s3s_compress_map_output_segments_device (they must agree)."""
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


def batch_call(codec, codec_id, data):
    """(return code, per-task status) of s3s_compress_map_outputs_batch over two host tasks."""
    from s3shuffle import codec as sc

    src = np.ascontiguousarray(data[:4096])
    dsts = [np.zeros(8192, np.uint8) for _ in range(2)]
    arr = (sc.MapTask * 2)()
    keep = []
    for i in range(2):
        offs, index = np.array([0, 4096], np.int64), np.zeros(2, np.int64)
        keep.append((offs, index))
        arr[i].d_src, arr[i].src_offsets, arr[i].num_partitions = src.ctypes.data, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1
        arr[i].d_dst, arr[i].dst_capacity = dsts[i].ctypes.data, 8192
        arr[i].out_index = index.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    rc = codec._lib.s3s_compress_map_outputs_batch(codec._h, codec_id, 0, arr, 2)
    return rc, [arr[i].status for i in range(2)]


def test_bound_capacity_and_the_switch(gpu_codec):
    import s3shuffle

    data, offs = L.inputs()["random"]
    text = L.inputs()["edges"][0]
    lib, h = gpu_codec._lib, gpu_codec._h
    assert gpu_codec.get_option(OPT_LZF_COMPRESS) == 0
    with pytest.raises(s3shuffle.CodecError) as ei:  # off: no bound, no compression
        gpu_codec.max_compressed_size(LZF, offs)
    assert ei.value.code == E_INVALID
    assert lib.s3s_set_option(h, OPT_LZF_COMPRESS, 2) == E_INVALID and lib.s3s_set_option(h, OPT_LZF_COMPRESS, -1) == E_INVALID
    assert gpu_codec.get_option(OPT_LZF_COMPRESS) == 0
    gpu_codec.set_option(OPT_LZF_COMPRESS, 1)
    try:
        assert lib.s3s_set_option(h, OPT_LZF_COMPRESS, 2) == E_INVALID and lib.s3s_set_option(h, OPT_LZF_COMPRESS, -1) == E_INVALID
        assert gpu_codec.get_option(OPT_LZF_COMPRESS) == 1   # refused values leave the option alone
        bound = gpu_codec.max_compressed_size(LZF, offs)
        img, index, sums = gpu_codec.compress_map_output(LZF, ADLER, data, offs)
        assert data.size < img.size <= bound  # random bytes: stored chunks
        with pytest.raises(s3shuffle.CodecError) as ei:
            gpu_codec.compress_map_output(LZF, ADLER, data, offs, dst_capacity=img.size - 1)
        assert ei.value.code == E_CAPACITY
        assert device_call_code(gpu_codec, LZF, text) == 0
        assert batch_call(gpu_codec, LZF, text) == (0, [0, 0])
        # key 10 does not open Zstandard, and a null context has no option
        assert device_call_code(gpu_codec, ZSTD, text) == E_UNSUPPORTED
        o = np.ascontiguousarray(offs, dtype=np.int64)
        assert int(lib.s3s_max_compressed_size(None, LZF, o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(o) - 1)) == E_INVALID
    finally:
        gpu_codec.set_option(OPT_LZF_COMPRESS, 0)
    # off again: refused again, with the answers the library gave before the key existed
    with pytest.raises(s3shuffle.CodecError) as ei:
        gpu_codec.compress_map_output(LZF, ADLER, data, offs, dst_capacity=data.size + 4096)
    assert ei.value.code == E_INVALID   # (the host form sizes its staging through s3s_max_compressed_size first)
    assert device_call_code(gpu_codec, LZF, text) == E_UNSUPPORTED
    rc, status = batch_call(gpu_codec, LZF, text)
    assert rc in (E_INVALID, E_UNSUPPORTED) and status == [STATUS_NOT_RUN] * 2
    # Zstandard's key on, this one off: LZF stays refused
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    try:
        assert device_call_code(gpu_codec, LZF, text) == E_UNSUPPORTED
        assert device_call_code(gpu_codec, ZSTD, text) == 0
        with pytest.raises(s3shuffle.CodecError) as ei:
            gpu_codec.max_compressed_size(LZF, offs)
        assert ei.value.code == E_INVALID
    finally:
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)


def test_seeded_shapes_round_trip(lc, oracle):
    """One seeded loop over the corpus shapes (every kind, ragged partition lengths around the chunk size, empty ones)."""
    import corpus

    rng = np.random.default_rng(2027)
    C = L.CHUNK
    for round_ in range(4):
        parts = []
        for p in range(14):
            kind = int(rng.integers(0, corpus.N_KINDS))
            n = int(rng.choice([0, 1, 7, 300, 5000, 40_000, C - 3, C, C + 2, 200_000]))
            if kind == 6:
                n = min(n, 5000)
            parts.append(corpus.chunk_corpus(kind, n, rng))
        offs = np.concatenate([[0], np.cumsum([q.size for q in parts])]).astype(np.int64)
        data = np.concatenate(parts)
        algo = (ADLER, CRC, 0, CRC32C)[round_]
        img, index, sums = lc.compress_map_output(LZF, algo, data, offs)
        check_image(lc, oracle, algo, data, offs, img, index, sums)
