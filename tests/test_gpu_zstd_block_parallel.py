"""GPU: block-independent Zstandard frames decoded one workgroup per block (S3S_OPT_ZSTD_DECODE_VARIANT = 1).
The frames of the library's own writer (S3S_OPT_ZSTD_COMPRESS = 1) must complete on the block path - S3S_OPT_ZSTD_DECODE_BLOCKS
counts their blocks exactly -, frames whose blocks lean on what lies in front of them must come out of the one-frame-per-
wavefront decoder, and whatever a call answers at variant 1 - bytes, return code, bad partition, batch statuses - is what the
same call answers at variant 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_block_parallel_lib as Z  # noqa: E402

pytestmark = pytest.mark.gpu

ZSTD = 3
ADLER, CRC = 1, 2
OPT_ZSTD_COMPRESS, OPT_VARIANT, OPT_BLOCKS = 9, 13, 14
B = Z.B
CANARY = 4096


@pytest.fixture()
def zc(gpu_codec):
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    gpu_codec.set_option(OPT_VARIANT, 1)
    try:
        yield gpu_codec
    finally:
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)
        gpu_codec.set_option(OPT_VARIANT, 1)
        gpu_codec.set_io_encryption(None)


def blocks_of(n):
    return -(-n // B) if n > B else 0  # (a frame of one block never enters the block path)


def image_of(parts, oracle=None, algo=0):
    """partitions (compressed bytes each) -> image, index, checksums"""
    index = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=index[1:])
    img = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    sums = np.array([oracle.checksum(algo, p) for p in parts], np.int64) if algo else None
    return img, index, sums


def both_variants(codec, call):
    """call() at variant 1 and at variant 0 -> ((result, key 14), (result, key 14))"""
    res = []
    for v in (1, 0):
        codec.set_option(OPT_VARIANT, v)
        assert codec.get_option(OPT_VARIANT) == v
        r = call()
        res.append((r, codec.get_option(OPT_BLOCKS)))
    codec.set_option(OPT_VARIANT, 1)
    return res


def test_the_keys(gpu_codec):
    lib, h = gpu_codec._lib, gpu_codec._h
    assert gpu_codec.get_option(OPT_VARIANT) == 1, "the block path is the default"
    assert lib.s3s_set_option(h, OPT_VARIANT, 2) == -1 and lib.s3s_set_option(h, OPT_VARIANT, -1) == -1
    assert lib.s3s_set_option(h, OPT_BLOCKS, 0) == -1 and lib.s3s_set_option(h, OPT_BLOCKS, 5) == -1, "key 14 is read-only"
    assert gpu_codec.get_option(OPT_VARIANT) == 1
    gpu_codec.set_option(OPT_VARIANT, 0)
    assert gpu_codec.get_option(OPT_VARIANT) == 0
    gpu_codec.set_option(OPT_VARIANT, 1)
    assert gpu_codec.zstd_decode_blocks == gpu_codec.get_option(OPT_BLOCKS) >= 0


# ---- 1. the writer's own images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b+1", "2b", "2b+1", "mixed"])
def test_writer_images(zc, oracle, name):
    src, n_blocks = Z.writer_sources()[name]
    # one partition
    offs = np.array([0, src.size], np.int64)
    img, index, sums = zc.compress_map_output(ZSTD, CRC, src, offs)
    assert np.array_equal(img, Z.writer_frame(name)), "the image is not the host build's frame"
    (out1, k1), (out0, k0) = both_variants(zc, lambda: zc.decompress_range(ZSTD, CRC, img, index, sums, dst_capacity=src.size).copy())
    assert np.array_equal(out1, src) and k1 == n_blocks
    assert np.array_equal(out0, src) and k0 == 0
    # five partitions with empty ones between them, other sizes around the block size
    cuts = [0, src.size - B - 1, src.size - B - 1, src.size - 1, src.size - 1, src.size] if src.size > 2 * B else \
        [0, 1, 1, src.size - 1, src.size - 1, src.size]
    offs = np.array(cuts, np.int64)
    want = sum(blocks_of(int(n)) for n in np.diff(offs))
    img, index, sums = zc.compress_map_output(ZSTD, ADLER, src, offs)
    (out1, k1), (out0, k0) = both_variants(zc, lambda: zc.decompress_range(ZSTD, ADLER, img, index, sums, dst_capacity=src.size).copy())
    assert np.array_equal(out1, src) and k1 == want
    assert np.array_equal(out0, src) and k0 == 0


# ---- 2. one range mixing frames ---------------------------------------------------------------------------------------------------
def _mixed_partitions():
    """[(compressed partition, content or None, blocks that complete on the block path)]"""
    from oracle import zstd_ref

    import zstd_conformance as C

    parts = [(Z.writer_frame("2b+1"), Z.writer_sources()["2b+1"][0], 3)]
    t = Z.text(200_000)
    parts.append((zstd_ref.compress_stream(t, 1), t, 0))
    for case in "abdf":
        frame, content, _ = Z.crafted(case)
        parts.append((frame, content, 0))
    bad = next(c for c in C.fixed_corpus() if c.name == "offset_one_beyond_the_history_invalid")
    C.arbiter(bad)
    parts.append((np.frombuffer(bad.data, np.uint8), None, 0))
    frame, content, independent = Z.crafted("c")
    assert independent
    parts.append((frame, content, len(Z.block_headers(frame))))
    return parts


def _device_call(codec, dev, ranges, algo, oracle, batch):
    """ranges: lists of (partition, content, blocks).  Decodes them as one batched device call (or as single device calls when
    batch is False) into destinations between canary bands.  -> [(status, out_len, bad partition, destination incl. canaries)]"""
    import s3shuffle

    args, dsts = [], []
    for parts in ranges:
        img, index, sums = image_of([p for p, _, _ in parts], oracle, algo)
        cap = sum(c.size for _, c, _ in parts if c is not None) + 300
        d = dev.upload(np.full(cap + 2 * CANARY, 0xA5, np.uint8))
        dsts.append((d, cap))
        args.append((dev.upload(img), img.size, index, sums, d + CANARY, cap))
    if batch:
        res = codec.decompress_ranges_batch_device(ZSTD, algo, args, raise_on_error=False)
    else:
        res = []
        for a in args:
            try:
                n = codec.decompress_range_device(ZSTD, algo, *a)
                res.append((0, n, -1))
            except s3shuffle.CodecError as e:
                res.append((e.code, 0, e.partition))
    return [(st, n, bad, dev.download(d, cap + 2 * CANARY)) for (st, n, bad), (d, cap) in zip(res, dsts)]


def _same_answers(r1, r0):
    assert len(r1) == len(r0)
    for (st1, n1, bad1, buf1), (st0, n0, bad0, buf0) in zip(r1, r0):
        assert (st1, n1, bad1) == (st0, n0, bad0), "the verdict depends on the variant"
        assert np.all(buf1[:CANARY] == 0xA5) and np.all(buf1[buf1.size - CANARY:] == 0xA5), "canary band damaged"
        if st1 == 0:
            assert np.array_equal(buf1[CANARY:CANARY + n1], buf0[CANARY:CANARY + n0]), "the bytes depend on the variant"
            assert np.all(buf1[CANARY + n1:] == 0xA5)


@pytest.mark.parametrize("algo", [0, CRC])
def test_mixed_range(gpu_codec, oracle, algo):
    from hipdev import Dev

    parts = _mixed_partitions()
    valid = [p for p in parts if p[1] is not None]
    want_blocks = sum(b for _, _, b in parts)
    assert want_blocks == 5
    dev = Dev()
    try:
        # everything in ONE range: the invalid frame is the range's verdict, at either variant
        (r1, k1), (r0, k0) = both_variants(gpu_codec, lambda: _device_call(gpu_codec, dev, [parts], algo, oracle, batch=False))
        _same_answers(r1, r0)
        assert r1[0][0] == -3 and (k1, k0) == (want_blocks, 0)
        # as a batch: the valid frames in one range, the invalid one in another
        ranges = [valid, [parts[6]]]
        (r1, k1), (r0, k0) = both_variants(gpu_codec, lambda: _device_call(gpu_codec, dev, ranges, algo, oracle, batch=True))
        _same_answers(r1, r0)
        assert [r[0] for r in r1] == [0, -3] and k0 == 0
        assert k1 == want_blocks, "key 14 counts the blocks of the frames in partitions that decoded, nothing else"
        content = np.concatenate([c for _, c, _ in valid])
        assert r1[0][1] == content.size and np.array_equal(r1[0][3][CANARY:CANARY + content.size], content)
    finally:
        dev.free()


# ---- 3. several frames in one partition ---------------------------------------------------------------------------------------------
def test_frames_in_one_partition(zc, oracle):
    from oracle import zstd_ref

    src = Z.writer_sources()["mixed"][0]
    segs = np.array([0, B + 1, B + 1, src.size], np.int64)   # partition 0 = two writer frames (and an empty piece between them)
    pfs = np.array([0, 3], np.int32)
    img, index, sums = zc.compress_map_output_segments(ZSTD, CRC, src, segs, pfs)
    (out1, k1), (out0, k0) = both_variants(zc, lambda: zc.decompress_range(ZSTD, CRC, img, index, sums, dst_capacity=src.size).copy())
    assert np.array_equal(out1, src) and np.array_equal(out0, src)
    assert (k1, k0) == (2 + blocks_of(src.size - B - 1), 0)
    # a writer frame behind a libzstd frame without a content size: its position is unknown before that frame is decoded
    t = Z.text(100_000)
    w, ws = Z.writer_frame("b+1"), Z.writer_sources()["b+1"][0]
    part = np.concatenate([zstd_ref.compress_stream(t, 1), w])
    idx = np.array([0, part.size], np.int64)
    (out1, k1), (out0, k0) = both_variants(zc, lambda: zc.decompress_range(ZSTD, 0, part, idx, None, dst_capacity=t.size + ws.size).copy())
    assert np.array_equal(out1, np.concatenate([t, ws])) and np.array_equal(out0, out1) and (k1, k0) == (0, 0)
    # ... and behind a libzstd frame that states its size (and is kept out by its window): judged on its own, on the block path
    lz, lsrc = Z.libzstd_frame()
    part = np.concatenate([lz, w])
    idx = np.array([0, part.size], np.int64)
    (out1, k1), (out0, k0) = both_variants(zc, lambda: zc.decompress_range(ZSTD, 0, part, idx, None, dst_capacity=lsrc.size + ws.size).copy())
    assert np.array_equal(out1, np.concatenate([lsrc, ws])) and np.array_equal(out0, out1) and (k1, k0) == (0, 0)


# ---- 4. every entry point ---------------------------------------------------------------------------------------------------------
def test_entry_points(zc, oracle):
    from hipdev import Dev

    names = ["2b+1", "b+1", "mixed"]
    srcs = [Z.writer_sources()[n][0] for n in names]
    imgs = [zc.compress_map_output(ZSTD, CRC, s, np.array([0, 1000, s.size], np.int64)) for s in srcs]
    want = [blocks_of(s.size - 1000) for s in srcs]
    # single, host buffers
    out = zc.decompress_range(ZSTD, CRC, *imgs[0], dst_capacity=srcs[0].size)
    assert np.array_equal(out, srcs[0]) and zc.zstd_decode_blocks == want[0]
    dev = Dev()
    try:
        args, outs = [], []
        for s, (img, index, sums) in zip(srcs, imgs):
            d_out = dev.upload(np.full(s.size + 16, 0xA5, np.uint8))
            outs.append(d_out)
            args.append((dev.upload(img), img.size, index, sums, d_out, s.size))
        # single, device buffers
        assert zc.decompress_range_device(ZSTD, CRC, *args[1]) == srcs[1].size and zc.zstd_decode_blocks == want[1]
        assert np.array_equal(dev.download(outs[1], srcs[1].size), srcs[1])
        dev.fill(outs[1], 0xA5, srcs[1].size)
        # batch of three, device buffers
        res = zc.decompress_ranges_batch_device(ZSTD, CRC, args)
        assert zc.zstd_decode_blocks == sum(want)
        for s, (st, n, bad), d_out in zip(srcs, res, outs):
            back = dev.download(d_out, s.size + 16)
            assert st == 0 and n == s.size and np.array_equal(back[:n], s) and np.all(back[n:] == 0xA5)
    finally:
        dev.free()
    # batch of three, host buffers: the call decodes group by group, the key reports its last decode
    keep = [np.ascontiguousarray(i[0]) for i in imgs]
    houts = [np.zeros(s.size, np.uint8) for s in srcs]
    res = zc.decompress_ranges_batch(ZSTD, CRC, [(k.ctypes.data, k.size, i[1], i[2], o.ctypes.data, o.size) for k, i, o in zip(keep, imgs, houts)])
    for s, (st, n, bad), o in zip(srcs, res, houts):
        assert st == 0 and n == s.size and np.array_equal(o, s)
    assert zc.zstd_decode_blocks in (sum(want), want[-1]), zc.zstd_decode_blocks
    # s3s_decompressed_size sizes, it does not decode: nothing completes on the block path
    assert zc.decompressed_size(ZSTD, imgs[0][0]) == srcs[0].size and zc.zstd_decode_blocks == 0


def test_under_io_encryption(zc, oracle):
    """The block path reads the decrypted workspace like the serial decoder does (128-bit key)."""
    src = Z.writer_sources()["2b+1"][0]
    offs = np.array([0, B + 5, B + 5, src.size], np.int64)
    ivs = np.arange(16 * 3, dtype=np.uint8)
    zc.set_io_encryption(bytes(range(16)))
    zc.set_stream_ivs(ivs)
    img, index, sums = zc.compress_map_output(ZSTD, ADLER, src, offs)
    assert bytes(img[:16]) == bytes(ivs[:16]) and bytes(img[16:20]) != b"\x28\xb5\x2f\xfd"
    (out1, k1), (out0, k0) = both_variants(zc, lambda: zc.decompress_range(ZSTD, ADLER, img, index, sums, dst_capacity=src.size).copy())
    assert np.array_equal(out1, src) and np.array_equal(out0, src)
    assert (k1, k0) == (2 + blocks_of(src.size - B - 5), 0)


# ---- 5. more blocks than resident workgroups ----------------------------------------------------------------------------------------
def test_more_blocks_than_resident_workgroups(zc):
    """One frame of 160 MiB = 1 280 blocks.  The block grid has the serial kernel's shape - 4 workgroups per compute unit, two
    blocks each: 2 048 blocks in flight on 256 compute units - so 1 280 blocks alone give no workgroup a second one; the second
    call below decodes two such frames (2 560 blocks), where 512 sequence wavefronts take a second block and their literal
    wavefronts run one hand-over ahead."""
    from hipdev import Dev
    from s3shuffle import datagen

    piece = datagen.terasort_map_output(8 << 20, 1, seed=11)[0]
    n = 160 << 20
    src = np.resize(piece, n)
    offs = np.array([0, n], np.int64)
    dev = Dev()
    try:
        cap = zc.max_compressed_size(ZSTD, offs)
        d_src, d_img, d_out = dev.upload(src), dev.alloc(cap + 16), dev.alloc(2 * n + 16)
        total, index, sums = zc.compress_map_output_device(ZSTD, CRC, d_src, offs, d_img, cap)
        assert zc.decompress_range_device(ZSTD, CRC, d_img, total, index, sums, d_out, n) == n
        assert zc.zstd_decode_blocks == 1280
        assert np.array_equal(dev.download(d_out, n), src)
        dev.fill(d_out, 0, 2 * n)
        res = zc.decompress_ranges_batch_device(ZSTD, CRC, [(d_img, total, index, sums, d_out, n), (d_img, total, index, sums, d_out + n, n)])
        assert [(st, m) for st, m, _ in res] == [(0, n), (0, n)] and zc.zstd_decode_blocks == 2560
        back = dev.download(d_out, 2 * n)
        assert np.array_equal(back[:n], src) and np.array_equal(back[n:], src)
    finally:
        dev.free()
