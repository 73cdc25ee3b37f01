"""GPU: Spark IO encryption (AES/CTR/NoPadding, s3s_set_io_encryption / s3s_set_stream_ivs) as a layer on both sides of the codec.

Map side: the expected image is tests/spark_crypto_ref.py (the layer restated on the host build of the same AES core, which
tests/test_aes_ctr_model.py holds against FIPS-197, SP 800-38A and libcrypto) applied to the library's OWN image with the layer
off, on the same context - bytes, index and all three checksums equal; for LZ4 and NONE also applied to the oracle's image.
Equal across the single, device, segments (a partition of three segments gets ONE IV), batch (one and three tasks) and
host-batch forms and across two consecutive calls.  Reduce side: every image decodes to its source under the right key in the
single, device, batch and host-batch forms and over sub-ranges; images built by the reference layer from oracle-written LZ4,
Snappy, zstd and LZF streams (the JVM-writer case) decode too.  Then the refusals.

Shapes (tests/io_encryption_inputs.py, properties asserted on the CPU in tests/test_aes_ctr_model.py): 20 partitions of words
text whose compressed starts have at least 8 residues mod 16, empties among them; codec NONE with partitions of 1 .. 70 000
bytes that end on and across the kernel's 16-byte units and 16 KiB tiles; keys of 16, 24 and 32 bytes; the IVs ff..ff and
00..00 ff..ff ff..f0, whose counters carry.  Images above 4 GiB with the layer on are NOT tested (the kernel's offsets and
block numbers are 64-bit throughout; unverified at that size)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import io_encryption_inputs as I  # noqa: E402
import spark_crypto_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
OPT_ZSTD_COMPRESS, OPT_LZF_COMPRESS, OPT_KEY_BITS = 9, 10, 11
E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, STATUS_NOT_RUN = -1, -2, -3, -4, -100
CODECS = [NONE, LZ4, SNAPPY, ZSTD, LZF]
NAMES = {NONE: "none", LZ4: "lz4", SNAPPY: "snappy", ZSTD: "zstd", LZF: "lzf"}


@pytest.fixture()
def ec(gpu_codec):
    """The shared context with both opt-in writers on; the layer is off again afterwards, whatever the test did."""
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    gpu_codec.set_option(OPT_LZF_COMPRESS, 1)
    try:
        yield gpu_codec
    finally:
        gpu_codec.set_io_encryption(None)
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)
        gpu_codec.set_option(OPT_LZF_COMPRESS, 0)


@pytest.fixture(scope="module")
def words():
    return I.words_input()


def plain(c, codec, algo, data, offs):
    c.set_io_encryption(None)
    return c.compress_map_output(codec, algo, data, offs)


def encrypted(c, key, ivs, codec, algo, data, offs):
    c.set_io_encryption(key)
    c.set_stream_ivs(ivs)
    return c.compress_map_output(codec, algo, data, offs)


def same(got, want, what=""):
    img, index, sums = got
    wimg, windex, wsums = want
    assert np.array_equal(index, windex), (what, index.tolist(), windex.tolist())
    assert img.size == wimg.size, what
    assert np.array_equal(img, wimg), "%s: first difference at byte %d" % (what, int(np.argmax(img != wimg)))
    if wsums is not None:
        assert np.array_equal(sums, wsums), what


# ---- map side -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", [16, 24, 32])
@pytest.mark.parametrize("codec", CODECS, ids=[NAMES[c] for c in CODECS])
def test_map_side_equals_the_reference_layer(ec, oracle, words, codec, kb):
    data, offs = words
    key, ivs = I.KEYS[kb], I.ivs_for(offs)
    for algo in (ADLER, CRC, CRC32C):
        p_img, p_index, _ = plain(ec, codec, algo, data, offs)
        want = R.encrypt_map_output(p_img, p_index, key, ivs, algo)
        got = encrypted(ec, key, ivs, codec, algo, data, offs)
        same(got, want, "%s key %d algo %d" % (NAMES[codec], kb, algo))
        assert ec.get_option(OPT_KEY_BITS) == 8 * kb
        if codec in (LZ4, NONE):  # ... and from the oracle's image
            o_img, o_index, _ = oracle.compress_map_output(codec, algo, data, offs)
            same(got, R.encrypt_map_output(o_img, o_index, key, ivs, algo), "oracle image")
        assert got[0].size <= ec.max_compressed_size(codec, offs)
    starts = {int(got[1][p]) % 16 for p in range(len(offs) - 1) if got[1][p + 1] > got[1][p]}
    if codec == LZ4:
        assert len(starts) >= 8, sorted(starts)
    for p in range(len(offs) - 1):  # an empty partition stays 0 bytes
        assert (got[1][p + 1] == got[1][p]) == (offs[p + 1] == offs[p])


@pytest.mark.parametrize("kb", [16, 24, 32])
def test_codec_none_partitions_on_and_across_the_tile_edges(ec, kb):
    data, offs = I.none_sizes_input()
    key, ivs = I.KEYS[kb], I.ivs_for(offs)
    want = R.encrypt_map_output(data, offs, key, ivs, CRC)
    same(encrypted(ec, key, ivs, NONE, CRC, data, offs), want)
    got = encrypted(ec, key, ivs, NONE, 0, data, offs)
    same(got, (want[0], want[1], None))
    back = ec.decompress_range(NONE, CRC, want[0], want[1], want[2], dst_capacity=data.size)
    assert np.array_equal(back, data)


def test_every_entry_point_gives_the_same_image(ec, words):
    from hipdev import Dev

    data, offs = words
    d2, o2 = I.none_sizes_input()
    d2, o2 = d2[:o2[11]], o2[:12]
    tasks = [(data, offs), (d2, o2), (data[:offs[8]], offs[:9])]
    key = I.KEYS[16]
    ivs = [I.ivs_for(o, seed=11 + t) for t, (_, o) in enumerate(tasks)]
    for codec in (LZ4, NONE, SNAPPY):
        want = []
        for (d, o), iv in zip(tasks, ivs):
            p_img, p_index, _ = plain(ec, codec, CRC, d, o)
            want.append(R.encrypt_map_output(p_img, p_index, key, iv, CRC))
        ec.set_io_encryption(key)
        for _ in range(2):  # two consecutive calls
            for (d, o), iv, w in zip(tasks, ivs, want):
                ec.set_stream_ivs(iv)
                same(ec.compress_map_output(codec, CRC, d, o), w, "single")
        dev = Dev()
        try:
            args, outs = [], []
            for (d, o), w in zip(tasks, want):
                cap = ec.max_compressed_size(codec, o)
                assert cap >= w[0].size
                d_out = dev.alloc(cap + 16)
                outs.append((d_out, cap))
                args.append((dev.upload(d), o, d_out, cap))
            ec.set_stream_ivs(np.concatenate(ivs))
            res = ec.compress_map_outputs_batch_device(codec, CRC, args)  # three tasks: the IVs task by task
            for (total, index, sums), (d_out, _), w in zip(res, outs, want):
                same((dev.download(d_out, total), index, sums), w, "batch of three")
            ec.set_stream_ivs(ivs[1])
            (total, index, sums), = ec.compress_map_outputs_batch_device(codec, CRC, args[1:2])  # a batch of one
            same((dev.download(outs[1][0], total), index, sums), want[1], "batch of one")
            ec.set_stream_ivs(ivs[0])
            total, index, sums = ec.compress_map_output_device(codec, CRC, args[0][0], tasks[0][1], outs[0][0], outs[0][1])
            same((dev.download(outs[0][0], total), index, sums), want[0], "device")
            import s3shuffle

            ec.set_stream_ivs(ivs[0])
            with pytest.raises(s3shuffle.CodecError) as ei:
                ec.compress_map_output_device(codec, CRC, args[0][0], tasks[0][1], outs[0][0], total - 1)
            assert ei.value.code == E_CAPACITY
        finally:
            dev.free()
        houts = [np.zeros(ec.max_compressed_size(codec, o), np.uint8) for _, o in tasks]
        ec.set_stream_ivs(np.concatenate(ivs))
        hres = ec.compress_map_outputs_batch(codec, CRC, [(d.ctypes.data, o, out.ctypes.data, out.size) for (d, o), out in zip(tasks, houts)])
        for (total, index, sums), out, w in zip(hres, houts, want):
            same((out[:total], index, sums), w, "host batch")


@pytest.mark.parametrize("codec", [LZ4, NONE, LZF], ids=["lz4", "none", "lzf"])
def test_a_partition_of_three_segments_gets_one_iv(ec, words, codec):
    data, _ = words
    data = data[:60000]
    segs = np.array([0, 20000, 20000, 20001, 46000, 60000, 60000], np.int64)
    pfs = np.array([0, 1, 4, 5, 6], np.int32)  # partition 1 = pieces 1 (empty), 2 (1 byte), 3; partition 3 = one empty piece
    key, ivs = I.KEYS[24], I.ivs_for(np.array([0, 20000, 46000, 60000, 60000]))
    ec.set_io_encryption(None)
    p_img, p_index, _ = ec.compress_map_output_segments(codec, ADLER, data, segs, pfs)
    want = R.encrypt_map_output(p_img, p_index, key, ivs, ADLER)
    assert want[1][-1] == p_index[-1] + 3 * 16  # three non-empty partitions, three IVs - not one per segment
    ec.set_io_encryption(key)
    ec.set_stream_ivs(ivs)
    same(ec.compress_map_output_segments(codec, ADLER, data, segs, pfs), want)
    back = ec.decompress_range(codec, ADLER, want[0], want[1], want[2], dst_capacity=data.size)
    assert np.array_equal(back, data)


def test_switching_the_layer_off_gives_the_plain_image_again(ec, words):
    data, offs = words
    before = plain(ec, LZ4, ADLER, data, offs)
    enc = encrypted(ec, I.KEYS[32], I.ivs_for(offs), LZ4, ADLER, data, offs)
    assert enc[0].size == before[0].size + 16 * int(np.sum(np.diff(offs) > 0))
    ec.set_io_encryption(None)
    assert ec.get_option(OPT_KEY_BITS) == 0
    same(ec.compress_map_output(LZ4, ADLER, data, offs), before)
    assert np.array_equal(ec.decompress_range(LZ4, ADLER, before[0], before[1], before[2], dst_capacity=data.size), data)


# ---- reduce side --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS, ids=[NAMES[c] for c in CODECS])
def test_every_image_decodes_to_its_source(ec, words, codec):
    from hipdev import Dev

    data, offs = words
    n = len(offs) - 1
    key = I.KEYS[16 if codec != SNAPPY else 32]
    img, index, sums = encrypted(ec, key, I.ivs_for(offs), codec, CRC32C, data, offs)
    assert np.array_equal(ec.decompress_range(codec, CRC32C, img, index, sums, dst_capacity=data.size), data)
    assert np.array_equal(ec.decompress_range(codec, CRC32C, img, index, sums), data)  # sized partition by partition
    assert np.array_equal(ec.decompress_range(codec, 0, img, index, None, dst_capacity=data.size + 100), data)
    ranges = [(0, n), (1, n - 1), (5, 8), (8, 10)]  # (8, 10): two empty partitions
    for r0, r1 in ranges:
        out = ec.decompress_range(codec, CRC32C, img[index[r0]:index[r1]], index[r0:r1 + 1] - index[r0], sums[r0:r1],
                                  dst_capacity=int(offs[r1] - offs[r0]))
        assert np.array_equal(out, data[offs[r0]:offs[r1]]), (r0, r1)
    for p in range(n):  # exact on ONE partition
        assert ec.decompressed_size(codec, img[index[p]:index[p + 1]]) == offs[p + 1] - offs[p]
    dev = Dev()
    try:
        d_img = dev.upload(img)
        d_out = dev.upload(np.full(data.size + 16, 0xA5, np.uint8))
        got = ec.decompress_range_device(codec, CRC32C, d_img, img.size, index, sums, d_out, data.size)
        back = dev.download(d_out, data.size + 16)
        assert got == data.size and np.array_equal(back[:got], data) and np.all(back[got:] == 0xA5)
        three = ranges[:3]
        d_back = [dev.upload(np.full(int(offs[r1] - offs[r0]) + 16, 0xA5, np.uint8)) for r0, r1 in three]
        res = ec.decompress_ranges_batch_device(codec, CRC32C, [
            (d_img + int(index[r0]), int(index[r1] - index[r0]), index[r0:r1 + 1] - index[r0], sums[r0:r1], d_b, int(offs[r1] - offs[r0]))
            for (r0, r1), d_b in zip(three, d_back)])
        for (st, nbytes, bad), (r0, r1), d_b in zip(res, three, d_back):
            back = dev.download(d_b, int(offs[r1] - offs[r0]) + 16)
            assert st == 0 and bad == -1 and nbytes == offs[r1] - offs[r0]
            assert np.array_equal(back[:nbytes], data[offs[r0]:offs[r1]]) and np.all(back[nbytes:] == 0xA5)
    finally:
        dev.free()
    pieces = [np.ascontiguousarray(img[index[r0]:index[r1]]) for r0, r1 in ranges[:3]]
    houts = [np.zeros(int(offs[r1] - offs[r0]) + 1, np.uint8) for r0, r1 in ranges[:3]]
    hres = ec.decompress_ranges_batch(codec, CRC32C, [
        (pc.ctypes.data, pc.size, index[r0:r1 + 1] - index[r0], sums[r0:r1], out.ctypes.data, out.size - 1)
        for pc, (r0, r1), out in zip(pieces, ranges[:3], houts)])
    for (st, nbytes, bad), (r0, r1), out in zip(hres, ranges[:3], houts):
        assert st == 0 and nbytes == offs[r1] - offs[r0] and np.array_equal(out[:nbytes], data[offs[r0]:offs[r1]])


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, ZSTD, LZF], ids=["lz4", "snappy", "zstd", "lzf"])
def test_jvm_written_encrypted_objects_decode(ec, oracle, words, codec):
    """Streams of another writer (the oracle's encoders, libzstd) under the reference layer: what a reduce task fetches from a
    cluster whose map side stayed on the JVM."""
    data, offs = words
    if codec == ZSTD:
        from oracle import zstd_ref

        p_img, p_index, _ = zstd_ref.compress_map_output(0, data, offs)
    else:
        p_img, p_index, _ = oracle.compress_map_output(codec, 0, data, offs)
    for kb in (16, 24, 32):
        img, index, sums = R.encrypt_map_output(p_img, p_index, I.KEYS[kb], I.ivs_for(offs, seed=kb), ADLER)
        ec.set_io_encryption(I.KEYS[kb])
        assert np.array_equal(ec.decompress_range(codec, ADLER, img, index, sums, dst_capacity=data.size), data)
        r0, r1 = 2, 13
        out = ec.decompress_range(codec, ADLER, img[index[r0]:index[r1]], index[r0:r1 + 1] - index[r0], sums[r0:r1],
                                  dst_capacity=int(offs[r1] - offs[r0]))
        assert np.array_equal(out, data[offs[r0]:offs[r1]])
        assert ec.decompressed_size(codec, img[index[7]:index[8]]) == offs[8] - offs[7]


def test_corruption_and_wrong_keys(ec, words):
    import s3shuffle

    data, offs = words
    key = I.KEYS[16]
    img, index, sums = encrypted(ec, key, I.ivs_for(offs), LZ4, CRC, data, offs)
    bad = img.copy()
    bad[index[6] + 16 + 100] ^= 0x40  # a cipher-text byte of partition 6
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.decompress_range(LZ4, CRC, bad, index, sums, dst_capacity=data.size)
    assert ei.value.code == E_CHECKSUM and ei.value.partition == 6
    bad = img.copy()
    bad[index[2] + 3] ^= 1  # an IV byte is stored data too
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.decompress_range(LZ4, CRC, bad, index, sums, dst_capacity=data.size)
    assert ei.value.code == E_CHECKSUM and ei.value.partition == 2
    # checksums off, another key: the LZ4Block magic decides (nothing else is claimed)
    ec.set_io_encryption(I.KEYS[24])
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.decompress_range(LZ4, 0, img, index, None, dst_capacity=data.size)
    assert ei.value.code == E_BAD_FRAME
    ec.set_io_encryption(key)
    # a stored partition of 7 bytes cannot hold an IV; one of exactly 16 is an empty stream
    seven = np.arange(7, dtype=np.uint8)
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.decompress_range(LZ4, 0, seven, [0, 7], None, dst_capacity=64)
    assert ei.value.code == E_BAD_FRAME
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.decompressed_size(LZ4, seven)
    assert ei.value.code == E_BAD_FRAME
    sixteen = np.arange(16, dtype=np.uint8)
    assert ec.decompress_range(LZ4, 0, sixteen, [0, 16], None, dst_capacity=64).size == 0
    assert ec.decompressed_size(LZ4, sixteen) == 0
    s = ec.checksum_ranges(ADLER, seven, [0, 7])
    with pytest.raises(s3shuffle.CodecError) as ei:  # ... and the checksum of the stored bytes still comes first
        ec.decompress_range(LZ4, ADLER, seven, [0, 7], s + 1, dst_capacity=64)
    assert ei.value.code == E_CHECKSUM and ei.value.partition == 0


# ---- refusals and answers ------------------------------------------------------------------------------------------------
def test_refusals_and_answers(ec, words):
    import s3shuffle
    from s3shuffle.codec import MapTask

    data, offs = words
    n = len(offs) - 1
    key, ivs = I.KEYS[16], I.ivs_for(offs)
    assert ec.get_option(OPT_KEY_BITS) == 0
    plain_bound = ec.max_compressed_size(LZ4, offs)
    for kb in (16, 24, 32):
        ec.set_io_encryption(I.KEYS[kb])
        assert ec.get_option(OPT_KEY_BITS) == 8 * kb
    ec.set_io_encryption(key)
    assert ec.get_option(OPT_KEY_BITS) == 128
    assert ec.max_compressed_size(LZ4, offs) == plain_bound + 16 * int(np.sum(np.diff(offs) > 0))
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.set_option(OPT_KEY_BITS, 128)
    assert ei.value.code == E_INVALID and ec.get_option(OPT_KEY_BITS) == 128
    secret = bytes(range(0x61, 0x61 + 17))
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.set_io_encryption(secret)
    assert ei.value.code == E_INVALID and "17" in str(ei.value)
    assert secret[:4].decode() not in str(ei.value) and secret.hex()[:8] not in str(ei.value)
    assert ec.get_option(OPT_KEY_BITS) == 128  # a refused key changes nothing
    for count in (n - 1, n + 1, 0):  # too few, too many, none at all
        ec.set_stream_ivs(ivs[:16 * count] if count <= n else np.concatenate([ivs, ivs[:16]]))
        with pytest.raises(s3shuffle.CodecError) as ei:
            ec.compress_map_output(LZ4, ADLER, data, offs)
        assert ei.value.code == E_INVALID
    want = encrypted(ec, key, ivs, LZ4, ADLER, data, offs)
    with pytest.raises(s3shuffle.CodecError) as ei:  # the call consumed them: a second call needs new IVs
        ec.compress_map_output(LZ4, ADLER, data, offs)
    assert ei.value.code == E_INVALID
    ec.set_stream_ivs(ivs[:16 * (n - 1)])  # a failed call consumes them too
    with pytest.raises(s3shuffle.CodecError):
        ec.compress_map_output(LZ4, ADLER, data, offs)
    with pytest.raises(s3shuffle.CodecError) as ei:
        ec.compress_map_output(LZ4, ADLER, data, offs)
    assert ei.value.code == E_INVALID and "no IVs" in str(ei.value)
    same(encrypted(ec, key, ivs, LZ4, ADLER, data, offs), want)
    # batch: a wrong count fails the call, every entry S3S_STATUS_NOT_RUN
    outs = [np.zeros(ec.max_compressed_size(LZ4, offs), np.uint8) for _ in range(2)]
    keep = []
    arr = (MapTask * 2)()
    for t in range(2):
        o = np.ascontiguousarray(offs, dtype=np.int64)
        idx, sm = np.zeros(n + 1, np.int64), np.zeros(n, np.int64)
        keep.append((o, idx, sm))
        arr[t].d_src = data.ctypes.data
        arr[t].src_offsets = o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        arr[t].num_partitions = n
        arr[t].d_dst = outs[t].ctypes.data
        arr[t].dst_capacity = outs[t].size
        arr[t].out_index = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        arr[t].out_checksums = sm.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        arr[t].status = 0
    ec.set_stream_ivs(ivs)  # n IVs for 2 n partitions
    assert ec._lib.s3s_compress_map_outputs_batch(ec._h, LZ4, ADLER, arr, 2) == E_INVALID
    assert [arr[t].status for t in range(2)] == [STATUS_NOT_RUN, STATUS_NOT_RUN]
    ec.set_stream_ivs(np.concatenate([ivs, ivs]))
    assert ec._lib.s3s_compress_map_outputs_batch(ec._h, LZ4, ADLER, arr, 2) == 0
    for t in range(2):
        assert arr[t].status == 0
        same((outs[t][:arr[t].out_total], keep[t][1], keep[t][2]), want)
