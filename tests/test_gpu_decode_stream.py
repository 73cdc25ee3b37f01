"""GPU: the streaming reduce side (s3s_dstream_*: a fetched range decoded window by window in bounded memory) and the seeded
checksums under it.  Images come from the oracle's writers (liblz4 for the 1 MiB blocks, the product's map side for the
multi-spill partitions, which the compress tests pin to the oracle); the truth is the source bytes and the one-shot call."""
import zlib

import numpy as np
import pytest

import corpus
import stream_units as su
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_UNSUPPORTED = -1, -2, -3, -4, -6
BLOCK = {NONE: 32768, LZ4: 32768, SNAPPY: 32768, LZF: 65535}  # decoded bytes of the largest unit the oracle's writers produce


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


def _code(exc_info):
    return exc_info.value.code


def _concat(parts):
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.uint8), offs


def run_stream(codec_ctx, dev, codec, algo, img, index, sums, window, cap, d_img=None, d_dst=None, max_feeds=100_000):
    """Feeds the range through a stream with windows of `window` bytes (grown to need_comp when told, back to `window` after a
    feed that consumed) and an output buffer of `cap` bytes -> (decoded bytes, feeds, growths, results)."""
    import s3shuffle

    total = int(index[-1])
    d_img = dev.upload(img) if d_img is None else d_img
    d_dst = dev.alloc(cap) if d_dst is None else d_dst
    out, results, feeds, growths, win = [], [], 0, 0, window
    with s3shuffle.DecodeStream(codec_ctx, codec, algo, index, sums if algo else None) as s:
        while True:
            pos = s.position
            w = min(win, total - pos)
            r = s.feed_device(d_img + pos, w, d_dst, cap)
            feeds += 1
            assert feeds <= max_feeds, "the stream makes no progress"
            assert r.code == 0, (r.code, r.need_dst, pos)
            assert s.position == pos + r.consumed and 0 <= r.consumed <= w and 0 <= r.out_len <= cap
            results.append((pos, w, r.consumed, r.out_len, r.need_comp, r.at_end))
            if r.out_len:
                out.append(dev.download(d_dst, r.out_len).copy())
            if r.at_end:
                assert s.position == total
                break
            if r.consumed == 0:
                assert r.need_comp > w, ("asked for no more than it had", pos, w, r.need_comp)
                win, growths = r.need_comp, growths + 1
            else:
                assert r.need_comp == 0
                win = window
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), feeds, growths, results


# ---- 1. equivalence ------------------------------------------------------------------------------------------------------
def _equivalence_source():
    rng = np.random.default_rng(1811)
    sizes = [0, 300_001, 1, 0, 400_003, 348_571, 0]  # empty first, middle and last, a 1-byte partition: ~1 MiB
    return _concat([corpus.chunk_corpus([7, 3, 0, 2, 7, 4, 5][p], n, rng) for p, n in enumerate(sizes)])


_EQ_SRC = {}


def _equivalence_image(oracle, codec, algo):
    if "src" not in _EQ_SRC:
        _EQ_SRC["src"] = _equivalence_source()
    data, offs = _EQ_SRC["src"]
    key = (codec, algo)
    if key not in _EQ_SRC:
        _EQ_SRC[key] = oracle.compress_map_output(codec, algo, data, offs)
    return (data, offs) + _EQ_SRC[key]


@pytest.mark.parametrize("algo", [0, ADLER, CRC, CRC32C], ids=["nosum", "adler32", "crc32", "crc32c"])
@pytest.mark.parametrize("codec", [NONE, LZ4, SNAPPY, LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_equivalence(gpu_codec, oracle, dev, codec, algo):
    data, offs, img, index, sums = _equivalence_image(oracle, codec, algo)
    total = int(index[-1])
    bs = BLOCK[codec]
    d_img = dev.upload(img)
    # the one-shot call on the same bytes
    d_one = dev.alloc(data.size)
    assert gpu_codec.decompress_range_device(codec, algo, d_img, total, index, sums, d_one, data.size) == data.size
    one_shot = dev.download(d_one, data.size)
    assert np.array_equal(one_shot, data)
    ulist = su.units(codec, img.tobytes(), index)
    # window x capacity pairs that cover every listed size once or more.  S3S_CODEC_NONE's units are bytes, so a window of
    # 1..22 bytes would be ~10^6 / window feeds on this image: here it takes the windows from 4099 up (the CPU check below
    # bounds every run), and test_equivalence_none_small_windows feeds the windows below on an image of 289 bytes
    windows = [1, 20, 21, 22, 4099, 65535, 65536, 65537, total]
    caps = [bs, bs + 1, 100_000, data.size + 4096]
    pairs = [(w, caps[i % 4]) for i, w in enumerate(windows)] + [(total, bs), (65536, 100_000), (4099, data.size + 4096)]
    if codec == NONE:
        pairs = [(w, c) for w, c in pairs if w >= 4099]
    d_dst = dev.alloc(max(caps))
    for window, cap in pairs:
        # CPU: a feed takes at least one unit (every unit decodes to <= bs <= cap) unless it grows the window, which a unit
        # needs at most three times (header, longer header, payload); S3S_CODEC_NONE takes min(window, cap) bytes per feed.
        # Finite, and small enough for a test
        assert max(u[2] for u in ulist) <= bs <= cap
        bound = 4 * len(ulist) + 2 if codec != NONE else -(-total // min(window, cap)) + 1
        assert bound < 1000, (window, cap, bound)
        out, feeds, growths, results = run_stream(gpu_codec, dev, codec, algo, img, index, sums, window, cap, d_img, d_dst, bound)
        assert np.array_equal(out, data), (window, cap)
        assert sum(r[2] for r in results) == total
        assert [r[5] for r in results].count(1) == 1 and results[-1][5] == 1  # at_end only at the end
        if codec != NONE:
            assert feeds <= len(ulist) + growths + 1, (window, cap, feeds, len(ulist), growths)
        # every feed took exactly the longest prefix of whole units that fits the window and the capacity
        for pos, w, consumed, out_len, _, _ in results:
            assert (consumed, out_len) == su.expected_feed(ulist, pos, w, cap) if codec != NONE else consumed == out_len == min(w, cap)


@pytest.mark.parametrize("algo", [0, ADLER, CRC, CRC32C], ids=["nosum", "adler32", "crc32", "crc32c"])
def test_equivalence_none_small_windows(gpu_codec, oracle, dev, algo):
    """S3S_CODEC_NONE through windows of 1, 20, 21 and 22 bytes: the same seven-partition shape (empty first, middle and last, a
    1-byte partition) at 289 bytes, so that a window of one byte is 289 feeds"""
    rng = np.random.default_rng(1812)
    data, offs = _concat([rng.integers(0, 256, n, dtype=np.uint8) for n in (0, 97, 1, 0, 130, 61, 0)])
    img, index, sums = oracle.compress_map_output(NONE, algo, data, offs)
    total = int(index[-1])
    assert total == data.size == 289
    d_img = dev.upload(img)
    d_one = dev.alloc(data.size)
    assert gpu_codec.decompress_range_device(NONE, algo, d_img, total, index, sums, d_one, data.size) == data.size
    assert np.array_equal(dev.download(d_one, data.size), data)
    d_dst = dev.alloc(4096)
    for window, cap in ((1, 4096), (20, 7), (21, 4096), (22, 21), (total, 1)):
        bound = -(-total // min(window, cap)) + 1
        out, feeds, growths, results = run_stream(gpu_codec, dev, NONE, algo, img, index, sums, window, cap, d_img, d_dst, bound)
        assert np.array_equal(out, data), (window, cap)
        assert sum(r[2] for r in results) == total and growths == 0
        assert [r[5] for r in results].count(1) == 1 and results[-1][5] == 1
        for pos, w, consumed, out_len, _, _ in results:
            assert consumed == out_len == min(w, cap)


def test_ring_decoder_variant_works(gpu_codec, oracle, dev):
    """S3S_OPT_LZ4_DECODE_VARIANT = 3 is not refused: a feed launches whichever decoder the option names."""
    default = gpu_codec.get_option(5)
    gpu_codec.set_option(5, 3)
    try:
        for codec in (LZ4, SNAPPY):
            data, offs, img, index, sums = _equivalence_image(oracle, codec, CRC)
            out, *_ = run_stream(gpu_codec, dev, codec, CRC, img, index, sums, 65537, 100_000)
            assert np.array_equal(out, data)
    finally:
        gpu_codec.set_option(5, default)


# ---- 2. every cut position ---------------------------------------------------------------------------------------------
def _two_feeds(gpu_codec, dev, codec, algo, img, index, sums, data, cuts):
    import s3shuffle

    total = int(index[-1])
    d_img = dev.upload(img)
    cap = data.size + 64
    d_dst = dev.alloc(cap)
    ulist = su.units(codec, img.tobytes(), index)
    for c in cuts:
        with s3shuffle.DecodeStream(gpu_codec, codec, algo, index, sums) as s:
            r1 = s.feed_device(d_img, c, d_dst, cap)
            assert r1.code == 0
            want = su.expected_feed(ulist, 0, c, cap)
            assert (r1.consumed, r1.out_len) == want, (c, r1.consumed, r1.out_len, want)
            a = dev.download(d_dst, r1.out_len).copy()
            if r1.consumed == 0:
                visible, ln, _ = su.unit_at(codec, img.tobytes(), 0, c, codec == SNAPPY)
                assert not visible and r1.need_comp == ln, (c, r1.need_comp, ln)
            r2 = s.feed_device(d_img + r1.consumed, total - r1.consumed, d_dst, cap)
            assert r2.code == 0 and r2.consumed == total - r1.consumed and r2.at_end == 1, (c, r2.consumed, r2.at_end)
            b = dev.download(d_dst, r2.out_len)
            assert np.array_equal(np.concatenate([a, b]), data), c


def test_every_cut_position_lz4(gpu_codec, oracle, dev):
    """two partitions, three frames each, 4 KiB blocks: cuts inside the magic, each length field, a byte short of a frame, on a
    frame end, inside an end frame, on the partition boundary"""
    rng = np.random.default_rng(5)
    data, offs = _concat([corpus.chunk_corpus(3, 3 * 4096 - 100, rng), corpus.chunk_corpus(7, 2 * 4096 + 9, rng)])
    img, index, sums = oracle.compress_map_output(LZ4, ADLER, data, offs, 4096)
    assert len(su.units(LZ4, img.tobytes(), index)) == 8 and img.size < 12_000
    _two_feeds(gpu_codec, dev, LZ4, ADLER, img, index, sums, data, range(1, img.size))


def test_every_cut_position_snappy(gpu_codec, oracle, dev):
    rng = np.random.default_rng(6)
    data, offs = _concat([corpus.chunk_corpus(3, 2 * 4096 + 5, rng), corpus.chunk_corpus(7, 4096 + 900, rng)])
    img, index, sums = oracle.compress_map_output(SNAPPY, CRC, data, offs, 4096)
    assert img.size < 10_000
    _two_feeds(gpu_codec, dev, SNAPPY, CRC, img, index, sums, data, range(1, img.size))


def test_every_cut_position_lzf(gpu_codec, oracle, dev):
    """both chunk header shapes: a stored chunk (5 bytes) and compressed ones (7); a chunk holds up to 65535 source bytes, so
    the partition of two chunks is made of words and a short period, which LZF packs into a few KiB"""
    data, offs, img, index, sums = su.lzf_cut_image(oracle, CRC32C)
    _two_feeds(gpu_codec, dev, LZF, CRC32C, img, index, sums, data, range(1, img.size))


@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4", "snappy"])
def test_multi_spill_partition(gpu_codec, oracle, dev, codec):
    """concatenated streams inside one partition: the stream boundary inside a window and at a window's edge"""
    rng = np.random.default_rng(8)
    segs = [corpus.chunk_corpus(7, 40_000, rng), corpus.chunk_corpus(3, 50_000, rng), corpus.chunk_corpus(7, 9_000, rng)]
    data, seg_offs = _concat(segs)
    img, index, sums = gpu_codec.compress_map_output_segments(codec, CRC, data, seg_offs, [0, 2, 3])
    boundary = oracle.compress_stream(codec, segs[0]).size  # where the second stream of partition 0 starts
    assert np.array_equal(img[:boundary], oracle.compress_stream(codec, segs[0]))
    _two_feeds(gpu_codec, dev, codec, CRC, img, index, sums, data, [boundary - 1, boundary, boundary + 1, boundary + 5, boundary + 16, boundary + 21])
    for window in (boundary, boundary + 7):
        out, *_ = run_stream(gpu_codec, dev, codec, CRC, img, index, sums, window, 65_536)
        assert np.array_equal(out, data)


# ---- 3. need_comp is exact enough ---------------------------------------------------------------------------------------
def test_need_comp_two_steps_on_1mib_blocks(gpu_codec, dev):
    import lz4_u32_ref as R
    import s3shuffle
    from s3shuffle import datagen

    parts = [datagen.terasort_map_output((2 << 20) + 12_345, 1, seed=3)[0], np.random.default_rng(9).integers(0, 256, (1 << 20) + 7, dtype=np.uint8)]
    img, index, sums = R.expected_map_output(parts, 1 << 20, CRC)
    img, index, sums = np.frombuffer(img, np.uint8), np.array(index, np.int64), np.array(sums, np.int64)
    data = np.concatenate(parts)
    total = int(index[-1])
    d_img, cap = dev.upload(img), (1 << 20) + 64
    d_dst = dev.alloc(cap)
    out, big = [], 0
    with s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, index, sums) as s:
        while True:
            pos = s.position
            w = min(65536, total - pos)
            r = s.feed_device(d_img + pos, w, d_dst, cap)
            steps = 0
            while r.consumed == 0 and not r.at_end:
                assert r.code == 0 and r.need_comp > w
                w, steps = r.need_comp, steps + 1  # a window of exactly need_comp bytes: takes a unit, or asks for strictly more
                assert steps <= 2, "header, then header + payload"
                r = s.feed_device(d_img + pos, w, d_dst, cap)
            big += steps > 0
            if r.out_len:
                out.append(dev.download(d_dst, r.out_len).copy())
            if r.at_end:
                break
    assert big >= 3  # the frames above 64 KiB were met
    assert np.array_equal(np.concatenate(out), data)


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------
def test_capacity(gpu_codec, oracle, dev):
    import s3shuffle

    data, offs, img, index, sums = _equivalence_image(oracle, LZ4, ADLER)
    ulist = su.units(LZ4, img.tobytes(), index)
    first = ulist[0][2]
    assert first == 32768
    d_img = dev.upload(img)
    d_dst = dev.alloc(first + 256)
    dev.fill(d_dst, 0xA5, first + 256)
    with s3shuffle.DecodeStream(gpu_codec, LZ4, ADLER, index, sums) as s:
        r = s.feed_device(d_img, 100_000, d_dst, first - 1)
        assert (r.code, r.need_dst, r.consumed, r.out_len, s.position) == (E_CAPACITY, first, 0, 0, 0)
        assert np.all(dev.download(d_dst, first + 256) == 0xA5)
        r = s.feed_device(d_img, 100_000, d_dst, r.need_dst)
        assert (r.code, r.consumed, r.out_len) == (0, ulist[0][1], first)
        got = dev.download(d_dst, first + 256)
        assert np.array_equal(got[:first], data[:first]) and np.all(got[first:] == 0xA5)  # nothing written behind out_len
        with pytest.raises(s3shuffle.CodecError) as e:  # a window that reaches past the end of the range
            s.feed_device(d_img, int(index[-1]) - s.position + 1, d_dst, first)
        assert _code(e) == E_INVALID
        s.close(check=False)
    # S3S_CODEC_NONE: units are bytes, so a capacity of 0 is the only one that cannot take the first unit
    with s3shuffle.DecodeStream(gpu_codec, NONE, 0, [0, 10]) as s:
        r = s.feed_device(d_img, 10, 0, 0)
        assert (r.code, r.need_dst, s.position) == (E_CAPACITY, 1, 0)
        s.close(check=False)


# ---- 5. checksum timing -----------------------------------------------------------------------------------------------------
def _literal_image(oracle, codec, algo):
    """three partitions (a short one, one of 250 000 incompressible bytes that the codec stores as literals, a short one) plus an
    empty one: a flipped byte deep inside a literal run leaves every frame well-formed"""
    rng = np.random.default_rng(12)
    data, offs = _concat([corpus.chunk_corpus(7, 5_000, rng), corpus.chunk_corpus(0, 250_000, rng), np.zeros(0, np.uint8),
                          corpus.chunk_corpus(7, 3_000, rng)])
    return (data, offs) + oracle.compress_map_output(codec, algo, data, offs)


def _raw_feed(s, d_comp, comp_len, d_dst, cap):
    """s3s_dstream_feed_device through ctypes -> (return code, the C result): what a failing feed leaves in the struct"""
    import ctypes

    import s3shuffle

    res = s3shuffle.codec.StreamResult()
    rc = s._lib.s3s_dstream_feed_device(s._s, ctypes.c_void_p(d_comp), comp_len, ctypes.c_void_p(d_dst), cap, ctypes.byref(res))
    return int(rc), res


def _timing_case(oracle, codec, algo, flip_in_feed):
    """-> (the image with one byte flipped in partition 1, where the first two windows end, the rest of the case)"""
    data, offs, img, index, sums = _literal_image(oracle, codec, algo)
    total = int(index[-1])
    # partition 1 spans three feeds: windows end at a third and two thirds of it, then the rest of the range
    p0, p1 = int(index[1]), int(index[2])
    cuts = [p0 + (p1 - p0) // 3, p0 + 2 * (p1 - p0) // 3, total]
    bad = img.copy()
    at = (p0 + 1000) if flip_in_feed == 0 else (cuts[1] + (p1 - cuts[1]) // 2)
    if codec != NONE:  # the middle of the unit that holds `at`: inside its literal run, far from any header
        at = next(u[0] + u[1] // 2 for u in su.units(codec, img.tobytes(), index) if u[0] <= at < u[0] + u[1] and u[1] > 1000)
    assert (p0 < at < cuts[0]) if flip_in_feed == 0 else (cuts[1] < at < p1)
    bad[at] ^= 0x40
    return bad, cuts, data, index, sums


# LZ4Block frames carry a hash of their own decoded bytes, so a flipped byte in a feed IN FRONT of the completing one is a
# corrupt frame to that feed (test_lz4_corrupt_frame_in_an_open_partition); in the completing feed the verdict comes first
@pytest.mark.parametrize("algo", [ADLER, CRC, CRC32C], ids=["adler32", "crc32", "crc32c"])
@pytest.mark.parametrize("codec,flip_in_feed", [(NONE, 0), (NONE, 2), (SNAPPY, 0), (SNAPPY, 2), (LZ4, 2)],
                         ids=["none-0", "none-2", "snappy-0", "snappy-2", "lz4-2"])
def test_checksum_timing(gpu_codec, oracle, dev, codec, algo, flip_in_feed):
    import s3shuffle

    bad, cuts, data, index, sums = _timing_case(oracle, codec, algo, flip_in_feed)
    total, p1 = int(index[-1]), int(index[2])
    d_img = dev.upload(bad)
    cap = data.size + 64
    d_dst = dev.alloc(cap)
    s = s3shuffle.DecodeStream(gpu_codec, codec, algo, index, sums)
    for k in range(2):  # the feeds in front of the partition's last byte return OK, flipped byte and all
        pos = s.position
        r = s.feed_device(d_img + pos, cuts[k] - pos, d_dst, cap)
        assert r.code == 0 and r.consumed > 0 and r.out_len > 0, k
        assert s.position <= cuts[k] < p1
    pos = s.position
    dev.fill(d_dst, 0xA5, cap)
    for _ in range(2):  # the completing feed, and every later one: the C result, then nothing moved and nothing decoded
        rc, res = _raw_feed(s, d_img + pos, total - pos, d_dst, cap)
        assert (rc, res.bad_partition, res.consumed, res.out_len, res.at_end) == (E_CHECKSUM, 1, 0, 0, 0)
        assert s.position == pos
    assert np.all(dev.download(d_dst, cap) == 0xA5)  # the verdict came before the decode was launched
    with pytest.raises(s3shuffle.CodecError) as e:  # the binding raises it, with the partition
        s.feed_device(d_img + pos, total - pos, d_dst, cap)
    assert _code(e) == E_CHECKSUM and e.value.partition == 1
    assert s.close(check=False) == E_CHECKSUM
    # the one-shot call on the same bytes: the same class, the same partition
    with pytest.raises(s3shuffle.CodecError) as e:
        gpu_codec.decompress_range_device(codec, algo, d_img, total, index, sums, d_dst, cap)
    assert _code(e) == E_CHECKSUM and e.value.partition == 1


def test_lz4_corrupt_frame_in_an_open_partition(gpu_codec, oracle, dev):
    """the documented difference: a flipped byte in a feed in front of the partition's end fails that frame's own hash, so the
    stream reports S3S_E_BAD_FRAME there and keeps it, where the one-shot call reports the partition's checksum first"""
    import s3shuffle

    bad, cuts, data, index, sums = _timing_case(oracle, LZ4, CRC, 0)
    total = int(index[-1])
    d_img = dev.upload(bad)
    cap = data.size + 64
    d_dst = dev.alloc(cap)
    s = s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, index, sums)
    for _ in range(2):
        rc, res = _raw_feed(s, d_img, cuts[0], d_dst, cap)
        assert (rc, res.consumed, res.out_len, res.at_end, s.position) == (E_BAD_FRAME, 0, 0, 0, 0)
    assert s.close(check=False) == E_BAD_FRAME
    with pytest.raises(s3shuffle.CodecError) as e:
        gpu_codec.decompress_range_device(LZ4, CRC, d_img, total, index, sums, d_dst, cap)
    assert _code(e) == E_CHECKSUM and e.value.partition == 1


def test_checksum_result_fields_and_empty_partition(gpu_codec, oracle, dev):
    import s3shuffle

    data, offs, img, index, sums = _literal_image(oracle, SNAPPY, CRC)
    total = int(index[-1])
    d_img = dev.upload(img)
    cap = data.size + 64
    d_dst = dev.alloc(cap)
    # the C result of a failing feed: consumed = out_len = 0, bad_partition set
    lib = gpu_codec._lib
    wrong = sums.copy()
    wrong[2] ^= 1  # the EMPTY partition's reference value
    s = s3shuffle.DecodeStream(gpu_codec, SNAPPY, CRC, index, wrong)
    r = s.feed_device(d_img, int(index[2]) - 10, d_dst, cap)  # stops short of the empty partition: OK
    assert r.code == 0 and s.position < int(index[2])
    pos = s.position
    res = s3shuffle.codec.StreamResult()
    import ctypes
    rc = lib.s3s_dstream_feed_device(s._s, ctypes.c_void_p(d_img + pos), total - pos, ctypes.c_void_p(d_dst), cap, ctypes.byref(res))
    assert (rc, res.bad_partition, res.consumed, res.out_len, res.at_end) == (E_CHECKSUM, 2, 0, 0, 0)  # reported as the position passes it
    assert s.close(check=False) == E_CHECKSUM
    # an empty FIRST partition with a wrong value: reported by the first feed, whatever its window
    data2, offs2, img2, index2, sums2 = _equivalence_image(oracle, LZ4, ADLER)
    wrong2 = sums2.copy()
    wrong2[0] = 7
    s = s3shuffle.DecodeStream(gpu_codec, LZ4, ADLER, index2, wrong2)
    with pytest.raises(s3shuffle.CodecError) as e:
        s.feed_device(dev.upload(img2[:21]), 21, d_dst, cap)
    assert _code(e) == E_CHECKSUM and e.value.partition == 0
    s.close(check=False)


# ---- 6. seeded checksums ----------------------------------------------------------------------------------------------------
def _truth(oracle, algo, b):
    return zlib.adler32(b) if algo == ADLER else zlib.crc32(b) if algo == CRC else oracle.crc32c(np.frombuffer(b, np.uint8))


@pytest.mark.parametrize("algo", [ADLER, CRC, CRC32C], ids=["adler32", "crc32", "crc32c"])
def test_seeded_checksums(gpu_codec, oracle, dev, algo):
    rng = np.random.default_rng(40 + algo)
    n = 200 * 1024
    buf = rng.integers(0, 256, n, dtype=np.uint8)
    d = dev.upload(buf)
    want = _truth(oracle, algo, buf.tobytes())
    fresh = 1 if algo == ADLER else 0
    for split in (0, 1, 16383, 16384, 16385, 100_000, n):
        a = gpu_codec.checksum_ranges_seeded_device(algo, d, [0, split], [fresh])[0]
        assert a == _truth(oracle, algo, buf[:split].tobytes())
        b = gpu_codec.checksum_ranges_seeded_device(algo, d + split, [0, n - split], [a])[0]
        assert b == want, split
    # many pieces chained, zero-length ones included; one call with several seeded ranges
    cuts = [0, 0, 1, 16383, 16384, 16384, 16385, 100_000, n, n]
    state = fresh
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        state = int(gpu_codec.checksum_ranges_seeded_device(algo, d, [lo, hi], [state])[0])
    assert state == want
    assert list(gpu_codec.checksum_ranges_seeded_device(algo, d, [5, 5, 5], [12345, want])) == [12345, want]  # no bytes: the seed
    # seeds = NULL is s3s_checksum_ranges_device
    offs = [0, 1, 16385, 100_000, n]
    assert np.array_equal(gpu_codec.checksum_ranges_seeded_device(algo, d, offs, None), gpu_codec.checksum_ranges_device(algo, d, offs))
    # the host-buffer form
    assert gpu_codec.checksum_ranges_seeded(algo, buf, [0, 100_000, n], [fresh, 0])[0] == _truth(oracle, algo, buf[:100_000].tobytes())
    # a piece longer than one fold group of the kernel (ranges above 32 MiB are folded in groups of 4 MiB): 33 MiB + 5 behind a seed
    big = np.resize(buf, (33 << 20) + 5 + 70_000)
    d_big = dev.upload(big)
    a = gpu_codec.checksum_ranges_seeded_device(algo, d_big, [0, 70_000], [fresh])[0]
    b = gpu_codec.checksum_ranges_seeded_device(algo, d_big, [70_000, big.size], [a])[0]
    assert b == _truth(oracle, algo, big.tobytes())


# ---- 7. verdict parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_verdict_parity(gpu_codec, oracle, dev, codec):
    import s3shuffle

    rng = np.random.default_rng(70 + codec)
    data, offs = _concat([corpus.chunk_corpus(7, 100_000, rng), corpus.chunk_corpus(3, 150_000, rng)])
    img, index, _ = oracle.compress_map_output(codec, 0, data, offs)
    cap = data.size + 64
    d_dst = dev.alloc(cap)

    def one_shot(b, idx):
        with pytest.raises(s3shuffle.CodecError) as e:
            gpu_codec.decompress_range_device(codec, 0, dev.upload(b), b.size, idx, None, d_dst, cap)
        return _code(e)

    def stream(b, idx, window):
        d = dev.upload(b)
        s = s3shuffle.DecodeStream(gpu_codec, codec, 0, idx)
        with pytest.raises(s3shuffle.CodecError) as e:
            for _ in range(100):
                pos = s.position
                r = s.feed_device(d + pos, min(window, b.size - pos), d_dst, cap)
                assert r.code == 0 and r.consumed > 0 and not r.at_end
        with pytest.raises(s3shuffle.CodecError) as e2:  # the error sticks
            s.feed_device(d + s.position, 1, d_dst, cap)
        assert _code(e2) == _code(e) == s.close(check=False)
        return _code(e)

    # truncated: the last frame is cut and the window ends at the end of the (shortened) range
    cutoff = int(index[-1]) - 30
    trunc, tidx = img[:cutoff].copy(), np.array([0, index[1], cutoff], np.int64)
    assert stream(trunc, tidx, 65536) == E_BAD_FRAME == one_shot(trunc, tidx)
    # a corrupt magic / chunk header in the middle of a window
    ulist = su.units(codec, img.tobytes(), index)
    victim = ulist[len(ulist) // 2][0]
    broken = img.copy()
    broken[victim + (2 if codec != SNAPPY else 0)] ^= 0xFF  # LZ4 'L Z [4]', LZF 'Z V [type]', Snappy: the length's top byte
    assert stream(broken, index, int(index[-1])) == E_BAD_FRAME == one_shot(broken, index)
    # closed before the end
    s = s3shuffle.DecodeStream(gpu_codec, codec, 0, index)
    r = s.feed_device(dev.upload(img), int(index[-1]) // 2, d_dst, cap)
    assert r.code == 0 and 0 < r.consumed < int(index[-1])
    with pytest.raises(s3shuffle.CodecError) as e:
        s.close()
    assert _code(e) == E_BAD_FRAME


# ---- 8. refusals and coexistence ------------------------------------------------------------------------------------------
def test_refusals_and_coexistence(gpu_codec, oracle, dev):
    import s3shuffle

    data, offs, img, index, sums = _equivalence_image(oracle, LZ4, CRC)

    def one_shot_ok():
        assert np.array_equal(gpu_codec.decompress_range(LZ4, CRC, img, index, sums), data)

    with pytest.raises(s3shuffle.CodecError) as e:
        s3shuffle.DecodeStream(gpu_codec, ZSTD, CRC, index, sums)
    assert _code(e) == E_UNSUPPORTED
    one_shot_ok()
    gpu_codec.set_io_encryption(bytes(range(16)))
    try:
        with pytest.raises(s3shuffle.CodecError) as e:
            s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, index, sums)
        assert _code(e) == E_UNSUPPORTED
    finally:
        gpu_codec.set_io_encryption(None)
    one_shot_ok()
    # a one-shot decode of ANOTHER image between two feeds: the stream's result does not change
    other = _equivalence_image(oracle, SNAPPY, ADLER)
    d_img, cap = dev.upload(img), 100_000
    d_dst = dev.alloc(cap)
    out = []
    with s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, index, sums) as s:
        while True:
            pos = s.position
            r = s.feed_device(d_img + pos, min(70_001, int(index[-1]) - pos), d_dst, cap)
            assert r.code == 0
            out.append(dev.download(d_dst, r.out_len).copy())
            assert np.array_equal(gpu_codec.decompress_range(SNAPPY, ADLER, other[2], other[3], other[4]), other[0])
            if r.at_end:
                break
    assert np.array_equal(np.concatenate(out), data)


# ---- 9. bounded memory at size -------------------------------------------------------------------------------------------
_BIG = {}


def _big_image(oracle, codec):
    from s3shuffle import datagen

    if "src" not in _BIG:
        data, offs = datagen.terasort_map_output(64 << 20, 1, seed=5)
        _BIG["src"] = (data, offs, zlib.crc32(data))
    if codec not in _BIG:
        _BIG[codec] = oracle.compress_map_output(codec, CRC, _BIG["src"][0], _BIG["src"][1])
    return _BIG["src"] + _BIG[codec]


@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4", "snappy"])
def test_bounded_memory_64mib_partition(gpu_codec, oracle, dev, codec):
    import s3shuffle

    data, offs, want_crc, img, index, sums = _big_image(oracle, codec)
    total = int(index[-1])
    window, cap = 4 << 20, 8 << 20
    d_img = dev.upload(img)
    d_dst = dev.alloc(cap)  # reused by every feed
    crc, n_out, feeds = 0, 0, 0
    with s3shuffle.DecodeStream(gpu_codec, codec, CRC, index, sums) as s:
        while True:
            pos = s.position
            r = s.feed_device(d_img + pos, min(window, total - pos), d_dst, cap)
            feeds += 1
            assert r.code == 0 and r.consumed > 0 and r.out_len <= cap
            crc = zlib.crc32(dev.download(d_dst, r.out_len), crc)
            n_out += r.out_len
            if r.at_end:
                break
    assert (n_out, crc) == (data.size, want_crc)
    assert feeds <= total // (window // 2) + data.size // (cap // 2) + 2


def test_bounded_memory_host_buffers(gpu_codec, oracle):
    """the host-buffer form once over the 64 MiB partition: the same windows, one reused 8 MiB destination"""
    import s3shuffle

    data, offs, want_crc, img, index, sums = _big_image(oracle, LZ4)
    total = int(index[-1])
    dst = np.empty(8 << 20, np.uint8)
    crc, n_out = 0, 0
    with gpu_codec.decode_stream(LZ4, CRC, index, sums) as s:
        while True:
            pos = s.position
            r = s.feed(img[pos:min(pos + (4 << 20), total)], dst)
            assert r.code == 0 and r.consumed > 0
            crc = zlib.crc32(dst[:r.out_len], crc)
            n_out += r.out_len
            if r.at_end:
                break
    assert (n_out, crc) == (data.size, want_crc)
