"""GPU: the streaming map side (s3s_cstream_*: a map output compressed window by window in bounded memory).

Every feed's answer is compared with the contract's Python model (cstream_units.py); the concatenated bytes, the lengths and
the checksums are compared with the one-shot device call on a second context with the same options."""
import numpy as np
import pytest

import cstream_units as cu
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, E_UNSUPPORTED = -1, -2, -6
OPT_LZ4_BS, OPT_SNAPPY_BS, OPT_LZ4_VARIANT, OPT_LZ4_VARIANT_USED, OPT_LZ4_BS_LARGE, OPT_LZF = 1, 2, 4, 7, 8, 10
CODEC_IDS = {NONE: "none", LZ4: "lz4", SNAPPY: "snappy", LZF: "lzf"}


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def ctxs():
    """pair(codec, bs) -> (stream context, reference context) with the same options; closed at teardown"""
    import s3shuffle

    made = []

    def pair(codec, bs=None, large=False, n=2):
        out = []
        for _ in range(n):
            c = s3shuffle.Codec(0)
            made.append(c)
            if codec == LZ4 and bs:
                c.set_option(OPT_LZ4_BS_LARGE if large else OPT_LZ4_BS, bs)
            if codec == SNAPPY and bs:
                c.set_option(OPT_SNAPPY_BS, bs)
            if codec == LZF:
                c.set_option(OPT_LZF, 1)
            out.append(c)
        return out

    yield pair
    for c in made:
        c.close()


def make_source(sizes, seed):
    """half compressible, half random (stored blocks), one run of zeros"""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    phrase = np.frombuffer(b"the quick brown fox jumps over the lazy dog; ", np.uint8)
    data = np.resize(phrase, total).copy()
    data[rng.integers(0, max(total, 1), total // 40)] = 7
    data[total // 2:] = rng.integers(0, 256, total - total // 2, dtype=np.uint8)
    data[total // 3: total // 3 + total // 10] = 0
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return data, offs


def one_shot(ref, dev, codec, algo, data, offs, d_src=None):
    d_src = dev.upload(data) if d_src is None else d_src
    cap = ref.max_compressed_size(codec, offs)
    d_dst = dev.alloc(cap + 64)
    total, index, sums = ref.compress_map_output_device(codec, algo, d_src, offs, d_dst, cap)
    img = dev.download(d_dst, total).copy()
    dev.release(d_dst)
    return img, index, sums


class Run:
    """One stream over one map output: every feed goes to the library and to the model, and the two must agree."""

    def __init__(self, ctx, dev, codec, algo, bs, data, offs, ref_img, ref_index, d_src=None, host=False, dst_bytes=None, d_dst=None):
        self.dev, self.codec, self.algo, self.data, self.offs, self.host = dev, codec, algo, data, offs, host
        self.model = cu.Model(codec, cu.block_size(codec, bs), cu.unit_sizes_from_image(codec, ref_img, ref_index))
        self.s = ctx.compress_stream(codec, algo)
        self.d_src = (dev.upload(data) if d_src is None else d_src) if not host else None
        self.dst_bytes = self.s.feed_bound(data.size, len(offs) - 1) + 64 if dst_bytes is None else dst_bytes
        self.d_dst = (dev.alloc(self.dst_bytes) if d_dst is None else d_dst) if not host else None
        self.h_dst = np.zeros(self.dst_bytes, np.uint8) if host else None
        self.out, self.lengths, self.sums, self.feeds = [], [], [], []

    def feed(self, pos, wlen, ends, cap):
        assert cap <= self.dst_bytes and self.s.position == pos
        before = self.s.written
        if self.host:
            r = self.s.feed(self.data[pos:pos + wlen], ends, self.h_dst, cap)
        else:
            r = self.s.feed_device(self.d_src + pos, wlen, ends, self.d_dst, cap)
        m = self.model.feed(wlen, ends, cap)
        got = cu.Feed(r.code, r.consumed, r.out_len, r.need_src, r.need_dst, r.parts_closed, [int(x) for x in r.lengths])
        assert got.fields() == m.fields(), (pos, wlen, list(ends), cap, got.fields(), m.fields())
        assert self.s.position == pos + r.consumed and self.s.written == before + r.out_len
        if r.out_len:
            self.out.append(self.h_dst[:r.out_len].copy() if self.host else self.dev.download(self.d_dst, r.out_len).copy())
        self.lengths += [int(x) for x in r.lengths]
        if self.algo:
            self.sums += [int(x) for x in r.checksums]
        self.feeds.append(got)
        return got

    def bound(self, step, wlen, n_ends):
        return self.s.feed_bound(wlen, n_ends)

    def finish(self, ref_img, ref_index, ref_sums):
        assert self.s.close() == 0
        img = np.concatenate(self.out) if self.out else np.zeros(0, np.uint8)
        assert img.size == ref_img.size and np.array_equal(img, ref_img)
        assert self.lengths == [int(x) for x in np.diff(ref_index)]
        if self.algo:
            assert self.sums == [int(x) for x in ref_sums]


def stream_equals_one_shot(ctx, dev, codec, algo, bs, data, offs, ref, window_of, cap_of=None, **kw):
    run = Run(ctx, dev, codec, algo, bs, data, offs, ref[0], ref[1], **kw)
    cu.drive(offs, run.feed, window_of, cap_of or run.bound)
    run.finish(*ref)
    return run


# ---- 1. codecs x checksums x schedules ----------------------------------------------------------------------------------------
SHAPE_BS = {NONE: 1024, LZ4: 1024, SNAPPY: 1024, LZF: 65535}


def shape_sizes(bs):
    return [0, 1, bs - 1, bs, bs + 1, 2 * bs, 3 * bs + 17, 0, 5]


def around_ends(offs, delta):
    marks = sorted({int(e) + delta for e in offs[1:] if 0 < int(e) + delta})
    return lambda step, pos: next((m for m in marks if m > pos), int(offs[-1])) - pos


@pytest.mark.parametrize("algo", [0, ADLER, CRC, CRC32C], ids=["nosum", "adler32", "crc32", "crc32c"])
@pytest.mark.parametrize("codec", [NONE, LZ4, SNAPPY, LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_codecs_and_schedules(ctxs, dev, codec, algo):
    bs = SHAPE_BS[codec]
    ctx, refc = ctxs(codec, bs)
    data, offs = make_source(shape_sizes(bs), 41 + codec)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, codec, algo, data, offs, d_src)
    total = data.size
    schedules = [lambda s, p: total, lambda s, p: bs, lambda s, p: bs + 1, lambda s, p: 3 * bs - 1] + [around_ends(offs, d) for d in (-1, 0, 1)]
    for window_of in schedules:
        run = stream_equals_one_shot(ctx, dev, codec, algo, bs, data, offs, ref, window_of, d_src=d_src)
        assert all(f.code == 0 for f in run.feeds)  # feed_bound never answers S3S_E_CAPACITY
        dev.release(run.d_dst)
    assert len(run.feeds) >= 6  # the last schedule stops behind every end that has bytes in front of it


# ---- 2. every cut position --------------------------------------------------------------------------------------------------
def test_every_cut_position_lz4(ctxs, dev):
    ctx, refc = ctxs(LZ4, 64)
    data, offs = make_source([130, 0, 64, 1, 200, 0, 205], 7)
    assert data.size == 600
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, LZ4, ADLER, data, offs, d_src)
    total = data.size
    shared = dict(d_src=d_src, d_dst=dev.alloc(4096), dst_bytes=4096)
    for w in range(total + 1):  # two feeds: the first window ends at every byte
        stream_equals_one_shot(ctx, dev, LZ4, ADLER, 64, data, offs, ref, lambda s, p, w=w: w if s == 0 else total, **shared)
    for w1 in range(0, total, 37):  # three feeds on a stride
        for w2 in range(1, total, 53):
            stream_equals_one_shot(ctx, dev, LZ4, ADLER, 64, data, offs, ref,
                                   lambda s, p, w1=w1, w2=w2: (w1, w2)[s] if s < 2 else total, **shared)


def test_cut_positions_snappy_1024(ctxs, dev):
    ctx, refc = ctxs(SNAPPY, 1024)
    data, offs = make_source([1024, 2048 + 5, 0, 1023, 3], 8)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, SNAPPY, CRC, data, offs, d_src)
    total = data.size
    cuts = sorted({c for k in range(1, 6) for c in (1024 * k - 1, 1024 * k, 1024 * k + 1)} | set(range(0, total, 97)) | {int(e) for e in offs})
    for w in (c for c in cuts if c <= total):
        run = stream_equals_one_shot(ctx, dev, SNAPPY, CRC, 1024, data, offs, ref, lambda s, p, w=w: w if s == 0 else total, d_src=d_src)
        dev.release(run.d_dst)


def test_cut_positions_lzf(ctxs, dev):
    ctx, refc = ctxs(LZF)
    data, offs = make_source([65535 + 10, 0, 2 * 65535, 3], 9)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, LZF, CRC32C, data, offs, d_src)
    total = data.size
    for w in (65534, 65535, 65536, 65535 + 9, 65535 + 10, 65535 + 11, 2 * 65535 + 9, 2 * 65535 + 10, 2 * 65535 + 11, total - 3, total - 1):
        run = stream_equals_one_shot(ctx, dev, LZF, CRC32C, 65535, data, offs, ref, lambda s, p, w=w: w if s == 0 else total, d_src=d_src)
        dev.release(run.d_dst)


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------
def test_capacity_first_unit_and_end_frame(ctxs, dev):
    ctx, refc = ctxs(LZ4, 64)
    data, offs = make_source([100, 64], 10)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, LZ4, ADLER, data, offs, d_src)
    sizes = cu.unit_sizes_from_image(LZ4, ref[0], ref[1])
    assert len(sizes[0]) == 3 and sizes[0][2] == 21
    run = Run(ctx, dev, LZ4, ADLER, 64, data, offs, ref[0], ref[1], d_src=d_src)
    ends = [100, 164]
    f = run.feed(0, 164, ends, sizes[0][0] - 1)  # one byte less than the first unit
    assert (f.code, f.need_dst, f.consumed, f.out_len, f.parts_closed) == (E_CAPACITY, sizes[0][0], 0, 0, 0)
    f = run.feed(0, 164, ends, sizes[0][0])  # exactly the first unit: the retry works and takes exactly it
    assert (f.code, f.consumed, f.out_len, f.parts_closed) == (0, 64, sizes[0][0], 0)
    f = run.feed(64, 100, [36, 100], sizes[0][1] + 20)  # the tail block fits, its end frame does not
    assert (f.code, f.consumed, f.out_len, f.parts_closed) == (0, 36, sizes[0][1], 0)
    f = run.feed(100, 0, [0], 64)  # an end at 0 in front of an open partition that has bytes: 21 bytes, closed
    assert (f.code, f.consumed, f.out_len, f.parts_closed) == (0, 0, 21, 1)
    f = run.feed(100, 64, [64], run.dst_bytes)
    assert (f.consumed, f.parts_closed) == (64, 1)
    run.finish(*ref)


def test_capacity_cut_inside_multi_fragment_snappy_chunk(ctxs, dev):
    bs = 128 << 10
    ctx, refc = ctxs(SNAPPY, bs)
    data, offs = make_source([300 * 1024 + 3], 11)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, SNAPPY, CRC, data, offs, d_src)
    sizes = cu.unit_sizes_from_image(SNAPPY, ref[0], ref[1])[0]
    assert len(sizes) == 3
    run = Run(ctx, dev, SNAPPY, CRC, bs, data, offs, ref[0], ref[1], d_src=d_src)
    f = run.feed(0, data.size, [data.size], sizes[0] + sizes[1] // 2)  # ends inside the second chunk, behind its first fragment
    assert (f.code, f.consumed, f.out_len, f.parts_closed) == (0, bs, sizes[0], 0)
    f = run.feed(bs, data.size - bs, [data.size - bs], sizes[1] + sizes[2] - 1)
    assert (f.code, f.consumed, f.out_len, f.parts_closed) == (0, bs, sizes[1], 0)
    f = run.feed(2 * bs, data.size - 2 * bs, [data.size - 2 * bs], sizes[2])
    assert (f.code, f.out_len, f.parts_closed) == (0, sizes[2], 1)
    run.finish(*ref)


@pytest.mark.parametrize("codec", [NONE, LZ4], ids=["none", "lz4"])
def test_capacities_cycling_through_small_primes(ctxs, dev, codec):
    ctx, refc = ctxs(codec, 64)
    data, offs = make_source([130, 0, 64, 1, 200, 0, 205], 12)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, codec, CRC, data, offs, d_src)
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 211, 307]
    for window in (data.size, 150):
        run = stream_equals_one_shot(ctx, dev, codec, CRC, 64, data, offs, ref, lambda s, p: window,
                                     lambda s, w, n: primes[s % len(primes)], d_src=d_src, dst_bytes=4096)
        if codec == LZ4:
            assert any(f.code == E_CAPACITY for f in run.feeds)  # the drive repeats those with need_dst
        dev.release(run.d_dst)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_feed_bound_holds_for_random_bytes(ctxs, dev, codec):
    """incompressible bytes in short partitions: the largest image a window of that shape can have"""
    bs = {LZ4: 64, SNAPPY: 1024, LZF: 65535}[codec]
    ctx, refc = ctxs(codec, bs)
    rng = np.random.default_rng(13)
    sizes = [1, 1, bs, 1, 2 * bs + 1, 1, 0, 1] if codec != LZF else [1, 1, bs + 1, 1]
    data = rng.integers(0, 256, sum(sizes), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, codec, ADLER, data, offs, d_src)
    for window in (data.size, bs, 1):
        run = stream_equals_one_shot(ctx, dev, codec, ADLER, bs, data, offs, ref, lambda s, p: window, d_src=d_src)
        assert all(f.code == 0 for f in run.feeds)
        dev.release(run.d_dst)


def test_guard_bytes_at_sixteen_alignments(ctxs, dev):
    ctx, refc = ctxs(LZ4, 64)
    data, offs = make_source([130, 0, 64, 1, 200], 14)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, LZ4, CRC, data, offs, d_src)
    sizes = [x for p in cu.unit_sizes_from_image(LZ4, ref[0], ref[1]) for x in p]
    cap = sum(sizes[:4]) + 5  # a cut in the middle of the plan: four units, then five bytes that must stay
    d_buf = dev.alloc(2048)
    for a in range(16):
        dev.fill(d_buf, 0xA5, 2048)
        with ctx.compress_stream(LZ4, CRC) as s:
            r = s.feed_device(d_src, data.size, offs[1:], d_buf + 64 + a, cap)
            assert r.code == 0 and r.out_len == sum(sizes[:4])
            got = dev.download(d_buf, 2048)
            assert np.all(got[:64 + a] == 0xA5) and np.all(got[64 + a + r.out_len:] == 0xA5), a
            assert np.array_equal(got[64 + a:64 + a + r.out_len], ref[0][:r.out_len])
            s.close(check=False)


# ---- 4. the tiles of the cut kernel -----------------------------------------------------------------------------------------
def test_cut_kernel_tiles(ctxs, dev):
    ctx, refc = ctxs(LZ4, 64)
    sizes = []
    for i in range(127):  # 127 non-empty partitions of 9 blocks each (10 units), 130 empty ones in runs: 257 ends, 1 270 units
        sizes.append(64 * 8 + 1 + i % 60)
        if i % 13 == 0:
            sizes += [0] * 13
    assert len(sizes) == 257 and sizes.count(0) == 130
    data, offs = make_source(sizes, 15)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, LZ4, ADLER, data, offs, d_src)
    assert sum(len(p) for p in cu.unit_sizes_from_image(LZ4, ref[0], ref[1])) >= 1025
    run = stream_equals_one_shot(ctx, dev, LZ4, ADLER, 64, data, offs, ref, lambda s, p: data.size, d_src=d_src)
    assert len(run.feeds) == 1
    # ... and cut in every tile of 256 items, and one unit in front of and behind a tile's edge
    img_total = ref[0].size
    for cap in (img_total * 3 // 10, img_total * 6 // 10, img_total - 1):
        run = stream_equals_one_shot(ctx, dev, LZ4, ADLER, 64, data, offs, ref, lambda s, p: data.size, lambda s, w, n: cap, d_src=d_src)
        assert len(run.feeds) > 1


def test_thousand_ends_at_zero(ctxs, dev):
    ctx = ctxs(LZ4, 64, n=1)[0]
    with ctx.compress_stream(LZ4, ADLER) as s:
        r = s.feed_device(0, 0, [0] * 1000, 0, 0)
        assert (r.code, r.consumed, r.out_len, r.parts_closed) == (0, 0, 0, 1000)
        assert list(r.lengths) == [0] * 1000 and list(r.checksums) == [1] * 1000  # a fresh Adler32
    with ctx.compress_stream(SNAPPY, CRC) as s:
        r = s.feed_device(0, 0, [0] * 1000, 0, 0)
        assert r.parts_closed == 1000 and list(r.lengths) == [0] * 1000 and list(r.checksums) == [0] * 1000
        r = s.feed_device(0, 0, [], 0, 0)  # an empty window with no ends
        assert (r.code, r.consumed, r.out_len, r.parts_closed, r.need_src) == (0, 0, 0, 0, 32768)


# ---- 5. large blocks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4-u32", "snappy-fragments"])
def test_large_blocks(ctxs, dev, codec):
    bs = 128 << 10
    ctx, refc = ctxs(codec, bs, large=True)
    data, offs = make_source([300 * 1024 + 3], 16)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, codec, ADLER, data, offs, d_src)
    run = stream_equals_one_shot(ctx, dev, codec, ADLER, bs, data, offs, ref, lambda s, p: 200 << 10, d_src=d_src)
    assert [f.consumed for f in run.feeds] == [bs, data.size - bs]  # the first window shows one whole block, the second the end
    with ctx.compress_stream(codec, ADLER) as s:
        r = s.feed_device(d_src, bs - 1, [], run.d_dst, 4096)
        assert (r.code, r.consumed, r.parts_closed, r.need_src) == (0, 0, 0, bs)


# ---- 6. the rest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,algo", [(LZ4, ADLER), (SNAPPY, CRC)], ids=["lz4-adler32", "snappy-crc32"])
def test_terasort_16mib_in_1mib_windows(ctxs, dev, codec, algo):
    from s3shuffle import datagen

    ctx, refc = ctxs(codec)
    data, offs = datagen.terasort_map_output(16 << 20, 200, seed=5, map_id=1)
    offs = np.asarray(offs, np.int64)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, codec, algo, data, offs, d_src)
    run = stream_equals_one_shot(ctx, dev, codec, algo, 32768, data, offs, ref, lambda s, p: 1 << 20, d_src=d_src,
                                 dst_bytes=ctx.compress_stream(codec, algo).feed_bound(1 << 20, 200) + 64)
    assert 16 <= len(run.feeds) <= 18
    if codec == LZ4:
        assert ctx.get_option(OPT_LZ4_VARIANT_USED) == 11


def test_other_calls_between_feeds_and_decode_back(ctxs, dev):
    """a one-shot compress and a decode on the SAME context between two feeds; the streamed image decodes back to the source
    through the streaming reduce side"""
    ctx, refc = ctxs(LZ4, 1024)
    data, offs = make_source(shape_sizes(1024), 17)
    d_src = dev.upload(data)
    ref = one_shot(refc, dev, LZ4, CRC, data, offs, d_src)
    run = Run(ctx, dev, LZ4, CRC, 1024, data, offs, ref[0], ref[1], d_src=d_src)

    def feed(pos, wlen, ends, cap):
        f = run.feed(pos, wlen, ends, cap)
        img, index, sums = one_shot(ctx, dev, LZ4, CRC, data, offs, d_src)  # the stream's own context
        assert np.array_equal(img, ref[0])
        d_img, d_back = dev.upload(img), dev.alloc(data.size)
        assert ctx.decompress_range_device(LZ4, CRC, d_img, img.size, index, sums, d_back, data.size) == data.size
        dev.release(d_img), dev.release(d_back)
        return f

    cu.drive(offs, feed, lambda s, p: 1500, run.bound)
    run.finish(*ref)
    img = np.concatenate(run.out)
    d_img, d_out = dev.upload(img), dev.alloc(4096)
    back = []
    with ctx.decode_stream(LZ4, CRC, ref[1], ref[2]) as ds:
        while True:
            r = ds.feed_device(d_img + ds.position, min(3000, img.size - ds.position), d_out, 4096)
            assert r.code == 0
            back.append(dev.download(d_out, r.out_len).copy())
            if r.at_end:
                break
            assert r.consumed > 0
    assert np.array_equal(np.concatenate(back), data)


@pytest.mark.parametrize("codec", [NONE, LZ4, SNAPPY, LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_host_buffer_feed(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    ctx, refc = ctxs(codec, bs)
    data, offs = make_source(shape_sizes(bs), 18)
    ref = one_shot(refc, dev, codec, CRC32C, data, offs)
    stream_equals_one_shot(ctx, dev, codec, CRC32C, bs, data, offs, ref, lambda s, p: 2 * bs + 7, host=True)


def test_refusals(ctxs, dev):
    import s3shuffle

    ctx = ctxs(LZ4, 64, n=1)[0]
    with pytest.raises(s3shuffle.CodecError) as e:
        ctx.compress_stream(ZSTD, 0)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(s3shuffle.CodecError) as e:
        ctx.compress_stream(LZF, 0)  # the option is off
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(s3shuffle.CodecError) as e:
        ctx.compress_stream(9, 0)
    assert e.value.code == E_INVALID
    ctx.set_io_encryption(bytes(range(16)))
    with pytest.raises(s3shuffle.CodecError) as e:
        ctx.compress_stream(LZ4, 0)  # a keyed context
    assert e.value.code == E_UNSUPPORTED
    ctx.set_io_encryption(None)
    data, offs = make_source([100, 64], 19)
    d_src, d_dst = dev.upload(data), dev.alloc(4096)
    s = ctx.compress_stream(LZ4, ADLER)
    ctx.set_io_encryption(bytes(range(16)))  # a key set after open
    with pytest.raises(s3shuffle.CodecError) as e:
        s.feed_device(d_src, 164, [100, 164], d_dst, 4096)
    assert e.value.code == E_UNSUPPORTED
    ctx.set_io_encryption(None)
    for ends in ([-1], [101, 100], [165], [100, 200]):  # negative, descending, beyond src_len
        with pytest.raises(s3shuffle.CodecError) as e:
            s.feed_device(d_src, 164, ends, d_dst, 4096)
        assert e.value.code == E_INVALID and s.position == 0 and s.written == 0
    for args in ((d_src, -1, [], d_dst, 16), (d_src, 16, [], d_dst, -1), (0, 16, [], d_dst, 16), (d_src, 164, [100], 0, 16)):
        with pytest.raises((s3shuffle.CodecError, ValueError)):
            s.feed_device(*args)
        assert s.position == 0 and s.written == 0
    assert s.close() == 0  # at a boundary: nothing of the open partition consumed
    s = ctx.compress_stream(LZ4, ADLER)
    r = s.feed_device(d_src, 64, [], d_dst, 4096)
    assert r.consumed == 64
    with pytest.raises(s3shuffle.CodecError) as e:
        s.close()  # inside a partition
    assert e.value.code == E_INVALID
    s = ctx.compress_stream(LZ4, ADLER)
    r = s.feed_device(d_src, 164, [100, 164], d_dst, 4096)
    assert (r.consumed, r.parts_closed) == (164, 2) and s.close() == 0


def test_lz4_variant_is_bound_at_open_and_auto_runs_11(ctxs, dev):
    ctx, refc = ctxs(LZ4, 1024)
    data, offs = make_source([3000, 0, 1024], 20)
    d_src = dev.upload(data)
    for variant, used in ((9, 11), (1, 1), (10, 10), (11, 11)):
        ctx.set_option(OPT_LZ4_VARIANT, variant)
        refc.set_option(OPT_LZ4_VARIANT, variant)
        ref = one_shot(refc, dev, LZ4, ADLER, data, offs, d_src)
        run = Run(ctx, dev, LZ4, ADLER, 1024, data, offs, ref[0], ref[1], d_src=d_src)
        ctx.set_option(OPT_LZ4_VARIANT, 1 if variant != 1 else 10)  # after open: the stream keeps what it was opened with
        cu.drive(offs, run.feed, lambda s, p: 2048, run.bound)
        assert ctx.get_option(OPT_LZ4_VARIANT_USED) == used
        run.finish(*ref)
        dev.release(run.d_dst)
