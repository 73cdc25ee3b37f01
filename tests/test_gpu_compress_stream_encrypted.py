"""GPU: the streaming map side under IO encryption (s3s_cstream_open_encrypted).

Every feed's answer is compared with the contract's Python model (cstream_units_encrypted.py); the concatenated bytes, the
lengths and the checksums are compared with the one-shot encrypted call on a second context (same options, key, IVs) and with
spark_crypto_ref.encrypt_map_output applied to the PLAIN one-shot image of a third, unkeyed context - an independent reference.
dst is prefilled before every feed and must be unchanged from out_len to the buffer's end behind it.  The shapes are small on
purpose (LZF, whose block is 65 535 bytes, gets partitions of up to 3 blocks where the others get up to 20)."""
import numpy as np
import pytest

import aes_ctr_model_lib as acm
import cstream_units as cu
import cstream_units_encrypted as cue
import spark_crypto_ref as scr
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, E_UNSUPPORTED = -1, -2, -6
OPT_LZ4_BS, OPT_SNAPPY_BS, OPT_LZF = 1, 2, 10
PREFILL = 0xA5
KEYS = {n: bytes((7 * i + n) & 0xFF for i in range(n)) for n in (16, 24, 32)}


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def ctxs():
    """trio(codec, bs, key) -> (stream context, one-shot context, both under the key; an unkeyed context), same options"""
    import s3shuffle

    made = []

    def trio(codec, bs=None, key=KEYS[16]):
        out = []
        for i in range(3):
            c = s3shuffle.Codec(0)
            made.append(c)
            if codec == LZ4 and bs:
                c.set_option(OPT_LZ4_BS, bs)
            if codec == SNAPPY and bs:
                c.set_option(OPT_SNAPPY_BS, bs)
            if codec == LZF:
                c.set_option(OPT_LZF, 1)
            if i < 2 and key is not None:
                c.set_io_encryption(key)
            out.append(c)
        return out

    yield trio
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


def make_ivs(nparts, seed):
    return np.random.default_rng(1000 + seed).integers(0, 256, (nparts, 16), dtype=np.uint8)


def one_shot(c, dev, codec, algo, offs, d_src, ivs=None):
    cap = c.max_compressed_size(codec, offs)
    d_dst = dev.alloc(cap + 64)
    if ivs is not None:
        c.set_stream_ivs(ivs.reshape(-1))
    total, index, sums = c.compress_map_output_device(codec, algo, d_src, offs, d_dst, cap)
    img = dev.download(d_dst, total).copy()
    dev.release(d_dst)
    return img, np.asarray(index, np.int64), sums


class Ref:
    """The references of one map output: the plain one-shot image (unit sizes), the encrypted one-shot call, and
    spark_crypto_ref over the plain image - the last two must agree before any stream is held against them."""

    def __init__(self, refc, plainc, dev, codec, algo, data, offs, key, ivs, d_src):
        self.plain_img, self.plain_index, _ = one_shot(plainc, dev, codec, 0, offs, d_src)
        self.img, self.index, self.sums = one_shot(refc, dev, codec, algo, offs, d_src, ivs)
        want_img, want_index, want_sums = scr.encrypt_map_output(self.plain_img, self.plain_index, key, ivs.reshape(-1), algo or None)
        assert np.array_equal(self.img, want_img) and [int(x) for x in self.index] == [int(x) for x in want_index]
        assert cue.stored_index(self.plain_index) == [int(x) for x in self.index]
        if algo:
            assert [int(x) for x in self.sums] == [int(x) for x in want_sums]
        self.spark_img = want_img
        self.sizes = cue.unit_sizes_from_plain_image(codec, self.plain_img, self.plain_index)


class Run:
    """One encrypted stream over one map output: every feed goes to the library and to the model, and the two must agree."""

    def __init__(self, ctx, dev, codec, algo, bs, data, offs, ref, ivs, d_src=None, host=False, dst_bytes=None, other_iv0=False):
        self.ctx, self.dev, self.codec, self.algo, self.data, self.offs, self.host = ctx, dev, codec, algo, data, offs, host
        self.ivs, self.other_iv0 = ivs, other_iv0
        self.model = cue.Model(codec, cu.block_size(codec, bs), ref.sizes)
        self.s = ctx.compress_stream(codec, algo, encrypted=True)
        self.d_src = (dev.upload(data) if d_src is None else d_src) if not host else None
        self.dst_bytes = self.s.feed_bound(data.size, len(offs) - 1) + 64 if dst_bytes is None else dst_bytes
        self.d_dst = dev.alloc(self.dst_bytes) if not host else None
        self.h_dst = np.zeros(self.dst_bytes, np.uint8) if host else None
        self.out, self.lengths, self.sums, self.feeds, self.fronts = [], [], [], [], []

    def feed_ivs(self, n_ends):
        """entry j: the IV of the partition piece j belongs to (a piece behind the last partition: zeros, never used)"""
        first = self.model.n_closed
        a = np.zeros((n_ends + 1, 16), np.uint8)
        for j in range(n_ends + 1):
            if first + j < len(self.ivs):
                a[j] = self.ivs[first + j]
        if self.other_iv0 and self.model.open_img > 0:  # entry 0 is ignored while the open partition has image bytes
            a[0] ^= 0x5A
        return a

    def feed(self, pos, wlen, ends, cap):
        assert cap <= self.dst_bytes and self.s.position == pos
        before = self.s.written
        self.fronts.append(self.model.open_img)
        self.ctx.set_stream_ivs(self.feed_ivs(len(ends)).reshape(-1))
        if self.host:
            self.h_dst[:] = PREFILL
            r = self.s.feed(self.data[pos:pos + wlen], ends, self.h_dst, cap)
        else:
            self.dev.fill(self.d_dst, PREFILL, self.dst_bytes)
            r = self.s.feed_device(self.d_src + pos, wlen, ends, self.d_dst, cap)
        assert self.s.feed_bound(wlen, len(ends)) == cue.feed_bound(self.codec, self.model.bs, wlen, len(ends))
        m = self.model.feed(wlen, ends, cap)
        got = cu.Feed(r.code, r.consumed, r.out_len, r.need_src, r.need_dst, r.parts_closed, [int(x) for x in r.lengths])
        assert got.fields() == m.fields(), (pos, wlen, list(ends), cap, got.fields(), m.fields())
        assert self.s.position == pos + r.consumed and self.s.written == before + r.out_len
        whole = self.h_dst if self.host else self.dev.download(self.d_dst, self.dst_bytes)
        assert np.all(whole[r.out_len:self.dst_bytes] == PREFILL), (pos, wlen, cap, r.out_len)  # nothing at or beyond out_len
        if r.out_len:
            self.out.append(whole[:r.out_len].copy())
        self.lengths += [int(x) for x in r.lengths]
        if self.algo:
            self.sums += [int(x) for x in r.checksums]
        self.feeds.append(got)
        return got

    def bound(self, step, wlen, n_ends):
        return self.s.feed_bound(wlen, n_ends)

    def image(self):
        return np.concatenate(self.out) if self.out else np.zeros(0, np.uint8)

    def finish(self, ref):
        assert self.s.close() == 0
        img = self.image()
        assert img.size == ref.img.size and np.array_equal(img, ref.img)
        assert np.array_equal(img, ref.spark_img)
        assert self.lengths == [int(x) for x in np.diff(ref.index)]
        if self.algo:
            assert self.sums == [int(x) for x in ref.sums]
        if self.d_dst is not None:
            self.dev.release(self.d_dst)


def stream_equals_one_shot(ctx, dev, codec, algo, bs, data, offs, ref, ivs, window_of, cap_of=None, **kw):
    run = Run(ctx, dev, codec, algo, bs, data, offs, ref, ivs, **kw)
    cu.drive(offs, run.feed, window_of, cap_of or run.bound)
    run.finish(ref)
    return run


# ---- 1. codecs x checksums x schedules ----------------------------------------------------------------------------------------
SHAPE_BS = {NONE: 1024, LZ4: 1024, SNAPPY: 1024, LZF: 65535}
KEY_OF_ALGO = {0: 16, ADLER: 24, CRC: 32, CRC32C: 16}  # every key size at least once per codec


def shape_sizes(codec):
    bs = SHAPE_BS[codec]
    if codec == LZF:
        return [0, 1, bs - 1, 0, bs, bs + 1, 0, 3 * bs + 17, 5, 2 * bs, 0]
    return [0, 1, bs - 1, bs, bs + 1, 0, 20 * bs + 17, 5 * bs, 0, 3 * bs + 1, 7 * bs - 1, 2 * bs, 0]


def schedules(bs, total, seed):
    rng = np.random.default_rng(seed)
    rand = [int(x) for x in rng.integers(1, 6 * bs, 4096)]
    return [lambda s, p: total, lambda s, p: bs + 5, lambda s, p: 3 * bs + 5, lambda s, p: 7 * bs + 5, lambda s, p: rand[s % len(rand)]]


@pytest.mark.parametrize("algo", [0, ADLER, CRC, CRC32C], ids=["nosum", "adler32", "crc32", "crc32c"])
@pytest.mark.parametrize("codec", [NONE, LZ4, SNAPPY, LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_codecs_checksums_schedules(ctxs, dev, codec, algo):
    bs = SHAPE_BS[codec]
    key = KEYS[KEY_OF_ALGO[algo]]
    ctx, refc, plainc = ctxs(codec, bs, key)
    data, offs = make_source(shape_sizes(codec), 41 + codec)
    ivs = make_ivs(len(offs) - 1, codec)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, codec, algo, data, offs, key, ivs, d_src)
    for window_of in schedules(bs, data.size, 50 + codec):
        run = stream_equals_one_shot(ctx, dev, codec, algo, bs, data, offs, ref, ivs, window_of, d_src=d_src)
        assert all(f.code == 0 for f in run.feeds)  # feed_bound never answers S3S_E_CAPACITY


# ---- 2. every cut position ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [NONE, LZ4, SNAPPY], ids=["none", "lz4", "snappy"])
def test_every_cut_position(ctxs, dev, codec):
    bs = {NONE: 64, LZ4: 64, SNAPPY: 1024}[codec]
    ctx, refc, plainc = ctxs(codec, bs, KEYS[32])
    data, offs = make_source([10, 40 * bs + 30, 7] if codec != NONE else [10, 90, 7], 7)
    ivs = make_ivs(3, 2)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, codec, ADLER, data, offs, KEYS[32], ivs, d_src)
    flat = [x for p in ref.sizes for x in p]
    if codec == LZ4:
        assert len(ref.sizes[1]) == 42 and ref.sizes[1][-1] == 21  # 41 blocks and the end frame
    total, unit_bs = data.size, cu.block_size(codec, bs)
    for i, c in enumerate(int(x) for x in np.cumsum(flat)[:-1]):  # the cut behind every unit in turn (LZ4: between a tail block and its end frame too)
        for cap in (c, c + min(15, flat[i + 1] - 1)):  # ... exactly, and short of the next unit
            run = stream_equals_one_shot(ctx, dev, codec, ADLER, bs, data, offs, ref, ivs, lambda s, p: total,
                                         lambda s, w, n, cap=cap: cap if s == 0 else cue.feed_bound(codec, unit_bs, w, n), d_src=d_src)
            assert run.feeds[0].out_len == c
    run = Run(ctx, dev, codec, ADLER, bs, data, offs, ref, ivs, d_src=d_src)
    f = run.feed(0, total, [int(e) for e in offs[1:]], flat[0] - 1)  # one byte below the first unit: need_dst includes the 16
    plain_first = cu.unit_sizes_from_image(codec, ref.plain_img, ref.plain_index)[0][0]
    assert (f.code, f.need_dst, f.consumed, f.out_len, f.parts_closed) == (E_CAPACITY, plain_first + 16, 0, 0, 0)
    f = run.feed(0, total, [int(e) for e in offs[1:]], flat[0])
    assert (f.code, f.out_len) == (0, flat[0])
    run.s.close(check=False)


# ---- 3. every key stream residue ----------------------------------------------------------------------------------------------
def test_every_key_stream_residue_lz4_stored_blocks(ctxs, dev):
    ctx, refc, plainc = ctxs(LZ4, 64, KEYS[24])
    data = np.random.default_rng(3).integers(0, 256, 64 * 18, dtype=np.uint8)
    offs = np.array([0, data.size], np.int64)
    ivs = make_ivs(1, 3)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, LZ4, CRC, data, offs, KEYS[24], ivs, d_src)
    assert ref.sizes[0][:18] == [16 + 85] + [85] * 17  # stored blocks
    run = stream_equals_one_shot(ctx, dev, LZ4, CRC, 64, data, offs, ref, ivs, lambda s, p: 64 if s < 17 else data.size, d_src=d_src)
    assert run.fronts[:18] == [0] + [16 + 85 * k for k in range(1, 18)]
    assert {f % 16 for f in run.fronts[1:17]} == set(range(16))  # a condition on the inputs: every residue of front mod 16 occurred


def test_every_key_stream_residue_none(ctxs, dev):
    ctx, refc, plainc = ctxs(NONE, None, KEYS[16])
    lens = list(range(1, 34))
    data, offs = make_source([sum(lens) - 40, 40], 4)
    ivs = make_ivs(2, 4)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, NONE, ADLER, data, offs, KEYS[16], ivs, d_src)
    run = stream_equals_one_shot(ctx, dev, NONE, ADLER, 1, data, offs, ref, ivs, lambda s, p: lens[s] if s < len(lens) else data.size, d_src=d_src)
    assert len(run.feeds) >= 33 and {f % 16 for f in run.fronts if f} == set(range(16))


# ---- 4. tile boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [1, 2], ids=["first-tile", "second-tile"])
@pytest.mark.parametrize("lead", [0, 5], ids=["aligned", "front-residue"])
def test_partition_starts_around_a_tile_end(ctxs, dev, tile, lead):
    """NONE: a partition's stored start at 16 384 tile - k, k = 0 .. 16, relative to the workgroup tiles of the feed that writes
    it: an IV that straddles the tile's end.  lead = 5: a first feed of 5 bytes makes front = 21, the tiles start 5 bytes in
    front of the second feed's output."""
    ctx, refc, plainc = ctxs(NONE, None, KEYS[16])
    src = np.random.default_rng(9).integers(0, 256, 16384 * tile + 64, dtype=np.uint8)
    d_all = dev.upload(src)
    ivs = make_ivs(2, 5)
    for k in range(17):
        start = 16384 * tile - k - (lead & 15)  # where partition 1's IV starts in the output of the feed that writes it
        size0 = start - 16 if lead == 0 else start + lead
        data, offs = src[:size0 + 40], np.array([0, size0, size0 + 40], np.int64)
        ref = Ref(refc, plainc, dev, NONE, CRC32C, data, offs, KEYS[16], ivs, d_all)
        run = stream_equals_one_shot(ctx, dev, NONE, CRC32C, 1, data, offs, ref, ivs, lambda s, p: lead if (lead and s == 0) else data.size,
                                     d_src=d_all)
        assert run.fronts[-1] == (16 + lead if lead else 0)
        assert run.feeds[-1].out_len - 56 == start  # the last feed's output: partition 0's rest, then IV + 40 bytes


# ---- 5. many pieces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [NONE, SNAPPY, LZ4], ids=["none", "snappy", "lz4"])
def test_257_ends_of_one_byte_partitions_under_a_small_capacity(ctxs, dev, codec):
    bs = {NONE: None, SNAPPY: 1024, LZ4: 64}[codec]
    ctx, refc, plainc = ctxs(codec, bs, KEYS[16])
    data, offs = make_source([1] * 257, 21)
    ivs = make_ivs(257, 6)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, codec, CRC, data, offs, KEYS[16], ivs, d_src)
    assert ref.sizes[0] == {NONE: [17], SNAPPY: [16 + int(ref.plain_index[1])], LZ4: [16 + 21 + 1, 21]}[codec]  # 16 + header + 1
    cap = 5 * sum(ref.sizes[0]) + 3  # five partitions a feed: every other piece lies behind the cut with length 0
    run = stream_equals_one_shot(ctx, dev, codec, CRC, bs or 1, data, offs, ref, ivs, lambda s, p: data.size, lambda s, w, n: cap, d_src=d_src,
                                 dst_bytes=1 << 16)
    assert len(run.feeds) >= 51 and run.feeds[0].parts_closed == 5


# ---- 6. alignment -----------------------------------------------------------------------------------------------------------------
def test_guard_bytes_at_sixteen_alignments(ctxs, dev):
    ctx, refc, plainc = ctxs(LZ4, 64, KEYS[32])
    data, offs = make_source([130, 0, 64, 1, 200], 14)
    ivs = make_ivs(5, 7)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, LZ4, CRC, data, offs, KEYS[32], ivs, d_src)
    flat = [x for p in ref.sizes for x in p]
    cap = sum(flat[:4]) + 5  # a cut in the middle of the plan: four units, then five bytes that must stay
    d_buf = dev.alloc(2048)
    for a in range(16):
        dev.fill(d_buf, PREFILL, 2048)
        with ctx.compress_stream(LZ4, CRC, encrypted=True) as s:
            ctx.set_stream_ivs(np.concatenate([ivs, np.zeros((1, 16), np.uint8)]).reshape(-1))
            r = s.feed_device(d_src, data.size, offs[1:], d_buf + 64 + a, cap)
            assert r.code == 0 and r.out_len == sum(flat[:4])
            got = dev.download(d_buf, 2048)
            assert np.all(got[:64 + a] == PREFILL) and np.all(got[64 + a + r.out_len:] == PREFILL), a
            assert np.array_equal(got[64 + a:64 + a + r.out_len], ref.img[:r.out_len])
            s.close(check=False)


# ---- 7. host buffers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [NONE, LZ4, SNAPPY, LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_host_buffer_feed(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    ctx, refc, plainc = ctxs(codec, bs, KEYS[24])
    data, offs = make_source(shape_sizes(codec), 18)
    ivs = make_ivs(len(offs) - 1, 8)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, codec, CRC32C, data, offs, KEYS[24], ivs, d_src)
    stream_equals_one_shot(ctx, dev, codec, CRC32C, bs, data, offs, ref, ivs, lambda s, p: 2 * bs + 7, host=True)


# ---- 8. beyond 2^32 inside one partition ------------------------------------------------------------------------------------------
def test_one_partition_beyond_4gib(ctxs, dev):
    """NONE, no checksum, one partition of 4 GiB + 1 MiB fed as the same 64 MiB device buffer again and again: the key stream's
    block number and the stream's front pass 2^32 stored bytes inside feed 63."""
    ctx = ctxs(NONE, None, KEYS[16])[0]
    W, TAIL = 64 << 20, 1 << 20
    buf = np.random.default_rng(11).integers(0, 256, W, dtype=np.uint8)
    d_src, d_dst = dev.upload(buf), dev.alloc(W + 64)
    iv = make_ivs(1, 9)
    probe = 4096

    def expect(plain_off, src_off, n):
        return acm.xor_stream(KEYS[16], iv[0].tobytes(), buf[src_off:src_off + n], offset=plain_off)

    with ctx.compress_stream(NONE, 0, encrypted=True) as s:
        for k in range(65):
            last = k == 64
            ctx.set_stream_ivs(np.concatenate([iv, iv]).reshape(-1) if last else iv.reshape(-1))
            r = s.feed_device(d_src, TAIL if last else W, [TAIL] if last else [], d_dst, W + 16)
            lead = 16 if k == 0 else 0
            assert (r.code, r.consumed, r.out_len, r.parts_closed) == (0, TAIL if last else W, (TAIL if last else W) + lead, int(last))
            if k == 0:
                got = dev.download(d_dst, 16 + probe)
                assert np.array_equal(got[:16], iv[0]) and np.array_equal(got[16:], expect(0, 0, probe))
            if k == 63:  # stored offset 2^32 = plain offset 2^32 - 16: the last 16 bytes of this window's output
                assert s.written == 16 + 64 * W and s.written - 16 == (1 << 32)
                got = dev.download(d_dst + W - probe, probe)
                assert np.array_equal(got, expect(64 * W - probe, W - probe, probe))
            if k == 64:
                got = dev.download(d_dst, TAIL)
                assert np.array_equal(got, expect(64 * W, 0, TAIL))
                assert [int(x) for x in r.lengths] == [(4 << 30) + TAIL + 16]
        assert s.written == (4 << 30) + TAIL + 16 and s.position == (4 << 30) + TAIL


# ---- 9. round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4", "snappy"])
def test_round_trip_through_both_reduce_sides(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    ctx, refc, plainc = ctxs(codec, bs, KEYS[32])
    data, offs = make_source(shape_sizes(codec), 41 + codec)
    ivs = make_ivs(len(offs) - 1, codec)
    d_src = dev.upload(data)
    ref = Ref(refc, plainc, dev, codec, CRC, data, offs, KEYS[32], ivs, d_src)
    # (entry 0 of every feed that finds its partition open is another IV: it is ignored, the bytes still match)
    run = stream_equals_one_shot(ctx, dev, codec, CRC, bs, data, offs, ref, ivs, lambda s, p: 3 * bs + 5, d_src=d_src, other_iv0=True)
    assert any(f > 0 for f in run.fronts)
    img = run.image()
    index = np.concatenate([[0], np.cumsum(run.lengths)]).astype(np.int64)
    sums = np.asarray(run.sums, np.int64)
    d_img, d_back = dev.upload(img), dev.alloc(data.size + 64)
    assert ctx.decompress_range_device(codec, CRC, d_img, img.size, index, sums, d_back, data.size) == data.size
    assert np.array_equal(dev.download(d_back, data.size), data)
    d_out, back = dev.alloc(8192), []
    with ctx.decode_stream(codec, CRC, index, sums, encrypted=True) as ds:
        while True:
            r = ds.feed_device(d_img + ds.position, min(5000, img.size - ds.position), d_out, 8192)
            assert r.code == 0
            back.append(dev.download(d_out, r.out_len).copy())
            if r.at_end:
                break
            assert r.consumed > 0 or r.out_len > 0
    assert np.array_equal(np.concatenate(back), data)


# ---- 10. refusals and protocol ------------------------------------------------------------------------------------------------------
def _one_shot_still_works(ctx, dev, d_src, offs, ivs, want):
    img, _, _ = one_shot(ctx, dev, LZ4, ADLER, offs, d_src, ivs)
    assert np.array_equal(img, want)


def test_refusals_and_protocol(ctxs, dev):
    import s3shuffle

    key = KEYS[16]
    ctx, refc, plainc = ctxs(LZ4, 64, key)
    data, offs = make_source([100, 64], 19)
    ivs = make_ivs(2, 10)
    d_src, d_dst = dev.upload(data), dev.alloc(4096)
    ref = Ref(refc, plainc, dev, LZ4, ADLER, data, offs, key, ivs, d_src)
    three = np.concatenate([ivs, np.zeros((1, 16), np.uint8)]).reshape(-1)

    with pytest.raises(s3shuffle.CodecError) as e:  # the layer is off
        plainc.compress_stream(LZ4, 0, encrypted=True)
    assert e.value.code == E_INVALID
    plainc.set_io_encryption(key)
    _one_shot_still_works(plainc, dev, d_src, offs, ivs, ref.img)
    plainc.set_io_encryption(None)
    for codec in (ZSTD, LZF):  # LZF: the option is off on this context
        with pytest.raises(s3shuffle.CodecError) as e:
            ctx.compress_stream(codec, 0, encrypted=True)
        assert e.value.code == E_UNSUPPORTED
    with pytest.raises(s3shuffle.CodecError) as e:  # the plain open keeps its answer on a keyed context
        ctx.compress_stream(LZ4, 0)
    assert e.value.code == E_UNSUPPORTED
    _one_shot_still_works(ctx, dev, d_src, offs, ivs, ref.img)

    # IV counts: none set, one too few, one too many - the stream does not move, and the array is consumed either way
    s = ctx.compress_stream(LZ4, ADLER, encrypted=True)
    for n_ivs in (None, 2, 4):
        if n_ivs is not None:
            ctx.set_stream_ivs(np.zeros(16 * n_ivs, np.uint8))
        with pytest.raises(s3shuffle.CodecError) as e:
            s.feed_device(d_src, 164, [100, 164], d_dst, 4096)
        assert e.value.code == E_INVALID and s.position == 0 and s.written == 0
    ctx.set_stream_ivs(three)
    with pytest.raises(s3shuffle.CodecError) as e:  # a refused feed consumed them too
        s.feed_device(d_src, 164, [100, -1], d_dst, 4096)
    with pytest.raises(s3shuffle.CodecError) as e:
        s.feed_device(d_src, 164, [100, 164], d_dst, 4096)
    assert e.value.code == E_INVALID and s.position == 0
    ctx.set_stream_ivs(np.zeros(16, np.uint8))  # a feed that launches nothing consumes them as well
    r = s.feed_device(d_src, 10, [], d_dst, 4096)
    assert (r.code, r.consumed, r.need_src) == (0, 0, 64)
    with pytest.raises(s3shuffle.CodecError) as e:
        s.feed_device(d_src, 10, [], d_dst, 4096)
    assert e.value.code == E_INVALID
    _one_shot_still_works(ctx, dev, d_src, offs, ivs, ref.img)

    # a one-shot encrypted call between two feeds; entry 0 differs on the partition already open; close inside a partition
    ctx.set_stream_ivs(ivs[0])
    r = s.feed_device(d_src, 64, [], d_dst, 4096)
    first = dev.download(d_dst, r.out_len).copy()
    assert r.consumed == 64 and np.array_equal(first, ref.img[:r.out_len])
    _one_shot_still_works(ctx, dev, d_src, offs, ivs, ref.img)
    assert ctx.compress_stream(LZ4, ADLER, encrypted=True).close() == 0  # at a boundary
    s2 = ctx.compress_stream(LZ4, ADLER, encrypted=True)
    ctx.set_stream_ivs(ivs[0])
    assert s2.feed_device(d_src, 64, [], d_dst, 4096).consumed == 64
    with pytest.raises(s3shuffle.CodecError) as e:
        s2.close()  # inside a partition
    assert e.value.code == E_INVALID
    other = three.copy()
    other[:16] ^= 0xFF
    ctx.set_stream_ivs(other)
    r = s.feed_device(d_src + 64, 100, [36, 100], d_dst, 4096)
    assert (r.consumed, r.parts_closed) == (100, 2)
    assert np.array_equal(np.concatenate([first, dev.download(d_dst, r.out_len)]), ref.img)
    assert [int(x) for x in r.lengths] == [int(x) for x in np.diff(ref.index)] and [int(x) for x in r.checksums] == [int(x) for x in ref.sums]
    assert s.close() == 0

    # a key change after open: the same key again, another key, off - feeds answer S3S_E_INVALID, then close
    for change in (key, KEYS[32], None):
        ctx.set_io_encryption(key)
        s = ctx.compress_stream(LZ4, ADLER, encrypted=True)
        ctx.set_io_encryption(change)
        ctx.set_stream_ivs(three)
        with pytest.raises(s3shuffle.CodecError) as e:
            s.feed_device(d_src, 164, [100, 164], d_dst, 4096)
        assert e.value.code == E_INVALID and s.position == 0 and s.written == 0
        assert s.close() == 0
    ctx.set_io_encryption(key)
    _one_shot_still_works(ctx, dev, d_src, offs, ivs, ref.img)
