"""GPU: the batched feed of the streaming map side under IO encryption (s3s_cstream_feed_batch* over streams of
s3s_cstream_open_encrypted: ONE AES-CTR pass over the outputs of all windows of a call).

The witnesses are the plain file's (test_gpu_compress_stream_batch.Rig, imported as it is): the keyed model of the contract
(cstream_units_encrypted.py); a twin - the same streams on a second keyed context, fed the same windows and IVs through single
keyed feeds, compared in status, every result field, bytes, lengths, checksums, position and written; and at the end the
one-shot keyed call's image, index differences and checksums, and spark_crypto_ref over the PLAIN image.  Every destination
lies between guard bands prefilled with 0xA5.  After every call the read-only key 19 equals the number of entries whose window
holds a unit (0 where the call goes one by one), and key 18 - plain windows only - is 0."""
import copy

import numpy as np
import pytest

import cstream_units as cu
from hipdev import Dev
from test_gpu_compress_stream_batch import (ADLER, CRC, CRC32C, E_CAPACITY, E_INVALID, GUARD, LZ4, LZF, NONE, NOT_RUN, OPT_BATCH, OPT_LZF, SHAPE_BS,
                                            SNAPPY, Rig, make_source, shape_sizes)

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -6
OPT_BATCH_ENC = 19
KEYS = {n: bytes((11 * i + n) & 0xFF for i in range(n)) for n in (16, 24, 32)}
KEY = KEYS[16]


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def ctxs():
    """make(codec) -> 4 contexts (the streams', the twin's, the one-shot reference's, an unkeyed one for the plain image)"""
    import s3shuffle

    made = []

    def make(codec, n=4):
        out = []
        for _ in range(n):
            c = s3shuffle.Codec(0)
            made.append(c)
            if codec == LZF:
                c.set_option(OPT_LZF, 1)
            out.append(c)
        return out

    yield make
    for c in made:
        c.close()


class KeyedRig(Rig):
    """Rig under a key, with the two counters read after every call.  other_iv0: entry 0 of the slice of a stream whose open
    partition already has image bytes is another IV (it is ignored: the carried one is used)."""

    def __init__(self, c4, dev, codec, algo, sources, key=KEY, other_iv0=False, **kw):
        self.other_iv0 = other_iv0
        super().__init__(c4[:3], dev, codec, algo, sources, key=key, plainc=c4[3], **kw)
        self.enc_calls = 0
        for st in self.S:
            st.dead = False  # True: the single feed refuses the stream itself (a stale key setting, a plain stream)

    def _ivs(self, st, n_ends):
        a = super()._ivs(st, n_ends)
        if self.other_iv0 and st.model.open_img > 0:
            a[0] = 0xEE
        return a

    def round(self, specs, expect_code=None):
        want = 0
        for i, wlen, cap, ends in specs:
            st = self.S[i]
            if ends is None:
                ends = cu.ends_in_window(st.offs, st.pos, st.n_closed, wlen)
            valid = wlen >= 0 and cap >= 0 and list(ends) == sorted(ends) and all(0 <= e <= wlen for e in ends)
            want += bool(valid and not st.dead and st.model._units(wlen, list(ends)))
        if self.codec == NONE or self.mixed_bs or len(specs) < 2:
            want = 0
        res = super().round(specs, expect_code)  # (asserts key 18 == 0: the rig is keyed)
        got = self.ctx.get_option(OPT_BATCH_ENC)
        assert got == want, (got, want, specs)
        assert self.ctx.compress_batch_encrypted_entries == got and self.ctx.get_option(OPT_BATCH) == 0
        self.enc_calls += got > 0
        return res

    def finish(self, key=KEY):
        import spark_crypto_ref as scr

        live = [st for st in self.S if not st.dead]
        dead, self.S = [st for st in self.S if st.dead], live
        super().finish()
        for st in live:  # the image is Spark's: IV | AES-CTR of the plain image, partition by partition
            want_img, _, want_sums = scr.encrypt_map_output(st.plain[0], np.asarray(st.plain[1], np.int64), key, st.ivs.reshape(-1), self.algo or ADLER)
            img = np.concatenate(st.out) if st.out else np.zeros(0, np.uint8)
            assert np.array_equal(img, want_img)
            if self.algo:
                assert st.sums == [int(x) for x in want_sums]
        for st in dead:
            st.s.close(check=False)
            st.t.close(check=False)


# ---- 1. equivalence: codec x checksum x key length ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo,key_bytes", [(0, 16), (ADLER, 24), (CRC, 32), (CRC32C, 16), (ADLER, 32), (CRC, 24)],
                         ids=["nosum-128", "adler32-192", "crc32-256", "crc32c-128", "adler32-256", "crc32-192"])
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_equivalence(ctxs, dev, codec, algo, key_bytes):
    bs = SHAPE_BS[codec]
    key = KEYS[key_bytes]
    sources = [make_source(shape_sizes(bs, 7 * i), 50 + i) for i in range(5)]
    rig = KeyedRig(ctxs(codec), dev, codec, algo, sources, key=key, bs=bs)
    rng = np.random.default_rng(codec * 10 + algo)
    windows = [lambda s, p: 1 << 30, lambda s, p: bs, lambda s, p: bs + 1, lambda s, p: 3 * bs - 1, lambda s, p: int(rng.integers(0, 4 * bs))]
    big = [max(x for p in st.model.sizes for x in p) for st in rig.S]
    caps = [rig.bound_of, lambda i, s, w, n: big[i] + 5, lambda i, s, w, n: [36, big[i] - 1, 3 * big[i]][s % 3], rig.bound_of,
            lambda i, s, w, n: int(rng.integers(0, 3 * big[i]))]
    rig.play(lambda i, s, p: windows[i](s, p), lambda i, s, w, n: caps[i](i, s, w, n))
    rig.finish(key)
    assert rig.enc_calls >= 3


# ---- 2. every cut position of a 600-byte map output, eight streams at a time ------------------------------------------------
def test_every_cut_position_lz4_eight_at_a_time(ctxs, dev):
    total, sizes = 600, [130, 0, 64, 1, 200, 0, 205]
    data, offs = make_source(sizes, 7)
    c4 = ctxs(LZ4)
    sched = [[w] for w in range(total + 1)]
    for k in range(0, len(sched), 8):
        group = sched[k:k + 8]
        rig = KeyedRig(c4, dev, LZ4, ADLER, [(data, offs)] * len(group), bs=64, ivs_seed=k)
        rig.play(lambda i, s, p: group[i][s] if s < len(group[i]) else int(offs[-1]), rig.bound_of)
        rig.finish()
        for p in (rig.d_src_all, rig.d_dst, rig.d_twin):
            dev.release(p)


# ---- 3. the carried key stream at every residue ---------------------------------------------------------------------------------
def test_all_sixteen_residues_of_the_carried_key_stream_in_one_call(ctxs, dev):
    """forty candidate streams whose first block of 64 bytes starts with k random bytes and ends in zeros: sixteen of them,
    one per residue of open_img mod 16 after that block, take it in round one and the rest of the partition in ONE call"""
    bs, rng = 64, np.random.default_rng(3)
    sources = []
    for k in range(40):
        data = np.zeros(200 + 64, np.uint8)
        data[:k] = rng.integers(1, 256, k, dtype=np.uint8)
        data[64:] = rng.integers(0, 256, 200, dtype=np.uint8)
        sources.append((data, np.array([0, 230, 264], np.int64)))
    rig = KeyedRig(ctxs(LZ4), dev, LZ4, CRC, sources, bs=bs, other_iv0=True)
    by_residue = {}
    for i, st in enumerate(rig.S):
        by_residue.setdefault(copy.deepcopy(st.model).feed(64, [], 1 << 20).out_len % 16, i)
    assert sorted(by_residue) == list(range(16)), sorted(by_residue)
    chosen = sorted(by_residue.values())
    rig.round([(i, 64, rig.S[i].bound, None) for i in chosen])
    assert sorted(rig.S[i].model.open_img % 16 for i in chosen) == list(range(16))
    res = rig.round([(i, 200, rig.S[i].bound, None) for i in chosen])
    assert all(r.code == 0 and r.parts_closed == 2 for r in res) and rig.ctx.get_option(OPT_BATCH_ENC) == 16
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


# ---- 4. mixed fates in one call -----------------------------------------------------------------------------------------------
def test_mixed_fates_in_one_call(ctxs, dev):
    c4 = ctxs(LZ4)
    ctx, twin = c4[:2]
    for c in c4[:3]:
        c.set_option(1, 64)
    plain = [c.compress_stream(LZ4, ADLER) for c in (ctx, twin)]  # opened before the layer is on
    for c in (ctx, twin):
        c.set_io_encryption(KEY)
    stale = [c.compress_stream(LZ4, ADLER, encrypted=True) for c in (ctx, twin)]  # ... and under an earlier key setting
    shapes = [[100, 64], [100], [0, 0, 50], [30, 30], [100, 64], [100, 64], [100, 64], [100, 64]]
    rig = KeyedRig(c4, dev, LZ4, ADLER, [make_source(s, 20 + i) for i, s in enumerate(shapes)], bs=64)
    S = rig.S
    for st, (s, t) in ((S[6], stale), (S[7], plain)):
        st.s.close(check=False)
        st.t.close(check=False)
        st.s, st.t, st.dead = s, t, True
    sizes0, sizes5 = S[0].model.sizes, S[5].model.sizes
    assert len(sizes5[0]) == 3 and sizes5[0][2] == 21
    rig.round([(5, 64, S[5].bound, None)])  # stream 5 takes its first block (and its IV) alone: n == 1 goes one by one
    before = [(st.s.position, st.s.written) for st in S]
    res = rig.round([(0, 164, sizes0[0][0] - 1, None),      # S3S_E_CAPACITY with the exact need_dst: the IV counts
                     (1, 10, 500, None),                     # no whole unit in the window: need_src
                     (2, 0, 500, [0, 0]),                    # only empty ends: nothing is launched, its IVs are consumed
                     (3, 60, 500, [60, 30]),                 # descending ends: this entry's own S3S_E_INVALID
                     (6, 164, S[6].bound, None),             # bound to an earlier key setting
                     (7, 164, S[7].bound, None),             # a plain stream on the keyed context
                     (4, 164, S[4].bound, None),             # takes its whole window
                     (5, 100, sizes5[0][1] + 20, None)],     # the tail block fits, its 21-byte end frame does not
                    expect_code=E_CAPACITY)
    assert (res[0].code, res[0].need_dst, res[0].out_len) == (E_CAPACITY, sizes0[0][0], 0) and sizes0[0][0] > 16 + 21
    assert (res[1].code, res[1].need_src, res[1].consumed, res[1].parts_closed) == (0, 64, 0, 0)
    assert (res[2].code, res[2].out_len, res[2].parts_closed, list(res[2].lengths)) == (0, 0, 2, [0, 0])
    assert res[3].code == E_INVALID and res[4].code == E_INVALID and res[5].code == E_UNSUPPORTED
    assert (res[6].code, res[6].consumed, res[6].parts_closed) == (0, 164, 2)
    assert (res[7].code, res[7].consumed, res[7].out_len, res[7].parts_closed) == (0, 36, sizes5[0][1], 0)
    assert rig.ctx.get_option(OPT_BATCH_ENC) == 3
    for i in (0, 1, 3, 6, 7):  # the untouched streams stay untouched
        assert (S[i].s.position, S[i].s.written) == before[i]
    res = rig.round([(5, 0, 64, [0]), (0, 164, S[0].bound, None)])  # an end at 0 writes the 21 bytes under the carried IV
    assert (res[0].code, res[0].consumed, res[0].out_len, res[0].parts_closed) == (0, 0, 21, 1) and res[1].parts_closed == 2
    for i in (6, 7):
        S[i].pos, S[i].n_closed = S[i].offs[-1], len(S[i].offs) - 1  # (they leave the schedule)
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


# ---- 5. the pass's 16 KiB tiles ---------------------------------------------------------------------------------------------
def test_outputs_that_end_around_a_pass_tile(ctxs, dev):
    """incompressible partitions (a stored LZ4 block is 21 + its bytes): outputs of 16383, 16384 and 16385 stored bytes that
    start their partition, and three that continue one at front = 1061 (residue 5: the tiles start 5 bytes in front of the
    output) and end 1 below, at and 1 above the first tile's end.  Every capacity is the bound: the next entry's destination
    lies directly behind the guard band"""
    bs, rng = 1024, np.random.default_rng(5)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8)  # noqa: E731
    sources = [(rnd(15 * bs + r), np.array([0, 15 * bs + r], np.int64)) for r in (650, 651, 652)]
    sources += [(rnd(16 * bs + r), np.array([0, 16 * bs + r], np.int64)) for r in (661, 662, 663)]
    rig = KeyedRig(ctxs(LZ4), dev, LZ4, CRC32C, sources, bs=bs, other_iv0=True)
    res = rig.round([(i, bs, rig.S[i].bound, None) for i in (3, 4, 5)])
    assert [r.out_len for r in res] == [16 + 21 + bs] * 3
    res = rig.round([(i, rig.S[i].offs[-1] - rig.S[i].pos, rig.S[i].bound, None) for i in range(6)])
    assert [r.out_len for r in res] == [16383, 16384, 16385, 16384 - 5 - 1, 16384 - 5, 16384 - 5 + 1]
    assert all(r.parts_closed == 1 for r in res) and rig.ctx.get_option(OPT_BATCH_ENC) == 6
    rig.finish()


# ---- 6. alignments and source order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4", "snappy"])
def test_guard_bands_at_sixteen_alignments(ctxs, dev, codec):
    bs = 1024
    sources = [make_source([bs + 3 * i, 0, 2 * bs + i, 5], 60 + i) for i in range(16)]
    rig = KeyedRig(ctxs(codec), dev, codec, ADLER, sources, bs=bs, aligns=list(range(16)))
    specs = []
    for i, st in enumerate(rig.S):
        f = copy.deepcopy(st.model).feed(st.offs[-1], st.offs[1:], 1 << 40)
        specs.append((i, st.offs[-1], f.out_len + (i % 7) - 3, None))  # a few bytes above and below out_len
    res = rig.round(specs)
    assert any(r.parts_closed < 4 for r in res) and any(r.parts_closed == 4 for r in res)
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_sources_at_descending_addresses(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    rig = KeyedRig(ctxs(codec), dev, codec, CRC, [make_source(shape_sizes(bs, i), 70 + i) for i in range(4)], bs=bs, src_descending=True)
    assert all(rig.S[i].d_src < rig.S[0].d_src for i in range(1, 4))
    rig.play(lambda i, s, p: 2 * bs + i, rig.bound_of)
    rig.finish()
    assert rig.enc_calls >= 2


# ---- 7. the IV across rounds, and the IV count ----------------------------------------------------------------------------------
def test_the_iv_is_carried_across_three_rounds(ctxs, dev):
    """a partition of four blocks and a tail, one block a round: rounds two to four get ANOTHER IV in entry 0 of their slice"""
    bs = 1024
    rig = KeyedRig(ctxs(SNAPPY), dev, SNAPPY, ADLER, [make_source([4 * bs + 9 + i, 0, bs], 140 + i) for i in range(3)], bs=bs, other_iv0=True)
    fronts = []
    for _ in range(4):
        fronts.append([st.model.open_img for st in rig.S])
        res = rig.round([(i, bs, rig.S[i].bound, None) for i in range(3)])
        assert all(r.code == 0 and r.consumed == bs and r.parts_closed == 0 for r in res)
    assert fronts[0] == [0, 0, 0] and all(f > 16 for row in fronts[1:] for f in row)
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


def test_a_wrong_iv_count_is_refused_and_the_array_consumed(ctxs, dev):
    rig = KeyedRig(ctxs(LZ4), dev, LZ4, ADLER, [make_source(shape_sizes(1024, i), 95 + i) for i in range(3)], bs=1024)
    rows = [(st.s, st.d_src, 2000, cu.ends_in_window(st.offs, 0, 0, 2000), rig.d_dst + st.dst_at, st.bound) for st in rig.S]
    right = sum(len(r[3]) + 1 for r in rows)
    for count in (right - 1, right + 1):
        rig.ctx.set_stream_ivs(np.zeros(16 * count, np.uint8))
        res = rig.ctx.compress_stream_feed_batch(rows)
        assert rig.ctx.last_compress_batch_code == E_INVALID and [r.code for r in res] == [NOT_RUN] * 3
        assert rig.ctx.get_option(OPT_BATCH_ENC) == 0 and rig.ctx.get_option(OPT_BATCH) == 0
        assert all((st.s.position, st.s.written) == (0, 0) for st in rig.S)
        res = rig.ctx.compress_stream_feed_batch(rows)  # consumed: the next call has no IVs at all
        assert rig.ctx.last_compress_batch_code == E_INVALID and [r.code for r in res] == [NOT_RUN] * 3
    with pytest.raises(Exception):
        rig.ctx.set_option(OPT_BATCH_ENC, 1)
    rig.play(lambda i, s, p: 1500 + 100 * i, rig.bound_of)
    rig.finish()
    assert rig.enc_calls >= 2


def test_only_plain_streams_on_a_keyed_context_go_one_by_one(ctxs, dev):
    """kept as found: a batch without a single keyed stream on a keyed context is not batched and wants no IVs - every entry
    gets the single feed's S3S_E_UNSUPPORTED as its own status, nothing is launched, keys 18 and 19 stay 0"""
    ctx = ctxs(LZ4, 1)[0]
    ctx.set_option(1, 64)
    plain = [ctx.compress_stream(LZ4, ADLER) for _ in range(3)]  # opened before the layer is on
    ctx.set_io_encryption(KEY)
    d_src, d_dst = dev.alloc(4096), dev.alloc(3 * 4096)
    res = ctx.compress_stream_feed_batch([(s, d_src, 100, [100], d_dst + 4096 * i, 4096) for i, s in enumerate(plain)])
    assert ctx.last_compress_batch_code == E_UNSUPPORTED and [r.code for r in res] == [E_UNSUPPORTED] * 3
    assert ctx.get_option(OPT_BATCH_ENC) == 0 and ctx.get_option(OPT_BATCH) == 0
    assert all((s.position, s.written) == (0, 0) for s in plain)
    for s in plain:
        s.close()


def test_a_window_of_too_many_blocks_is_refused_behind_the_checks(ctxs, dev):
    """kept as found: the single feed counts the blocks of its window (0x7fffff00 of them at most) only behind the argument
    checks and the IV count check.  A window that claims 2^31 blocks of 64 bytes and has a negative capacity, descending ends or
    a wrong IV count gets that check's S3S_E_INVALID at once: its blocks are never walked, nothing is launched"""
    import s3shuffle

    ctx = ctxs(LZ4, 1)[0]
    ctx.set_option(1, 64)
    ctx.set_io_encryption(KEY)
    s = ctx.compress_stream(LZ4, ADLER, encrypted=True)
    d_src, d_dst = dev.alloc(4096), dev.alloc(4096)
    huge = 64 << 31
    for ends, cap, n_ivs in (([], -1, 1), ([huge, 5], 4096, 3), ([], 4096, 2), ([], 4096, None)):
        if n_ivs is not None:
            ctx.set_stream_ivs(np.zeros(16 * n_ivs, np.uint8))
        with pytest.raises(s3shuffle.CodecError) as e:
            s.feed_device(d_src, huge, ends, d_dst, cap)
        assert e.value.code == E_INVALID, e.value
        assert (s.position, s.written) == (0, 0)
    s.close()


# ---- 8. host buffers, many streams ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_host_buffers(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    rig = KeyedRig(ctxs(codec), dev, codec, ADLER, [make_source(shape_sizes(bs, 3 * i), 100 + i) for i in range(3)], bs=bs, host=True)
    big = [max(x for p in st.model.sizes for x in p) for st in rig.S]
    rig.play(lambda i, s, p: 2 * bs + 7 * i, lambda i, s, w, n: [big[i] - 1, 2 * big[i] + 40][s % 2] if i else rig.bound_of(i, s, w, n))
    rig.finish()
    assert rig.enc_calls >= 2


def test_sixty_four_streams_in_one_call(ctxs, dev):
    bs = 32768
    rig = KeyedRig(ctxs(LZ4), dev, LZ4, CRC32C, [make_source([bs], 200 + i) for i in range(64)], key=KEYS[32])
    res = rig.round([(i, bs, rig.S[i].bound, None) for i in range(64)])
    assert all(r.code == 0 and r.consumed == bs and r.parts_closed == 1 for r in res) and rig.ctx.get_option(OPT_BATCH_ENC) == 64
    rig.finish(KEYS[32])


# ---- 9. other calls between rounds, then every image decoded back ---------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_other_calls_between_rounds_and_round_trip(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    rig = KeyedRig(ctxs(codec), dev, codec, ADLER, [make_source(shape_sizes(bs, i), 110 + i) for i in range(3)], bs=bs)
    other, ooffs = make_source([3000, 0, 4000], 120)
    oivs = np.arange(48, dtype=np.uint8)
    rig.refc.set_stream_ivs(oivs)
    want = rig.refc.compress_map_output(codec, ADLER, other, ooffs)
    rounds = 0
    while not all(rig.done(i) for i in range(3)):
        rounds += 1
        assert rounds < 100
        live = [i for i in range(3) if not rig.done(i)]
        rig.round([(i, min(bs + 100, rig.S[i].offs[-1] - rig.S[i].pos), rig.S[i].bound, None) for i in live])
        rig.ctx.set_stream_ivs(oivs)  # a keyed one-shot compress and a checksum call on the same context
        got = rig.ctx.compress_map_output(codec, ADLER, other, ooffs)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(rig.ctx.checksum_ranges(CRC, other, ooffs), rig.refc.checksum_ranges(CRC, other, ooffs))
    rig.finish()
    win, cap = (70000, 70000) if codec == LZF else (5000, 8192)  # (a window and a destination that hold a unit)
    d_out = dev.alloc(cap)
    for st in rig.S:
        img = np.concatenate(st.out)
        index, sums = np.asarray(st.ref[1], np.int64), np.asarray(st.sums, np.int64)
        back = rig.ctx.decompress_range(codec, ADLER, img, index, sums, dst_capacity=st.data.size)
        assert np.array_equal(back, st.data)
        d_img, parts = dev.upload(img), []
        with rig.ctx.decode_stream(codec, ADLER, index, sums, encrypted=True) as ds:
            while True:
                r = ds.feed_device(d_img + ds.position, min(win, img.size - ds.position), d_out, cap)
                assert r.code == 0
                parts.append(dev.download(d_out, r.out_len).copy())
                if r.at_end:
                    break
                assert r.consumed > 0 or r.out_len > 0
        assert np.array_equal(np.concatenate(parts), st.data)
