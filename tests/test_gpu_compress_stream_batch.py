"""GPU: the batched feed of the streaming map side (s3s_cstream_feed_batch*: one window of each of several streams per call).

Three witnesses check every round: the contract's Python model (cstream_units.py); a twin - the same streams on a second
context, fed the same windows through single feeds, compared in status, every result field, bytes, lengths, checksums, position
and written; and, when a stream has closed its map output, the concatenation against the one-shot call's image, index
differences and checksums.  Every destination lies between guard bands in one allocation prefilled with 0xA5: the bands and
d_dst[out_len, dst_capacity) must stay untouched.  The read-only key 18 is read after every call and compared with the number
of entries whose window holds at least one unit (0 where the call goes one by one)."""
import copy

import numpy as np
import pytest

import cstream_units as cu
import cstream_units_encrypted as cue
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, LZF = 0, 1, 2, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, NOT_RUN = -1, -2, -100
OPT_LZ4_BS, OPT_SNAPPY_BS, OPT_LZ4_BS_LARGE, OPT_LZF, OPT_BATCH = 1, 2, 8, 10, 18
PREFILL, GUARD = 0xA5, 64
KEY = bytes((7 * i + 16) & 0xFF for i in range(16))


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def ctxs():
    """make(codec, n) -> n contexts with the codec's opt-in set; closed at teardown"""
    import s3shuffle

    made = []

    def make(codec, n=3):
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


def set_bs(c, codec, bs, large=False):
    if codec == LZ4 and bs:
        c.set_option(OPT_LZ4_BS_LARGE if large else OPT_LZ4_BS, bs)
    if codec == SNAPPY and bs:
        c.set_option(OPT_SNAPPY_BS, bs)


def make_source(sizes, seed):
    """half compressible, half random (stored blocks), one run of zeros"""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    phrase = np.frombuffer(b"the quick brown fox jumps over the lazy dog; ", np.uint8)
    data = np.resize(phrase, total).copy()
    data[rng.integers(0, max(total, 1), total // 40)] = 7
    data[total // 2:] = rng.integers(0, 256, total - total // 2, dtype=np.uint8)
    data[total // 3: total // 3 + total // 10] = 0
    return data, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class St:
    """one stream of a rig, with its twin and its model"""


class Rig:
    """n streams on `ctx`, their twins on `twin`, the one-shot references from `refc` (and, encrypted, the plain image from an
    unkeyed context).  sources: [(data, offs)]; bs: one block size or one per stream."""

    def __init__(self, ctx3, dev, codec, algo, sources, bs=None, large=False, key=None, src_descending=False, aligns=None, host=False,
                 plainc=None, ivs_seed=5):
        self.ctx, self.twin, self.refc = ctx3[:3]
        self.dev, self.codec, self.algo, self.key, self.host = dev, codec, algo, key, host
        n = len(sources)
        bss = list(bs) if isinstance(bs, (list, tuple)) else [bs] * n
        self.mixed_bs = len(set(bss)) > 1
        if key is not None:
            for c in ctx3[:3]:
                c.set_io_encryption(key)
        # one allocation for the sources (ascending or descending addresses), one for the destinations of each side
        lens = [int(d.size) for d, _ in sources]
        starts = np.concatenate([[0], np.cumsum([x + GUARD for x in lens])]).astype(int)
        self.d_src_all = dev.alloc(int(starts[-1]) + GUARD)
        self.S = []
        dst_at = GUARD
        for i, ((data, offs), b) in enumerate(zip(sources, bss)):
            st = St()
            for c in ctx3[:3] + ([plainc] if plainc else []):
                set_bs(c, codec, b, large)
            st.data, st.offs, st.bs = data, [int(x) for x in offs], cu.block_size(codec, b or 32768)
            k = (n - 1 - i) if src_descending else i
            st.d_src = self.d_src_all + int(starts[k])
            dev.write(st.d_src, data)
            st.ivs = np.random.default_rng(ivs_seed + i).integers(0, 256, (len(offs) - 1, 16), dtype=np.uint8) if key is not None else None
            st.ref = self._one_shot(self.refc, st, st.ivs)
            if key is not None:
                plain = self._one_shot(plainc, st, None, algo=0)
                st.plain = plain
                st.model = cue.Model(codec, st.bs, cue.unit_sizes_from_plain_image(codec, plain[0], plain[1]))
            else:
                st.model = cu.Model(codec, st.bs, cu.unit_sizes_from_image(codec, st.ref[0], st.ref[1]))
            st.s = self.ctx.compress_stream(codec, algo, encrypted=key is not None)
            st.t = self.twin.compress_stream(codec, algo, encrypted=key is not None)
            st.bound = max(st.s.feed_bound(data.size, len(offs) - 1), 1024)  # (the slot's size; a few tests give small sources large capacities)
            st.align = (aligns[i] if aligns else 0)
            st.dst_at = ((dst_at + 15) & ~15) + st.align
            dst_at = st.dst_at + st.bound + GUARD
            st.pos = st.n_closed = 0
            st.out, st.lengths, st.sums, st.want_w, st.want_c, st.step = [], [], [], 0, 0, 0
            self.S.append(st)
        self.dst_bytes = dst_at + GUARD
        if host:
            self.h_dst, self.h_twin = np.full(self.dst_bytes, PREFILL, np.uint8), np.full(self.dst_bytes, PREFILL, np.uint8)
        else:
            self.d_dst, self.d_twin = dev.alloc(self.dst_bytes), dev.alloc(self.dst_bytes)
        self.calls = self.batched_calls = 0

    def _one_shot(self, c, st, ivs, algo=None):
        algo = self.algo if algo is None else algo
        cap = c.max_compressed_size(self.codec, st.offs)
        d_dst = self.dev.alloc(cap + 64)
        if ivs is not None:
            c.set_stream_ivs(ivs.reshape(-1))
        total, index, sums = c.compress_map_output_device(self.codec, algo, st.d_src, st.offs, d_dst, cap)
        img = self.dev.download(d_dst, total).copy()
        self.dev.release(d_dst)
        return img, [int(x) for x in index], sums

    def done(self, i):
        st = self.S[i]
        return st.pos >= st.offs[-1] and st.n_closed >= len(st.offs) - 1

    def _ivs(self, st, n_ends):
        a = np.zeros((max(n_ends, 0) + 1, 16), np.uint8)
        for j in range(a.shape[0]):
            if st.n_closed + j < len(st.ivs):
                a[j] = st.ivs[st.n_closed + j]
        return a

    def batchable(self):
        return self.codec != NONE and self.key is None and not self.mixed_bs

    def round(self, specs, expect_code=None):
        """specs: [(stream, wlen, cap, ends or None)] -> the results.  Every witness is consulted."""
        dev, S = self.dev, self.S
        if self.host:
            self.h_dst[:] = PREFILL
            self.h_twin[:] = PREFILL
        else:
            dev.fill(self.d_dst, PREFILL, self.dst_bytes)
            dev.fill(self.d_twin, PREFILL, self.dst_bytes)
        rows, want_batched = [], 0
        full = []
        for i, wlen, cap, ends in specs:
            st = S[i]
            if ends is None:
                ends = cu.ends_in_window(st.offs, st.pos, st.n_closed, wlen)
            full.append((i, wlen, cap, list(ends)))
            valid = wlen >= 0 and cap >= 0 and list(ends) == sorted(ends) and all(0 <= e <= wlen for e in ends)
            want_batched += bool(valid and st.model._units(wlen, list(ends)))
            assert cap <= st.bound + GUARD // 2
            if self.host:
                rows.append((st.s, st.data[st.pos:st.pos + max(wlen, 0)], ends, self.h_dst[st.dst_at:st.dst_at + max(cap, 0)], cap))
            else:
                rows.append((st.s, st.d_src + st.pos, wlen, ends, self.d_dst + st.dst_at, cap))
        if self.key is not None:
            self.ctx.set_stream_ivs(np.concatenate([self._ivs(S[i], len(e)) for i, _, _, e in full]).reshape(-1))
        res = self.ctx.compress_stream_feed_batch_host(rows) if self.host else self.ctx.compress_stream_feed_batch(rows)
        code = self.ctx.last_compress_batch_code
        got18 = self.ctx.get_option(OPT_BATCH)
        self.calls += 1
        if self.batchable() and len(specs) > 1:
            assert got18 == want_batched, (got18, want_batched, full)
            self.batched_calls += got18 > 0
        else:
            assert got18 == 0
        mine = self.h_dst if self.host else dev.download(self.d_dst, self.dst_bytes)
        first_bad = 0
        for (i, wlen, cap, ends), r in zip(full, res):
            st = S[i]
            if self.key is not None:
                self.twin.set_stream_ivs(self._ivs(st, len(ends)).reshape(-1))
            try:
                if self.host:
                    st.t.feed(st.data[st.pos:st.pos + max(wlen, 0)], ends, self.h_twin[st.dst_at:st.dst_at + max(cap, 0)], cap)
                else:
                    st.t.feed_device(st.d_src + st.pos, wlen, ends, self.d_twin + st.dst_at, cap)
            except Exception as e:  # noqa: BLE001 - the twin's refusal: the code is in last_result
                assert getattr(e, "code", None) == st.t.last_result.code != 0, e
            t = st.t.last_result
            fields = lambda x: (x.code, x.consumed, x.out_len, x.need_src, x.need_dst, x.parts_closed, [int(v) for v in x.lengths],  # noqa: E731
                                [int(v) for v in x.checksums] if x.checksums is not None else None)
            assert fields(r) == fields(t), (i, wlen, cap, ends, fields(r), fields(t))
            assert (st.s.position, st.s.written) == (st.t.position, st.t.written)
            if t.code == 0 or t.code == E_CAPACITY:
                m = st.model.feed(wlen, ends, cap)
                assert (r.code, r.consumed, r.out_len, r.need_src, r.need_dst, r.parts_closed, tuple(int(v) for v in r.lengths)) == m.fields(), \
                    (i, wlen, cap, ends, m.fields())
            if r.code != 0 and first_bad == 0:
                first_bad = r.code
            out_len = r.out_len if r.code == 0 else 0
            # bytes: equal to the twin's, nothing at or beyond out_len, the bands around the destination untouched
            theirs = self.h_twin[st.dst_at:st.dst_at + out_len] if self.host else dev.download(self.d_twin + st.dst_at, out_len)
            assert np.array_equal(mine[st.dst_at:st.dst_at + out_len], theirs), (i, wlen, cap)
            end = st.dst_at + st.bound + GUARD
            assert (mine[st.dst_at + out_len:end] == PREFILL).all() and (mine[st.dst_at - GUARD // 2:st.dst_at] == PREFILL).all(), (i, wlen, cap, out_len)
            if r.code == 0:
                st.pos += r.consumed
                st.n_closed += r.parts_closed
                assert st.s.position == st.pos
                if out_len:
                    st.out.append(mine[st.dst_at:st.dst_at + out_len].copy())
                st.lengths += [int(v) for v in r.lengths]
                if self.algo:
                    st.sums += [int(v) for v in r.checksums]
        assert code == first_bad if expect_code is None else code == expect_code, (code, first_bad)
        return res

    def play(self, window_of, cap_of, max_rounds=2000, per_call=None):
        """every stream follows its own schedule (window_of(i, step, pos), cap_of(i, step, wlen, n_ends); a feed that asks for
        more is repeated with what it asked for) until all have closed; finished streams leave the call"""
        rounds = 0
        while not all(self.done(i) for i in range(len(self.S))):
            rounds += 1
            assert rounds < max_rounds, "the schedule does not end"
            live = [i for i in range(len(self.S)) if not self.done(i)][:per_call]
            specs = []
            for i in live:
                st = self.S[i]
                wlen = min(max(window_of(i, st.step, st.pos), st.want_w), st.offs[-1] - st.pos)
                ends = cu.ends_in_window(st.offs, st.pos, st.n_closed, wlen)
                specs.append((i, wlen, min(max(cap_of(i, st.step, wlen, len(ends)), st.want_c), st.bound), ends))
            for (i, wlen, cap, _), r in zip(specs, self.round(specs)):
                st = self.S[i]
                st.step += 1
                st.want_w = st.want_c = 0
                if r.code == E_CAPACITY:
                    st.want_w, st.want_c = wlen, r.need_dst
                elif r.consumed == 0 and r.parts_closed == 0:
                    st.want_w = r.need_src
        return rounds

    def finish(self):
        for st in self.S:
            assert st.s.close() == 0 and st.t.close() == 0
            img = np.concatenate(st.out) if st.out else np.zeros(0, np.uint8)
            ref_img, ref_index, ref_sums = st.ref
            assert img.size == ref_img.size and np.array_equal(img, ref_img)
            assert st.lengths == [int(x) for x in np.diff(ref_index)]
            if self.algo:
                assert st.sums == [int(x) for x in ref_sums]

    def bound_of(self, i, step, wlen, n_ends):
        return self.S[i].s.feed_bound(wlen, n_ends)


def shape_sizes(bs, k):
    """7 partitions; empty ones first, in the middle and last"""
    return [0, bs + k, 1 + k, 0, 2 * bs + 3 * k, bs - 1, 0]


SHAPE_BS = {LZ4: 1024, SNAPPY: 1024, LZF: 65535}


# ---- 1. equivalence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, ADLER, CRC, CRC32C], ids=["nosum", "adler32", "crc32", "crc32c"])
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_equivalence(ctxs, dev, codec, algo):
    bs = SHAPE_BS[codec]
    sources = [make_source(shape_sizes(bs, 7 * i), 50 + i) for i in range(5)]
    rig = Rig(ctxs(codec), dev, codec, algo, sources, bs=bs)
    rng = np.random.default_rng(codec * 10 + algo)
    windows = [lambda s, p: 1 << 30, lambda s, p: bs, lambda s, p: bs + 1, lambda s, p: 3 * bs - 1, lambda s, p: int(rng.integers(0, 4 * bs))]
    big = [max(x for p in st.model.sizes for x in p) for st in rig.S]
    caps = [rig.bound_of, lambda i, s, w, n: big[i] + 5, lambda i, s, w, n: [20, big[i] - 1, 3 * big[i]][s % 3], rig.bound_of,
            lambda i, s, w, n: int(rng.integers(0, 3 * big[i]))]
    rig.play(lambda i, s, p: windows[i](s, p), lambda i, s, w, n: caps[i](i, s, w, n))
    rig.finish()
    assert rig.batched_calls >= 3


# ---- 2. every cut position, eight at a time ---------------------------------------------------------------------------------
def _eight_at_a_time(ctxs, dev, codec, algo, bs, sizes, seed, schedules):
    """schedules: one list of window lengths per stream run (then the rest of the source); eight runs share a call"""
    data, offs = make_source(sizes, seed)
    c3 = ctxs(codec)
    for k in range(0, len(schedules), 8):
        group = schedules[k:k + 8]
        rig = Rig(c3, dev, codec, algo, [(data, offs)] * len(group), bs=bs)
        rig.play(lambda i, s, p: group[i][s] if s < len(group[i]) else int(offs[-1]), rig.bound_of)
        rig.finish()
        for p in (rig.d_src_all, rig.d_dst, rig.d_twin):
            dev.release(p)


def test_every_cut_position_lz4_eight_at_a_time(ctxs, dev):
    total = 600
    sched = [[w] for w in range(total + 1)] + [[w1, w2] for w1 in range(0, total, 37) for w2 in range(1, total, 53)]
    _eight_at_a_time(ctxs, dev, LZ4, ADLER, 64, [130, 0, 64, 1, 200, 0, 205], 7, sched)


def test_cut_positions_snappy_1024_eight_at_a_time(ctxs, dev):
    sizes = [1024, 2048 + 5, 0, 1023, 3]
    total, offs = sum(sizes), np.cumsum([0] + sizes)
    cuts = sorted({c for k in range(1, 6) for c in (1024 * k - 1, 1024 * k, 1024 * k + 1)} | set(range(0, total, 97)) | {int(e) for e in offs})
    _eight_at_a_time(ctxs, dev, SNAPPY, CRC, 1024, sizes, 8, [[c] for c in cuts if c <= total])


def test_cut_positions_lzf_eight_at_a_time(ctxs, dev):
    sizes = [65535 + 10, 0, 2 * 65535, 3]
    total = sum(sizes)
    ws = (65534, 65535, 65536, 65535 + 9, 65535 + 10, 65535 + 11, 2 * 65535 + 9, 2 * 65535 + 10, 2 * 65535 + 11, total - 3, total - 1)
    _eight_at_a_time(ctxs, dev, LZF, CRC32C, None, sizes, 9, [[w] for w in ws])


# ---- 3. mixed fates in one call -------------------------------------------------------------------------------------------------
def test_mixed_fates_in_one_call(ctxs, dev):
    shapes = [[100, 64], [100], [0, 0, 50], [30, 30], [100, 64], [100, 64]]
    rig = Rig(ctxs(LZ4), dev, LZ4, ADLER, [make_source(s, 20 + i) for i, s in enumerate(shapes)], bs=64)
    S = rig.S
    sizes0, sizes5 = S[0].model.sizes, S[5].model.sizes
    assert len(sizes5[0]) == 3 and sizes5[0][2] == 21
    rig.round([(5, 64, S[5].bound, None)])  # stream 5 takes its first block alone: n == 1 goes one by one
    before = [(st.s.position, st.s.written) for st in S]
    res = rig.round([(0, 164, sizes0[0][0] - 1, None),      # S3S_E_CAPACITY with the exact need_dst
                     (1, 10, 500, None),                     # no whole unit in the window: need_src
                     (2, 0, 500, [0, 0]),                    # only empty ends: nothing is launched
                     (3, 60, 500, [60, 30]),                 # descending ends: this entry's own S3S_E_INVALID
                     (4, 164, S[4].bound, None),             # takes its whole window
                     (5, 100, sizes5[0][1] + 20, None)],     # the tail block fits, its 21-byte end frame does not
                    expect_code=E_CAPACITY)
    assert (res[0].code, res[0].need_dst, res[0].out_len) == (E_CAPACITY, sizes0[0][0], 0)
    assert (res[1].code, res[1].need_src, res[1].consumed, res[1].parts_closed) == (0, 64, 0, 0)
    assert (res[2].code, res[2].out_len, res[2].parts_closed, list(res[2].lengths)) == (0, 0, 2, [0, 0])
    assert res[3].code == E_INVALID
    assert (res[4].code, res[4].consumed, res[4].parts_closed) == (0, 164, 2)
    assert (res[5].code, res[5].consumed, res[5].out_len, res[5].parts_closed) == (0, 36, sizes5[0][1], 0)
    assert rig.ctx.get_option(OPT_BATCH) == 3
    for i in (0, 1, 3):  # the untouched streams stay untouched
        assert (S[i].s.position, S[i].s.written) == before[i]
    res = rig.round([(5, 0, 64, [0]), (0, 164, S[0].bound, None)])  # an end at 0 writes the 21 bytes
    assert (res[0].code, res[0].consumed, res[0].out_len, res[0].parts_closed) == (0, 0, 21, 1) and res[1].parts_closed == 2
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


# ---- 4. cut tiles ---------------------------------------------------------------------------------------------------------------
def test_cut_tiles(ctxs, dev):
    """windows of 1, 255, 256, 257 and 513 plan items in one call at block size 64: a partition of n - 1 blocks and its end
    frame (1: one block of an open partition), each cut at its own capacity in the next rounds"""
    items = [1, 255, 256, 257, 513]
    sources = [make_source([64 * (n - 1) - 5] if n > 1 else [128], 30 + n) for n in items]
    rig = Rig(ctxs(LZ4), dev, LZ4, CRC, sources, bs=64)
    for st, n in zip(rig.S, items):
        assert len(st.model._units(st.offs[-1] if n > 1 else 64, [st.offs[1]] if n > 1 else [])) == n
    flat = [[x for p in st.model.sizes for x in p] for st in rig.S]
    cut_at = [0, 128, 254, 255, 256]  # units the first round takes: in the middle of a tile, near its end, and exactly one tile
    specs = []
    for i, (st, n) in enumerate(zip(rig.S, items)):
        w = st.offs[-1] if n > 1 else 64
        specs.append((i, w, sum(flat[i][:cut_at[i]]) + (3 if cut_at[i] else flat[i][0] - 1), None))
    res = rig.round(specs, expect_code=E_CAPACITY)
    assert res[0].code == E_CAPACITY and [r.consumed for r in res[1:]] == [64 * k for k in cut_at[1:]]
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


# ---- 5. guard bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4", "snappy"])
def test_guard_bands_at_sixteen_alignments(ctxs, dev, codec):
    bs = 1024
    sources = [make_source([bs + 3 * i, 0, 2 * bs + i, 5], 60 + i) for i in range(16)]
    rig = Rig(ctxs(codec), dev, codec, ADLER, sources, bs=bs, aligns=list(range(16)))
    specs = []
    for i, st in enumerate(rig.S):
        f = copy.deepcopy(st.model).feed(st.offs[-1], st.offs[1:], 1 << 40)
        specs.append((i, st.offs[-1], f.out_len + (i % 7) - 3, None))  # a few bytes above and below out_len
    res = rig.round(specs)
    assert any(r.parts_closed < 4 for r in res) and any(r.parts_closed == 4 for r in res)
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()


# ---- 6. source order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_sources_at_descending_addresses(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    rig = Rig(ctxs(codec), dev, codec, CRC, [make_source(shape_sizes(bs, i), 70 + i) for i in range(4)], bs=bs, src_descending=True)
    assert all(rig.S[i].d_src < rig.S[0].d_src for i in range(1, 4))
    rig.play(lambda i, s, p: 2 * bs + i, rig.bound_of)
    rig.finish()
    assert rig.batched_calls >= 2


# ---- 7. call-level refusals ---------------------------------------------------------------------------------------------------
def test_call_level_refusals(ctxs, dev):
    import s3shuffle

    ctx, other, refc = ctxs(LZ4)
    data, offs = make_source([5000, 100], 80)
    d_srcs, d_dst = [dev.upload(data), dev.upload(data)], dev.alloc(1 << 16)
    a, b = ctx.compress_stream(LZ4, ADLER), ctx.compress_stream(LZ4, ADLER)
    foreign, snappy, crc = other.compress_stream(LZ4, ADLER), ctx.compress_stream(SNAPPY, ADLER), ctx.compress_stream(LZ4, CRC)
    row = lambda s, k: (s, d_srcs[k], 5100, [5000, 5100], d_dst + k * 8192, 8192)  # noqa: E731
    for rows in ([row(a, 0), row(foreign, 1)], [row(a, 0), row(a, 1)], [row(a, 0), row(snappy, 1)], [row(a, 0), row(crc, 1)], [row(a, 0), row(None, 1)]):
        res = ctx.compress_stream_feed_batch(rows)
        assert ctx.last_compress_batch_code == E_INVALID and [r.code for r in res] == [NOT_RUN] * 2
        assert ctx.get_option(OPT_BATCH) == 0
        for s in (a, b, foreign, snappy, crc):
            assert (s.position, s.written) == (0, 0)
    lib = s3shuffle.load_library()
    assert lib.s3s_cstream_feed_batch_device(ctx._h, None, 2) == E_INVALID and lib.s3s_cstream_feed_batch(ctx._h, None, 2) == E_INVALID
    assert lib.s3s_cstream_feed_batch_device(ctx._h, None, -1) == E_INVALID
    assert lib.s3s_cstream_feed_batch_device(ctx._h, None, 0) == 0 and ctx.get_option(OPT_BATCH) == 0
    with pytest.raises(s3shuffle.CodecError):
        ctx.set_option(OPT_BATCH, 1)
    res = ctx.compress_stream_feed_batch([row(a, 0), row(b, 1)])  # the streams still work
    assert [r.code for r in res] == [0, 0] and ctx.get_option(OPT_BATCH) == 2
    for s in (a, b, foreign, snappy, crc):
        s.close(check=False)


# ---- 8. not batched, still equal to the twin ------------------------------------------------------------------------------------
def test_one_entry_goes_one_by_one(ctxs, dev):
    rig = Rig(ctxs(LZ4), dev, LZ4, ADLER, [make_source(shape_sizes(1024, 0), 90)], bs=1024)
    rig.play(lambda i, s, p: 1500, rig.bound_of)
    rig.finish()
    assert rig.batched_calls == 0


def test_codec_none_goes_one_by_one(ctxs, dev):
    rig = Rig(ctxs(NONE), dev, NONE, CRC, [make_source(shape_sizes(256, i), 91 + i) for i in range(3)])
    rig.play(lambda i, s, p: 300 + i, lambda i, s, w, n: 200)
    rig.finish()
    assert rig.batched_calls == 0


def test_streams_of_different_block_sizes_go_one_by_one(ctxs, dev):
    rig = Rig(ctxs(LZ4), dev, LZ4, ADLER, [make_source(shape_sizes(1024, i), 93 + i) for i in range(2)], bs=[1024, 2048])
    rig.play(lambda i, s, p: 3000, rig.bound_of)
    rig.finish()
    assert rig.batched_calls == 0


@pytest.mark.parametrize("codec", [LZ4, NONE], ids=["lz4", "none"])
def test_encrypted_streams_go_one_by_one_with_sliced_ivs(ctxs, dev, codec):
    import s3shuffle
    import spark_crypto_ref as scr

    c4 = ctxs(codec, 4)
    rig = Rig(c4[:3], dev, codec, ADLER, [make_source(shape_sizes(1024, i), 95 + i) for i in range(3)], bs=1024, key=KEY, plainc=c4[3])
    # a wrong IV count is refused before anything runs, with the streams unchanged and the array consumed
    rows = [(st.s, st.d_src, 2000, cu.ends_in_window(st.offs, 0, 0, 2000), rig.d_dst + st.dst_at, st.bound) for st in rig.S]
    right = sum(len(r[3]) + 1 for r in rows)
    for count in (right - 1, right + 1):
        rig.ctx.set_stream_ivs(np.zeros(16 * count, np.uint8))
        res = rig.ctx.compress_stream_feed_batch(rows)
        assert rig.ctx.last_compress_batch_code == E_INVALID and [r.code for r in res] == [NOT_RUN] * 3
        assert all((st.s.position, st.s.written) == (0, 0) for st in rig.S)
        res = rig.ctx.compress_stream_feed_batch(rows)  # consumed: the next call has no IVs at all
        assert rig.ctx.last_compress_batch_code == E_INVALID
    rig.play(lambda i, s, p: 1500 + 100 * i, rig.bound_of)
    rig.finish()
    assert rig.batched_calls == 0
    for st in rig.S:  # the image is Spark's: IV | AES-CTR of the plain image, partition by partition
        want_img, want_index, want_sums = scr.encrypt_map_output(st.plain[0], np.asarray(st.plain[1], np.int64), KEY, st.ivs.reshape(-1), ADLER)
        assert np.array_equal(np.concatenate(st.out), want_img) and st.sums == [int(x) for x in want_sums]
    assert isinstance(s3shuffle.CompressFeedEntry(), s3shuffle.CompressFeedEntry)


# ---- 9. host buffers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_host_buffers(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    rig = Rig(ctxs(codec), dev, codec, ADLER, [make_source(shape_sizes(bs, 3 * i), 100 + i) for i in range(3)], bs=bs, host=True)
    big = [max(x for p in st.model.sizes for x in p) for st in rig.S]
    rig.play(lambda i, s, p: 2 * bs + 7 * i, lambda i, s, w, n: [big[i] - 1, 2 * big[i] + 40][s % 2] if i else rig.bound_of(i, s, w, n))
    rig.finish()
    assert rig.batched_calls >= 2


# ---- 10. sixty-four streams ---------------------------------------------------------------------------------------------------
def test_sixty_four_streams_in_one_call(ctxs, dev):
    bs = 32768
    rig = Rig(ctxs(LZ4), dev, LZ4, CRC32C, [make_source([bs], 200 + i) for i in range(64)])
    res = rig.round([(i, bs, rig.S[i].bound, None) for i in range(64)])
    assert all(r.code == 0 and r.consumed == bs and r.parts_closed == 1 for r in res) and rig.ctx.get_option(OPT_BATCH) == 64
    rig.finish()


# ---- 11. other calls between rounds, then every image decoded back -------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_other_calls_between_rounds_and_round_trip(ctxs, dev, codec):
    bs = SHAPE_BS[codec]
    rig = Rig(ctxs(codec), dev, codec, ADLER, [make_source(shape_sizes(bs, i), 110 + i) for i in range(3)], bs=bs)
    other, ooffs = make_source([3000, 0, 4000], 120)
    want = rig.refc.compress_map_output(codec, ADLER, other, ooffs)
    rounds = 0
    while not all(rig.done(i) for i in range(3)):
        rounds += 1
        assert rounds < 100
        live = [i for i in range(3) if not rig.done(i)]
        rig.round([(i, min(bs + 100, rig.S[i].offs[-1] - rig.S[i].pos), rig.S[i].bound, None) for i in live])
        got = rig.ctx.compress_map_output(codec, ADLER, other, ooffs)  # a one-shot compress and a checksum call on the same context
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert np.array_equal(rig.ctx.checksum_ranges(CRC, other, ooffs), rig.refc.checksum_ranges(CRC, other, ooffs))
    rig.finish()
    for st in rig.S:
        img = np.concatenate(st.out)
        back = rig.ctx.decompress_range(codec, ADLER, img, np.asarray(st.ref[1], np.int64), np.asarray(st.sums, np.int64), dst_capacity=st.data.size)
        assert np.array_equal(back, st.data)


# ---- 12. large blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4-u32", "snappy-fragments"])
def test_large_blocks(ctxs, dev, codec):
    """128 KiB blocks: LZ4's 32-bit-table parse, and a Snappy chunk of two fragments as one unit"""
    bs = 128 << 10
    rig = Rig(ctxs(codec), dev, codec, CRC, [make_source([bs + 5000 * (i + 1), 0, 3 * bs], 130 + i) for i in range(2)], bs=bs, large=True)
    sizes = [st.model.sizes for st in rig.S]
    res = rig.round([(0, rig.S[0].offs[-1], rig.S[0].bound, None), (1, rig.S[1].offs[-1], sizes[1][0][0] + sizes[1][0][1] // 2, None)])
    assert res[0].parts_closed == 3 and (res[1].consumed, res[1].parts_closed) == (bs, 0) and rig.ctx.get_option(OPT_BATCH) == 2
    rig.play(lambda i, s, p: 1 << 30, rig.bound_of)
    rig.finish()
