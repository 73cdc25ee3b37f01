"""GPU: the batched feed over streams under IO encryption (s3s_dstream_open_encrypted in s3s_dstream_feed_batch*).  The rig is
tests/test_gpu_decode_stream_batch.py's: the judge is a TWIN - the same streams opened on a second context under the same key
and fed the same windows one by one - compared per entry and round in status, every result word, position, the bytes of dst
between guard bands, and at the end close()'s code and the concatenated output against the source.  Stored images come from
the reference layer (tests/stream_units_encrypted.encrypt), never from the code under test.

Beyond the twin: after every batched round the read-only option key 17 (S3S_OPT_DSTREAM_BATCH_ENTRIES) must hold the number
of entries that were real windows of the batch - an entry with a sticky error, an empty window or a stale key is answered by
the single feed inside the call and is not counted.  A library that feeds encrypted streams one by one does not have the key
(S3S_E_INVALID), so these tests fail on it."""
import numpy as np
import pytest

import corpus
import spark_crypto_ref as scr
import stream_damage as sd
import stream_damage_encrypted as sde
import stream_units as su
import stream_units_encrypted as sue
import test_gpu_decode_stream_batch as tb
import test_gpu_decode_stream_encrypted as te
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, LZF = 0, 1, 2, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_UNSUPPORTED, NOT_RUN = -1, -2, -3, -4, -6, -100
OPT_BATCH_ENTRIES = 17
REST = tb.REST
STICKY = (E_CHECKSUM, E_BAD_FRAME)


@pytest.fixture(scope="module")
def twin_codec(gpu_codec):
    import s3shuffle

    c = s3shuffle.Codec(0)
    yield c
    c.close()


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def keyed(gpu_codec, twin_codec):
    """-> set(key): the same key on both contexts; the layer is off again when the test ends, whichever way"""
    def set_key(key):
        gpu_codec.set_io_encryption(key)
        twin_codec.set_io_encryption(key)

    yield set_key
    set_key(None)


class Rig(tb.Rig):
    """tb.Rig whose rounds also check key 17"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.sticky = set()   # streams whose error sticks: the single feed answers them inside the call
        self.stale = set()    # streams bound to an earlier key setting

    def round(self, windows, expect_entries=None, decoder_may_judge=(), **kw):
        """decoder_may_judge: entries whose S3S_E_BAD_FRAME may be the DECODER's (a corrupt payload): the batch's one decode status
        word then sends the undecided entries through the single feed, and key 17 counts only what the batch decided before"""
        pos = self.positions()
        live = [i for i, (w, _) in enumerate(windows)
                if i not in self.sticky and i not in self.stale and min(w, int(self.specs[i]["index"][-1]) - pos[i]) > 0]
        got = super().round(windows, **kw)
        want = (len(live) if len(windows) > 1 else 0) if expect_entries is None else expect_entries
        have = self.b.ctx.get_option(OPT_BATCH_ENTRIES)
        if any(got[i][0] == E_BAD_FRAME for i in decoder_may_judge):
            assert 0 <= have <= want, ("key 17", self.rounds - 1, have, want)
        else:
            assert have == want, ("key 17", self.rounds - 1, have, want)
        for i, (code, _) in enumerate(got):
            if code in STICKY:
                self.sticky.add(i)
        return got


def _spec(codec, algo, kb, data, img, index, seed, iv_only=()):
    """a plain image under the reference layer -> what tb.Side opens"""
    enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[kb], sue.ivs_for(len(index) - 1, seed), iv_only=iv_only, algo=algo)
    return dict(codec=codec, algo=algo, data=data, img=np.asarray(enc, np.uint8), index=np.asarray(eidx, np.int64), sums=sums,
                units=sue.stored_units(codec, np.asarray(img, np.uint8).tobytes(), eidx), open=dict(encrypted=True))


def _image(oracle, codec, algo, kb, k):
    """tb._image (two or three partitions of 5 - 12 KiB, 4 KiB blocks), stored under the layer"""
    p = tb._image(oracle, codec, 0, k)
    return _spec(codec, algo, kb, p["data"], p["img"], p["index"], 900 + 7 * k + kb)


# ---- 1. equivalence ----------------------------------------------------------------------------------------------------------
# the product codec x checksum x key length, thinned to a Latin square: every codec with every checksum, every codec and every
# checksum with every key length
EQ = [(codec, algo, (16, 24, 32)[(ci + algo) % 3]) for ci, codec in enumerate((LZ4, SNAPPY, LZF)) for algo in (0, ADLER, CRC, CRC32C)]


def _equivalence(gpu_codec, twin_codec, oracle, dev, keyed, codec, algo, kb, seed=21, host=False):
    keyed(sue.KEYS[kb])
    specs = [_image(oracle, codec, algo, kb, k) for k in range(5)]
    rounds = tb._schedule(specs, seed)  # seeded window and capacity draws, replayed on the CPU over the STORED units
    cap_max = 4 * tb._umax(specs)
    rig = Rig(gpu_codec, twin_codec, dev, specs, cap_max)
    seen = set()
    for row in rounds + [[(REST, cap_max)] * 5]:
        for code, r in rig.round(row, host=host):
            seen.add(code)
    assert all(r.at_end == 1 for _, r in rig.round([(0, 0)] * 5, host=host))
    assert 0 in seen and E_CAPACITY in seen, seen
    rig.finish()
    return len(rounds)


@pytest.mark.parametrize("codec,algo,kb", EQ, ids=["%s-%s-aes%d" % ({1: "lz4", 2: "snappy", 4: "lzf"}[c], ("nosum", "adler32", "crc32", "crc32c")[a], 8 * k)
                                                  for c, a, k in EQ])
def test_equivalence(gpu_codec, twin_codec, oracle, dev, keyed, codec, algo, kb):
    """five encrypted streams; every round draws a window length (0, 1, 20, a few hundred bytes, the rest) and a capacity (0,
    below a unit, a unit, four units) per stream from a seeded generator, until every stream is at its end"""
    assert gpu_codec.get_option(OPT_BATCH_ENTRIES) >= 0, "the library has no key 17: encrypted streams are not batched"
    print("rounds:", _equivalence(gpu_codec, twin_codec, oracle, dev, keyed, codec, algo, kb))


def test_key_17_is_read_only(gpu_codec):
    import s3shuffle

    with pytest.raises(s3shuffle.CodecError) as e:
        gpu_codec.set_option(OPT_BATCH_ENTRIES, 1)
    assert e.value.code == E_INVALID and gpu_codec.get_option(OPT_BATCH_ENTRIES) >= 0


# ---- 2. every cut position, eight at a time -------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_every_cut_position_eight_at_a_time(gpu_codec, twin_codec, oracle, dev, keyed, codec):
    """the small encrypted images of the single feed's every-cut test (at most 12 KB; a window end on every byte of every IV):
    entry i's window is [0, c_i), eight windows packed back to back in one allocation, so a pass that read or decrypted past
    window i would meet window i + 1.  Capacities 0, 1, one below a unit and a unit: all four at every cut within 17 bytes of a
    partition's start and at every unit's two ends, one of the four - rotating - at the others.  The judge here is the unit
    list (su.expected_feed over the stored units) and the source bytes: a twin would double the feeds of 12 000 cuts."""
    data, enc, eidx, sums, ulist, algo, kb = te._cut_image(oracle, codec)
    keyed(sue.KEYS[kb])
    import s3shuffle

    enc = np.asarray(enc, np.uint8)
    total = int(eidx[-1])
    unit = max(u[2] for u in ulist)
    caps = (0, 1, unit - 1, unit)
    near = set()
    for p in range(len(eidx) - 1):
        near.update(range(int(eidx[p]) - 1, int(eidx[p]) + 18))
    for s, ln, _ in ulist:
        near.update((s - 1, s, s + 1, s + ln - 1, s + ln, s + ln + 1))
    jobs = []
    for c in range(1, total):
        jobs += [(c, cap) for cap in caps] if c in near else [(c, caps[c % 4])]
    d_pack = dev.alloc(8 * total)
    slots = tb.Slots(dev, 8, unit)
    for g in range(0, len(jobs), 8):
        group = jobs[g:g + 8]
        streams = [s3shuffle.DecodeStream(gpu_codec, codec, algo, eidx, sums, encrypted=True) for _ in group]
        dev.write(d_pack, np.concatenate([enc[:c] for c, _ in group]))
        at = np.concatenate([[0], np.cumsum([c for c, _ in group])])
        slots.wipe()
        got = gpu_codec.feed_streams_device([(streams[i], d_pack + int(at[i]), c, slots.dst(i), cap) for i, (c, cap) in enumerate(group)])
        assert gpu_codec.get_option(OPT_BATCH_ENTRIES) == (len(group) if len(group) > 1 else 0), group
        rows = slots.read()
        for i, ((c, cap), (code, r)) in enumerate(zip(group, got)):
            # (from the start of a range the first unit is an IV, which fits any capacity: S3S_E_CAPACITY cannot be the answer)
            want = su.expected_feed(ulist, 0, c, cap)
            assert code == 0 and (r.consumed, r.out_len) == want, (c, cap, code, (r.consumed, r.out_len), want)
            assert streams[i].position == r.consumed
            assert np.array_equal(rows[i][tb.GUARD:tb.GUARD + r.out_len], data[:r.out_len]), (c, cap)
            if r.consumed == 0:
                assert c < 16 and r.need_comp == 16, (c, cap, r.need_comp)  # less than the first IV
            assert (rows[i][:tb.GUARD] == tb.CANARY).all() and (rows[i][tb.GUARD + r.out_len:] == tb.CANARY).all(), ("write outside dst[0, out_len)", c, cap)
        for s in streams:
            s.close(check=False)


# ---- 3. mixed fates in one call ------------------------------------------------------------------------------------------------
def _snappy_parts(oracle, sizes, seed):
    rng = np.random.default_rng(seed)
    data, offs = tb._concat([corpus.chunk_corpus([3, 7, 0, 4][p % 4], n, rng) if n else np.zeros(0, np.uint8) for p, n in enumerate(sizes)])
    img, index, _ = oracle.compress_map_output(SNAPPY, 0, data, offs, 4096)
    return data, np.asarray(img, np.uint8), [int(x) for x in index]


def test_mixed_fates_in_one_call(gpu_codec, twin_codec, oracle, dev, keyed):
    """ten Snappy streams with Adler32 under AES-128 in ONE call, each with a fate of its own; every entry equals the twin, and
    the healthy ones at both ends of the array get what they get alone"""
    keyed(sue.KEYS[16])
    big = 1 << 16
    d0, i0, x0 = _snappy_parts(oracle, [6000, 5000], 1)
    d1, i1, x1 = _snappy_parts(oracle, [0, 0, 7000, 0], 2)
    healthy = lambda seed: _spec(SNAPPY, ADLER, 16, d0, i0, x0, seed)  # noqa: E731
    specs = [healthy(1), healthy(2), _spec(SNAPPY, ADLER, 16, d1, i1, x1, 3), healthy(4)]
    # 4: a partition of 7 stored bytes between two good ones, with the checksums of the bytes as stored
    base = healthy(5)
    e, x = base["img"], [int(v) for v in base["index"]]
    simg = np.concatenate([e[:x[1]], e[x[1]:x[1] + 7], e[x[1]:]])
    sidx = np.array([0, x[1], x[1] + 7, x[1] + 7 + (x[2] - x[1])], np.int64)
    specs.append(dict(codec=SNAPPY, algo=ADLER, img=simg, index=sidx, sums=scr.checksums(simg, sidx, ADLER), open=dict(encrypted=True)))
    specs.append(tb._bad_sums(healthy(6), 0))  # 5: a wrong checksum in a partition whose last byte the window holds
    specs.append(healthy(7))                   # 6: S3S_E_CAPACITY
    # 7: a chunk that claims more than any decoder takes: refused, nothing consumed, not sticky
    case = next(c for c in sd.cases(oracle) if c.codec == SNAPPY and c.cls == sd.OVERSIZED and c.claim > sd.K_MAX)
    cimg, cidx, csums = sue.encrypt(np.frombuffer(case.img, np.uint8), case.index, sue.KEYS[16], sue.ivs_for(len(case.index) - 1, 8), algo=ADLER)
    specs.append(dict(codec=SNAPPY, algo=ADLER, img=np.asarray(cimg, np.uint8), index=cidx, sums=csums, open=dict(encrypted=True)))
    specs.append(tb._bad_sums(healthy(9), 0))  # 8: a sticky error from an earlier feed
    specs.append(healthy(10))
    rig = Rig(gpu_codec, twin_codec, dev, specs, big)
    first_chunk = next(u for u in specs[6]["units"] if u[2] > 0)
    for side in (rig.b, rig.t):  # before the call, each side on its own
        r = tb._single(side.streams[1], specs[1]["d_img"], int(specs[1]["index"][-1]), side.slots.dst(1), big)
        assert r.code == 0 and r.at_end == 1
        r = tb._single(side.streams[6], specs[6]["d_img"], first_chunk[0], side.slots.dst(6), big)  # the IV and the stream header
        assert r.code == 0 and r.consumed == first_chunk[0] == 32 and r.out_len == 0
        r = tb._single(side.streams[8], specs[8]["d_img"], int(specs[8]["index"][-1]), side.slots.dst(8), big)
        assert (r.code, r.bad_partition) == (E_CHECKSUM, 0)
    rig.sticky.add(8)
    got = rig.round([(REST, big), (REST, big), (0, big), (7, big), (REST, big), (REST, big), (REST, first_chunk[2] - 1), (REST, big), (REST, big), (300, big)])
    codes = [c for c, _ in got]
    assert codes == [0, 0, 0, 0, E_BAD_FRAME, E_CHECKSUM, E_CAPACITY, E_UNSUPPORTED, E_CHECKSUM, 0], codes
    assert gpu_codec.get_option(OPT_BATCH_ENTRIES) == 7  # all but the one at its end, the empty window and the sticky one
    assert got[0][1].at_end == 1 and got[1][1].at_end == 1 and got[1][1].consumed == 0
    assert rig.b.streams[2].position == 0 and got[2][1].need_comp == 16  # the empty partitions are passed, the next unit is an IV
    assert (got[3][1].consumed, got[3][1].need_comp) == (0, 16)        # less than an IV
    assert got[5][1].bad_partition == 0 and got[8][1].bad_partition == 0
    assert got[6][1].need_dst == first_chunk[2]
    assert got[9][1].consumed > 0
    # the refused one and the one without room stay usable, the sticky ones stick, the healthy ones go on
    got = rig.round([(0, 0), (0, 0), (REST, big), (REST, big), (REST, big), (REST, big), (REST, big), (REST, big), (REST, big), (REST, big)])
    assert [c for c, _ in got] == [0, 0, 0, 0, E_BAD_FRAME, E_CHECKSUM, 0, E_UNSUPPORTED, E_CHECKSUM, 0]
    closed = rig.finish(healthy={0, 2, 3, 6, 9})  # (stream 1 handed its bytes out before the call)
    assert (closed[4], closed[5], closed[8]) == (E_BAD_FRAME, E_CHECKSUM, E_CHECKSUM)


def test_corrupt_lz4_payload_sends_the_batch_one_by_one(gpu_codec, twin_codec, oracle, dev, keyed):
    """without checksums a flipped cipher byte of a payload is met by the decoder: the batch's one decode status word comes back
    non-zero, nothing was committed, and the undecided entries are fed one by one.  Key 17 counts what the batch decided itself:
    the entry whose first unit did not fit had its answer before the decode"""
    keyed(sue.KEYS[24])
    specs = [_image(oracle, LZ4, 0, 24, k) for k in range(4)]
    bad = dict(specs[1])
    img = bad["img"].copy()
    start, length, _ = [u for u in bad["units"] if u[2] > 0][1]
    img[start + 21 + (length - 21) // 2] ^= 0xFF  # inside the second frame's payload
    bad["img"] = img
    bad.pop("data")
    specs[1] = bad
    big = 4 * 12 * 1024
    rig = Rig(gpu_codec, twin_codec, dev, specs, big)
    for side in (rig.b, rig.t):  # stream 3 stands behind its IV: a unit that does not fit is S3S_E_CAPACITY there
        assert tb._single(side.streams[3], specs[3]["d_img"], 16, side.slots.dst(3), big).consumed == 16
    got = rig.round([(REST, big), (REST, big), (REST, big), (REST, 5)], expect_entries=1)
    assert [c for c, _ in got] == [0, E_BAD_FRAME, 0, E_CAPACITY] and got[0][1].at_end == got[2][1].at_end == 1
    got = rig.round([(REST, big)] * 4)
    assert [c for c, _ in got] == [0, E_BAD_FRAME, 0, 0]
    assert rig.finish(healthy={0, 2, 3})[1] == E_BAD_FRAME


# ---- 4. the IV carried across rounds -----------------------------------------------------------------------------------------
def test_iv_carry_across_three_rounds(gpu_codec, twin_codec, oracle, dev, keyed):
    """a partition of nine LZ4 blocks stays open across three rounds: its IV arrives in round one - for one stream in a window that
    ends exactly behind it - and every later window's key stream starts at another residue of a block"""
    keyed(sue.KEYS[32])
    rng = np.random.default_rng(41)
    data, offs = tb._concat([corpus.chunk_corpus(3, 9 * 4096 - 77, rng), corpus.chunk_corpus(7, 4096 + 5, rng)])
    img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs, 4096)
    specs = [_spec(LZ4, CRC, 32, data, img, index, 50 + k) for k in range(3)]
    ends = [u[0] + u[1] for u in specs[0]["units"]]  # the same for all three: the IV, then nine frames, ...
    assert ends[0] == 16 and int(specs[0]["index"][1]) > ends[8]
    big = 1 << 16
    rig = Rig(gpu_codec, twin_codec, dev, specs, big)
    plan = [[ends[1], 16, ends[2] + 5], [ends[3] - ends[1] + 9, ends[2] - 16, ends[4] - ends[2]], [ends[5] - ends[3], ends[6] - ends[2] + 1, ends[7] - ends[4]]]
    residues = set()
    for rnd, row in enumerate(plan):
        pos = rig.positions()
        if rnd:
            assert all(16 <= p < int(specs[0]["index"][1]) for p in pos)  # partition 0 is open, its IV is the stream's
            residues.update((p - 16) % 16 for p in pos)
        got = rig.round([(w, big) for w in row])
        assert all(code == 0 and r.consumed > 0 for code, r in got), (rnd, [(c, r.consumed) for c, r in got])
        if rnd == 0:
            assert (got[1][1].consumed, got[1][1].out_len) == (16, 0)  # the window ended exactly behind the IV
    assert len(residues) >= 3, sorted(residues)
    got = rig.round([(REST, big)] * 3)
    assert all(code == 0 and r.at_end == 1 for code, r in got)
    rig.finish()


# ---- 5. the key epoch ----------------------------------------------------------------------------------------------------------
def test_streams_of_an_earlier_key_setting_are_refused_per_entry(gpu_codec, twin_codec, oracle, dev, keyed):
    keyed(sue.KEYS[16])
    old = [_image(oracle, SNAPPY, CRC, 16, k) for k in range(2)]
    new = [_image(oracle, SNAPPY, CRC, 24, k) for k in range(2)]
    big = 1 << 16
    rig_old = Rig(gpu_codec, twin_codec, dev, old, big)
    got = rig_old.round([(3000, big)] * 2)
    assert [c for c, _ in got] == [0, 0]
    keyed(sue.KEYS[24])
    rig = Rig(gpu_codec, twin_codec, dev, old + new, big)  # (fresh streams over the old images would decode garbage: replace them)
    for side, side_old in ((rig.b, rig_old.b), (rig.t, rig_old.t)):
        for i in range(2):
            side.streams[i].close(check=False)
            side.streams[i] = side_old.streams[i]
    rig.stale = {0, 1}
    pos = rig.positions()
    got = rig.round([(REST, big)] * 4)
    assert [c for c, _ in got] == [E_INVALID, E_INVALID, 0, 0] and rig.positions()[:2] == pos[:2]
    assert gpu_codec.get_option(OPT_BATCH_ENTRIES) == 2
    assert got[2][1].at_end == got[3][1].at_end == 1
    rig.finish(healthy={2, 3})


# ---- 6. fallbacks --------------------------------------------------------------------------------------------------------------
def test_fallbacks_read_zero(gpu_codec, twin_codec, oracle, dev, keyed):
    """encrypted S3S_CODEC_NONE, n == 1 and a call-level refusal: the call's answers are the twin's and key 17 reads 0"""
    keyed(sue.KEYS[16])
    big = 1 << 16
    lz = [_image(oracle, LZ4, ADLER, 16, k) for k in range(2)]
    rig = Rig(gpu_codec, twin_codec, dev, lz, big)
    rig.round([(3000, big)] * 2)
    assert gpu_codec.get_option(OPT_BATCH_ENTRIES) == 2
    # S3S_CODEC_NONE
    rng = np.random.default_rng(78)
    data, offs = tb._concat([rng.integers(0, 256, n, dtype=np.uint8) for n in (900, 0, 700)])
    img, index, _ = oracle.compress_map_output(NONE, 0, data, offs)
    none = [dict(_spec(NONE, CRC, 16, data, img, index, 60 + k), units=None) for k in range(2)]
    rig_none = Rig(gpu_codec, twin_codec, dev, none, big)
    for row in ([(500, 300)] * 2, [(REST, big)] * 2):
        rig_none.round(row, expect_entries=0)
    rig_none.finish()
    rig.round([(2000, big)] * 2)
    assert gpu_codec.get_option(OPT_BATCH_ENTRIES) == 2
    # n == 1
    one = Rig(gpu_codec, twin_codec, dev, [_image(oracle, LZ4, ADLER, 16, 2)], big)
    one.round([(REST, big)], expect_entries=0)
    one.finish()
    rig.round([(100, big)] * 2)
    # a call-level refusal: the same stream twice
    pos = rig.positions()
    sa, sb = rig.b.streams
    got = gpu_codec.feed_streams_device([(sa, lz[0]["d_img"] + pos[0], 500, rig.b.slots.dst(0), big), (sb, lz[1]["d_img"] + pos[1], 500, rig.b.slots.dst(1), big),
                                         (sa, lz[0]["d_img"] + pos[0], 500, rig.b.slots.dst(0), big)])
    assert gpu_codec.last_batch_code == E_INVALID and [c for c, _ in got] == [NOT_RUN] * 3
    assert gpu_codec.get_option(OPT_BATCH_ENTRIES) == 0 and rig.positions() == pos
    got = rig.round([(REST, big)] * 2)
    assert all(r.at_end for _, r in got)
    rig.finish()


# ---- 7. damaged ranges ---------------------------------------------------------------------------------------------------------
_MODEL = {}
AMPLE = 1 << 18
WORDS = ("code", "consumed", "out_len", "need_comp", "need_dst", "at_end")


def _damaged_batch(gpu_codec, twin_codec, oracle, dev, c):
    """the damaged range, encrypted, as entry 2 of four, three healthy streams over its base image around it (checksums off, as
    the contract model of tests/stream_damage_encrypted.py predicts).  The first window of every stream is half of its range,
    the later ones the rest; a window grows to need_comp, dst to need_dst.  Entry 2's words are the model's, round by round"""
    model = _MODEL.setdefault("m", sd.Model(oracle))
    e = sde.EncCase(c)
    base = c.image
    benc, bidx, _ = sue.encrypt(np.frombuffer(base.img, np.uint8), base.index, sde.KEY, sue.ivs_for(len(base.index) - 1, 3))
    healthy = dict(codec=c.codec, algo=0, img=np.asarray(benc, np.uint8), index=np.asarray(bidx, np.int64), sums=None, open=dict(encrypted=True))
    damaged = dict(codec=c.codec, algo=0, img=np.asarray(e.img, np.uint8), index=np.asarray(e.eidx, np.int64), sums=None, open=dict(encrypted=True))
    specs = [dict(healthy), dict(healthy), damaged, dict(healthy)]
    rig = Rig(gpu_codec, twin_codec, dev, specs, AMPLE)
    st = dict(pos=0, plain=dict(pos=0, cur=0, err=0, bad=-1))
    win = [int(sp["index"][-1]) // 2 for sp in specs]
    cap = [AMPLE // 4] * 4
    last, done = [None] * 4, [False] * 4
    for _ in range(64):
        pos2 = st["pos"]
        got = rig.round([(0, 0) if done[i] else (win[i], cap[i]) for i in range(4)], decoder_may_judge=(2,))
        if not done[2]:
            want = sde.feed(model, e, st, max(0, min(win[2], e.total - pos2)), cap[2])
            code, r = got[2]
            assert (code,) + tuple(int(getattr(r, k)) for k in WORDS[1:]) == tuple(want[k] for k in WORDS), (c.name, pos2, win[2], cap[2], want)
            assert rig.b.streams[2].position == st["pos"], c.name
        for i, (code, r) in enumerate(got):
            if done[i]:
                continue
            last[i] = (code, r)
            if code == E_CAPACITY and r.need_dst <= AMPLE:
                cap[i] = r.need_dst
            elif code != 0 or r.at_end:
                done[i] = True
            elif r.consumed == 0:
                win[i] = r.need_comp
            else:
                win[i] = REST
        if all(done):
            break
    assert all(done), (c.name, last)
    for i in (0, 1, 3):
        assert last[i][0] == 0 and last[i][1].at_end == 1, (c.name, i, last[i][0])
    rig.round([(REST, AMPLE // 4)] * 4)  # what the next feed says: sticky errors stick, a refusal repeats
    rig.finish(healthy=())
    for side in (rig.b, rig.t):
        dev.release(side.slots.base)
    for sp in specs:
        dev.release(sp["d_img"])
    return last[2][0]


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_damaged_ranges_as_entry_two_of_four(gpu_codec, twin_codec, oracle, dev, keyed, codec):
    """every tenth case of tests/stream_damage.py's list per codec, stored under the layer"""
    keyed(sde.KEY)
    selected = [c for c in sd.cases(oracle) if c.codec == codec][::10]
    assert len(selected) >= 3
    codes = {}
    for c in selected:
        code = _damaged_batch(gpu_codec, twin_codec, oracle, dev, c)
        codes[code] = codes.get(code, 0) + 1
    print("final codes of the damaged entry:", sorted(codes.items()))
    assert any(code != 0 for code in codes)


# ---- 8. host buffers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,algo,kb", [(LZ4, CRC32C, 16), (SNAPPY, ADLER, 32), (LZF, CRC, 24)], ids=["lz4", "snappy", "lzf"])
def test_host_buffers(gpu_codec, twin_codec, oracle, dev, keyed, codec, algo, kb):
    """s3s_dstream_feed_batch against single s3s_dstream_feed calls, guard bytes around the host destination"""
    _equivalence(gpu_codec, twin_codec, oracle, dev, keyed, codec, algo, kb, seed=23, host=True)


# ---- 9. width ----------------------------------------------------------------------------------------------------------------------
def test_sixty_four_streams(gpu_codec, twin_codec, oracle, dev, keyed):
    """64 encrypted streams in one call with windows of 1 KiB .. 64 KiB: more windows than a workgroup has wavefronts, windows of
    one decrypt tile next to windows of four, several pieces (and IVs) per window"""
    keyed(sue.KEYS[16])
    rng = np.random.default_rng(89)
    specs = []
    for k in range(4):  # four images, sixteen streams over each
        data, offs = tb._concat([corpus.chunk_corpus([3, 7, 0, 4][(k + p) % 4], int(n), rng) for p, n in enumerate(rng.integers(6000, 14000, 16))])
        img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs)
        sp = _spec(LZ4, ADLER, 16, data, img, index, 70 + k)
        sp["d_img"] = dev.upload(sp["img"])
        specs += [dict(sp) for _ in range(16)]
    cap = 1 << 16
    rig = Rig(gpu_codec, twin_codec, dev, specs, cap)
    for n in range(200):
        got = rig.round([(1024 << ((i + n) % 7), cap if (i + n) % 3 else cap // 2) for i in range(64)])
        if all(r.at_end for _, r in got):
            break
    assert all(r.at_end for _, r in got) and n >= 2
    rig.finish()
