"""GPU: the batched feed (s3s_dstream_feed_batch*: one window of each of several streams per call).  The judge everywhere is a
TWIN: the same streams opened on a second context and fed the same windows one by one with s3s_dstream_feed_device.  Compared
per entry and round: the status and every field of the result, the position, the bytes of dst between guard bands of 64 bytes
(which must be untouched; after S3S_OK nothing is written at or beyond out_len either), and at the end close()'s code and
the concatenated output against the source."""
import numpy as np
import pytest

import corpus
import stream_damage as sd
import stream_units as su
import stream_units_encrypted as sue
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_UNSUPPORTED, NOT_RUN = -1, -2, -3, -4, -6, -100
OPT_DECODE_VARIANT, OPT_ZSTD_COMPRESS = 5, 9
CANARY, GUARD = 0xA5, 64
WORDS = ("code", "consumed", "out_len", "need_comp", "need_dst", "bad_partition", "at_end")
REST = 1 << 40  # "the rest of the range" as a window length


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


def _concat(parts):
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return np.concatenate(parts).astype(np.uint8), offs


class Slots:
    """n destinations of cap_max bytes, each between two guard bands, in one device allocation"""

    def __init__(self, dev, n, cap_max):
        self.dev, self.n, self.cap_max = dev, n, cap_max
        self.stride = (cap_max + 2 * GUARD + 255) & ~255
        self.base = dev.alloc(n * self.stride)

    def dst(self, i):
        return self.base + i * self.stride + GUARD

    def wipe(self):
        self.dev.fill(self.base, CANARY, self.n * self.stride)

    def read(self):
        return self.dev.download(self.base, self.n * self.stride).reshape(self.n, self.stride)


class Side:
    """one context, its streams and their destinations"""

    def __init__(self, ctx, dev, specs, cap_max):
        import s3shuffle

        self.ctx, self.slots = ctx, Slots(dev, len(specs), cap_max)
        self.streams = [s3shuffle.DecodeStream(ctx, sp["codec"], sp["algo"], sp["index"], sp["sums"] if sp["algo"] else None, **sp.get("open", {}))
                        for sp in specs]

    def close(self):
        return [s.close(check=False) for s in self.streams]


def _words(r):
    return tuple(int(getattr(r, w)) for w in WORDS)


def _single(stream, d_comp, w, d_dst, cap):
    import s3shuffle

    try:
        return stream.feed_device(d_comp, w, d_dst, cap)
    except s3shuffle.CodecError:
        return stream.last_result


class Rig:
    """the batch side and its twin over the same images; one round = one batched feed against the same feeds one by one"""

    def __init__(self, gpu_codec, twin_codec, dev, specs, cap_max):
        self.dev, self.specs = dev, specs
        for sp in specs:
            if "d_img" not in sp:
                sp["d_img"] = dev.upload(np.ascontiguousarray(sp["img"], dtype=np.uint8))
        self.b, self.t = Side(gpu_codec, dev, specs, cap_max), Side(twin_codec, dev, specs, cap_max)
        self.out = [[] for _ in specs]
        self.rounds = 0

    def positions(self):
        return [s.position for s in self.b.streams]

    def round(self, windows, comp_at=None, host=False):
        """windows[i] = (window length, capacity) of stream i (the length is cut at what the range has left); comp_at[i]: a
        device address that holds the window instead of the image's own bytes -> the per-entry results"""
        n, specs, b, t = len(self.specs), self.specs, self.b, self.t
        pos = self.positions()
        assert pos == [s.position for s in t.streams]
        win = [(max(0, min(w, int(specs[i]["index"][-1]) - pos[i])), cap) for i, (w, cap) in enumerate(windows)]
        src = [specs[i]["d_img"] + pos[i] if comp_at is None else comp_at[i] for i in range(n)]
        b.slots.wipe()
        t.slots.wipe()
        if host:
            bufs = [np.full(cap + 2 * GUARD, CANARY, np.uint8) for _, cap in win]
            got = b.ctx.feed_streams([(b.streams[i], np.asarray(specs[i]["img"], np.uint8)[pos[i]:pos[i] + win[i][0]],
                                       bufs[i][GUARD:GUARD + win[i][1]], win[i][1]) for i in range(n)])
        else:
            got = b.ctx.feed_streams_device([(b.streams[i], src[i], win[i][0], b.slots.dst(i), win[i][1]) for i in range(n)])
        want = []
        for i in range(n):
            if host:
                tb = np.full(win[i][1] + 2 * GUARD, CANARY, np.uint8)
                try:
                    r = t.streams[i].feed(np.asarray(specs[i]["img"], np.uint8)[pos[i]:pos[i] + win[i][0]], tb[GUARD:GUARD + win[i][1]], win[i][1])
                except Exception:  # noqa: BLE001 - a CodecError: the struct the failing feed filled
                    r = t.streams[i].last_result
                want.append((r, tb))
            else:
                want.append((_single(t.streams[i], src[i], win[i][0], t.slots.dst(i), win[i][1]), None))
        first_bad = next((code for code, _ in got if code != 0), 0)
        assert b.ctx.last_batch_code == first_bad, (b.ctx.last_batch_code, [c for c, _ in got])
        rows_b, rows_t = (None, None) if host else (b.slots.read(), t.slots.read())
        for i in range(n):
            what = (self.rounds, i, pos[i], win[i])
            code, r = got[i]
            assert (code,) + _words(r)[1:] == _words(want[i][0]), (what, (code,) + _words(r)[1:], _words(want[i][0]))
            assert b.streams[i].position == t.streams[i].position, what
            cap = win[i][1]
            rb, rt = (bufs[i], want[i][1]) if host else (rows_b[i], rows_t[i])
            for row, side in ((rb, "batch"), (rt, "twin")):
                assert (row[:GUARD] == CANARY).all(), ("write in front of dst", side, what)
                assert (row[GUARD + cap:] == CANARY).all(), ("write behind dst_capacity", side, what)
            if code == 0:
                assert np.array_equal(rb[GUARD:GUARD + r.out_len], rt[GUARD:GUARD + r.out_len]), ("decoded bytes", what)
                assert (rb[GUARD + r.out_len:] == CANARY).all(), ("write at or beyond out_len", what)
                if r.out_len:
                    self.out[i].append(rb[GUARD:GUARD + r.out_len].copy())
        self.rounds += 1
        return got

    def finish(self, healthy=None):
        """close() gives the same code on both sides; the concatenated output of every healthy stream is its source"""
        cb, ct = self.b.close(), self.t.close()
        assert cb == ct, (cb, ct)
        for i, sp in enumerate(self.specs):
            if (healthy is None or i in healthy) and "data" in sp:
                assert cb[i] == 0, (i, cb[i])
                got = np.concatenate(self.out[i]) if self.out[i] else np.zeros(0, np.uint8)
                assert np.array_equal(got, sp["data"]), ("stream %d" % i, got.size, sp["data"].size)
        return cb


# ---- images: `corpus`, 4 KiB blocks, two or three partitions of 5 - 12 KiB --------------------------------------------------------
_IMG = {}


def _image(oracle, codec, algo, k):
    key = (codec, algo, k)
    if key not in _IMG:
        rng = np.random.default_rng(7000 + k)
        sizes = rng.integers(5 * 1024, 12 * 1024, 2 + k % 2)
        data, offs = _concat([corpus.chunk_corpus([3, 7, 0, 4, 5][(k + p) % 5], int(n), rng) for p, n in enumerate(sizes)])
        if codec == LZF:
            img, index, sums = oracle.compress_map_output(codec, algo, data, offs)
        else:
            img, index, sums = oracle.compress_map_output(codec, algo, data, offs, 4096)
        _IMG[key] = dict(codec=codec, algo=algo, data=data, img=np.asarray(img, np.uint8), index=np.asarray(index, np.int64), sums=sums,
                         units=su.units(codec, np.asarray(img, np.uint8).tobytes(), index))
    sp = dict(_IMG[key])
    sp.pop("d_img", None)
    return sp


def _umax(specs):
    return max(u[2] for sp in specs for u in sp["units"])


# ---- 1. equivalence ----------------------------------------------------------------------------------------------------------
def _draw(rng, umax):
    """a window length and a capacity, drawn independently of what the streams answer (so the CPU can replay the schedule)"""
    x, y = rng.random(), rng.random()
    w = 0 if x < 0.08 else 1 if x < 0.16 else 20 if x < 0.24 else int(rng.integers(1, 3000)) if x < 0.55 else REST
    cap = 0 if y < 0.08 else int(rng.integers(0, umax)) if y < 0.25 else umax if y < 0.35 else 4 * umax
    return w, cap


def _schedule(specs, seed, bound=2000):
    """the rounds of the seeded schedule, replayed here on the CPU with stream_units.expected_feed: every stream is at its end
    inside the bound"""
    rng, umax = np.random.default_rng(seed), _umax(specs)
    pos, rounds = [0] * len(specs), []
    while any(p < int(sp["index"][-1]) for p, sp in zip(pos, specs)):
        assert len(rounds) < bound, "the twin schedule does not end inside the bound"
        row = [_draw(rng, umax) for _ in specs]
        rounds.append(row)
        for i, sp in enumerate(specs):
            w = min(row[i][0], int(sp["index"][-1]) - pos[i])
            pos[i] += su.expected_feed(sp["units"], pos[i], w, row[i][1])[0]
    return rounds


def _equivalence(gpu_codec, twin_codec, oracle, dev, codec, algo, seed=11, host=False):
    specs = [_image(oracle, codec, algo, k) for k in range(5)]
    rounds = _schedule(specs, seed)
    rig = Rig(gpu_codec, twin_codec, dev, specs, 4 * _umax(specs))
    seen = set()
    for row in rounds + [[(REST, 4 * _umax(specs))] * 5]:  # (one more round: every stream is at its end already)
        for code, r in rig.round(row, host=host):
            seen.add(code)
    assert all(r.at_end == 1 for _, r in rig.round([(0, 0)] * 5, host=host))
    assert 0 in seen and E_CAPACITY in seen, seen
    rig.finish()
    return len(rounds)


@pytest.mark.parametrize("algo", [0, ADLER, CRC, CRC32C], ids=["nosum", "adler32", "crc32", "crc32c"])
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_equivalence(gpu_codec, twin_codec, oracle, dev, codec, algo):
    """five streams over five images; every round draws a window length (0, 1, 20, a few hundred bytes, the rest) and a capacity
    (0, below a unit, a unit, four units) per stream from a seeded generator, until every stream is at its end"""
    n = _equivalence(gpu_codec, twin_codec, oracle, dev, codec, algo)
    print("rounds:", n)


# ---- 2. every cut position, eight at a time -------------------------------------------------------------------------------------
def _cut_image(oracle, codec):
    if codec == LZ4:
        rng = np.random.default_rng(5)
        data, offs = _concat([corpus.chunk_corpus(3, 3 * 4096 - 100, rng), corpus.chunk_corpus(7, 2 * 4096 + 9, rng)])
        return (data, offs) + tuple(oracle.compress_map_output(LZ4, ADLER, data, offs, 4096)) + (ADLER,)
    if codec == SNAPPY:
        rng = np.random.default_rng(6)
        data, offs = _concat([corpus.chunk_corpus(3, 2 * 4096 + 5, rng), corpus.chunk_corpus(7, 4096 + 900, rng)])
        return (data, offs) + tuple(oracle.compress_map_output(SNAPPY, CRC, data, offs, 4096)) + (CRC,)
    return tuple(su.lzf_cut_image(oracle, CRC32C)) + (CRC32C,)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_every_cut_position_eight_at_a_time(gpu_codec, twin_codec, oracle, dev, codec):
    """the cut list of test_every_cut_position_*: entry i's first window ends at cut c_i, then the rest.  The eight first windows
    lie back to back in one device allocation: a kernel that read past window i would see window i + 1's valid header"""
    data, offs, img, index, sums, algo = _cut_image(oracle, codec)
    img = np.asarray(img, np.uint8)
    total = int(index[-1])
    ulist = su.units(codec, img.tobytes(), index)
    d_img = dev.upload(img)
    d_pack = dev.alloc(8 * total)
    cap = data.size + 64
    cuts = list(range(1, total))
    for g in range(0, len(cuts), 8):
        group = cuts[g:g + 8]
        specs = [dict(codec=codec, algo=algo, data=data, img=img, index=index, sums=sums, d_img=d_img) for _ in group]
        rig = Rig(gpu_codec, twin_codec, dev, specs, cap)
        packed = np.concatenate([img[:c] for c in group])
        dev.write(d_pack, packed)
        at = np.concatenate([[0], np.cumsum(group)])
        got = rig.round([(c, cap) for c in group], comp_at=[d_pack + int(at[i]) for i in range(len(group))])
        for c, (code, r) in zip(group, got):
            assert code == 0 and (r.consumed, r.out_len) == su.expected_feed(ulist, 0, c, cap), (c, code, r.consumed, r.out_len)
        got = rig.round([(REST, cap)] * len(group))
        assert all(code == 0 and r.at_end == 1 for code, r in got), group
        rig.finish()
        for side in (rig.b, rig.t):
            dev.release(side.slots.base)


# ---- 3. mixed fates in one batch ---------------------------------------------------------------------------------------------
def _bad_sums(sp, part):
    out = dict(sp)
    out["sums"] = np.array(sp["sums"], np.int64).copy()
    out["sums"][part] ^= 0x5A5A
    out.pop("data")
    return out


def test_mixed_fates_in_one_batch(gpu_codec, twin_codec, oracle, dev):
    """healthy neighbours get what they get alone next to: a stream at its end, one with a sticky error, one whose first unit does
    not fit, one with a wrong checksum in a partition whose last byte the window holds"""
    specs = [_image(oracle, LZ4, ADLER, 0), _image(oracle, LZ4, ADLER, 1), _bad_sums(_image(oracle, LZ4, ADLER, 2), 0), _image(oracle, LZ4, ADLER, 3),
             _bad_sums(_image(oracle, LZ4, ADLER, 4), 1), _image(oracle, LZ4, ADLER, 2)]
    big = 4 * 12 * 1024
    rig = Rig(gpu_codec, twin_codec, dev, specs, big)
    # before the batch: stream 1 is read to its end, stream 2 meets its wrong checksum (each side on its own)
    for side in (rig.b, rig.t):
        r = _single(side.streams[1], specs[1]["d_img"], int(specs[1]["index"][-1]), side.slots.dst(1), big)
        assert r.code == 0 and r.at_end == 1
        r = _single(side.streams[2], specs[2]["d_img"], int(specs[2]["index"][-1]), side.slots.dst(2), big)
        assert (r.code, r.bad_partition) == (E_CHECKSUM, 0)
    first_unit = specs[3]["units"][0][2]
    got = rig.round([(REST, big), (REST, big), (REST, big), (REST, first_unit - 1), (REST, big), (300, big)])
    codes = [c for c, _ in got]
    assert codes == [0, 0, E_CHECKSUM, E_CAPACITY, E_CHECKSUM, 0], codes
    assert got[1][1].at_end == 1 and got[1][1].consumed == 0
    assert got[2][1].bad_partition == 0 and got[4][1].bad_partition == 1
    assert got[3][1].need_dst == first_unit
    assert got[0][1].at_end == 1
    # the stream that did not fit stays usable, the sticky ones stick, the healthy ones go on
    got = rig.round([(0, 0), (0, 0), (REST, big), (REST, big), (REST, big), (REST, big)])
    assert [c for c, _ in got] == [0, 0, E_CHECKSUM, 0, E_CHECKSUM, 0]
    closed = rig.finish(healthy={0, 3, 5})
    assert closed[2] == closed[4] == E_CHECKSUM


def test_refused_snappy_claim_next_to_healthy_streams(gpu_codec, twin_codec, oracle, dev):
    """a Snappy chunk that claims more than 32 MiB: refused (S3S_E_UNSUPPORTED, nothing consumed, not sticky), its neighbours go on"""
    case = next(c for c in sd.cases(oracle) if c.codec == SNAPPY and c.cls == sd.OVERSIZED and c.claim > sd.K_MAX)
    _damaged_batch(gpu_codec, twin_codec, oracle, dev, case, 0, expect=E_UNSUPPORTED)


def test_corrupt_lz4_payload_sends_the_batch_one_by_one(gpu_codec, twin_codec, oracle, dev):
    """without partition checksums a flipped payload byte is met by the decoder: the batch's one decode status word comes back
    non-zero, nothing was committed, and the entries are fed one by one - the healthy ones get what they get alone"""
    specs = [_image(oracle, LZ4, 0, k) for k in range(3)]
    bad = dict(specs[1])
    img = bad["img"].copy()
    start, length, _ = bad["units"][1]
    img[start + 21 + (length - 21) // 2] ^= 0xFF  # inside the second frame's payload
    bad["img"] = img
    bad.pop("data")
    specs[1] = bad
    big = 4 * 12 * 1024
    rig = Rig(gpu_codec, twin_codec, dev, specs, big)
    got = rig.round([(REST, big)] * 3)
    assert [c for c, _ in got] == [0, E_BAD_FRAME, 0] and got[0][1].at_end == got[2][1].at_end == 1
    got = rig.round([(REST, big)] * 3)
    assert [c for c, _ in got] == [0, E_BAD_FRAME, 0]
    assert rig.finish(healthy={0, 2})[1] == E_BAD_FRAME


# ---- 4. damaged ranges -------------------------------------------------------------------------------------------------------------
AMPLE = 1 << 18


def _damaged_batch(gpu_codec, twin_codec, oracle, dev, c, algo, expect=None):
    """the damaged range as entry 2 of four, three healthy streams over its base image around it.  The "half" schedule: the first
    window of every stream is half of its range, the later ones the rest; a window grows to need_comp, dst to need_dst"""
    model = _MODEL.setdefault("m", sd.Model(oracle))
    base = c.image
    refs = np.array(model.ref_sums(base, algo), np.int64) if algo else None
    healthy = dict(codec=c.codec, algo=algo, img=np.frombuffer(base.img, np.uint8), index=np.array(base.index, np.int64), sums=refs)
    damaged = dict(codec=c.codec, algo=algo, img=np.frombuffer(c.img, np.uint8), index=np.array(c.index, np.int64), sums=refs)
    specs = [dict(healthy), dict(healthy), damaged, dict(healthy)]
    rig = Rig(gpu_codec, twin_codec, dev, specs, AMPLE)
    win = [int(sp["index"][-1]) // 2 for sp in specs]
    cap = [AMPLE // 4] * 4
    last, done = [None] * 4, [False] * 4
    for _ in range(64):
        got = rig.round([(0, 0) if done[i] else (win[i], cap[i]) for i in range(4)])
        for i, (code, r) in enumerate(got):
            if done[i]:
                continue
            last[i] = (code, r)
            if code == E_CAPACITY and r.need_dst <= AMPLE:
                cap[i] = r.need_dst
            elif code != 0 or r.at_end:
                done[i] = True  # (an error of its own, the end, or a unit larger than the test gives a destination for)
            elif r.consumed == 0:
                win[i] = r.need_comp
            else:
                win[i] = REST
        if all(done):
            break
    assert all(done), (c.name, last)
    for i in (0, 1, 3):
        assert last[i][0] == 0 and last[i][1].at_end == 1, (c.name, i, last[i][0])
    if expect is not None:
        assert last[2][0] == expect, (c.name, last[2][0])
    rig.round([(REST, AMPLE // 4)] * 4)  # what the next feed says: sticky errors stick, a refusal repeats
    rig.finish(healthy=())
    for side in (rig.b, rig.t):
        dev.release(side.slots.base)
    for sp in specs:
        dev.release(sp["d_img"])
    return last[2][0]


_MODEL = {}


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_damaged_ranges_as_entry_two_of_four(gpu_codec, twin_codec, oracle, dev, codec):
    """every tenth case of tests/stream_damage.py's list per codec, checksums on (CRC32 for the Snappy cut-position image, Adler32
    elsewhere)"""
    selected = [c for c in sd.cases(oracle) if c.codec == codec][::10]
    assert len(selected) >= 3
    codes = {}
    for c in selected:
        code = _damaged_batch(gpu_codec, twin_codec, oracle, dev, c, sd.CRC if c.image.crc else sd.ADLER)
        codes[code] = codes.get(code, 0) + 1
    print("final codes of the damaged entry:", sorted(codes.items()))
    assert any(code != 0 for code in codes)


# ---- 5. fallbacks and refusals ---------------------------------------------------------------------------------------------------
def _drain(rig, n, cap, first=3000):
    rig.round([(first, cap)] * n)
    for _ in range(8):
        got = rig.round([(REST, cap)] * n)
        if all(r.at_end for _, r in got):
            break
    assert all(r.at_end for _, r in got)
    rig.finish()


def test_streams_that_are_not_batched_equal_the_twin(gpu_codec, twin_codec, oracle, dev):
    """S3S_CODEC_NONE, Zstandard and encrypted streams are fed one by one inside the call"""
    rng = np.random.default_rng(77)
    parts = [corpus.chunk_corpus(3, 9000, rng), corpus.chunk_corpus(7, 7000, rng)]
    data, offs = _concat(parts)
    # S3S_CODEC_NONE
    img, index, sums = oracle.compress_map_output(NONE, CRC, data, offs)
    specs = [dict(codec=NONE, algo=CRC, data=data, img=np.asarray(img, np.uint8), index=index, sums=sums) for _ in range(3)]
    _drain(Rig(gpu_codec, twin_codec, dev, specs, 20000), 3, 20000)
    # Zstandard
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    try:
        img, index, sums = gpu_codec.compress_map_output(ZSTD, ADLER, data, offs)
    finally:
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)
    specs = [dict(codec=ZSTD, algo=ADLER, data=data, img=np.asarray(img, np.uint8), index=np.asarray(index, np.int64), sums=sums,
                  open=dict(window_log_max=20)) for _ in range(2)]
    _drain(Rig(gpu_codec, twin_codec, dev, specs, 1 << 17), 2, 1 << 17)
    # encrypted
    img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs, 4096)
    enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[16], sue.ivs_for(len(index) - 1, 5), algo=ADLER)
    gpu_codec.set_io_encryption(sue.KEYS[16])
    twin_codec.set_io_encryption(sue.KEYS[16])
    try:
        specs = [dict(codec=LZ4, algo=ADLER, data=data, img=np.asarray(enc, np.uint8), index=np.asarray(eidx, np.int64), sums=sums,
                      open=dict(encrypted=True)) for _ in range(2)]
        _drain(Rig(gpu_codec, twin_codec, dev, specs, 20000), 2, 20000)
    finally:
        gpu_codec.set_io_encryption(None)
        twin_codec.set_io_encryption(None)


def test_call_level_refusals_leave_every_stream_unchanged(gpu_codec, twin_codec, oracle, dev):
    import s3shuffle

    a, b = _image(oracle, LZ4, ADLER, 0), _image(oracle, LZ4, ADLER, 1)
    other_codec, other_algo = _image(oracle, SNAPPY, ADLER, 0), _image(oracle, LZ4, CRC, 0)
    d = {id(sp): dev.upload(sp["img"]) for sp in (a, b, other_codec, other_algo)}
    cap = 1 << 16
    d_dst = [dev.alloc(cap) for _ in range(3)]

    def stream(ctx, sp):
        return s3shuffle.DecodeStream(ctx, sp["codec"], sp["algo"], sp["index"], sp["sums"] if sp["algo"] else None)

    sa, sb, sc, sg, foreign = stream(gpu_codec, a), stream(gpu_codec, b), stream(gpu_codec, other_codec), stream(gpu_codec, other_algo), stream(twin_codec, a)
    try:
        def entry(s, sp, k):
            return (s, d[id(sp)], int(sp["index"][-1]), d_dst[k], cap)

        for what, entries, n in (("mixed codecs", [entry(sa, a, 0), entry(sc, other_codec, 1)], None),
                                 ("mixed checksum algorithms", [entry(sa, a, 0), entry(sg, other_algo, 1)], None),
                                 ("the same stream twice", [entry(sa, a, 0), entry(sb, b, 1), entry(sa, a, 2)], None),
                                 ("a stream of another context", [entry(sa, a, 0), entry(foreign, a, 1)], None),
                                 ("a null stream", [entry(sa, a, 0), (None, d[id(b)], 100, d_dst[1], cap)], None),
                                 ("n < 0", [entry(sa, a, 0), entry(sb, b, 1)], -1)):
            if n is None:
                got = gpu_codec.feed_streams_device(entries)
                assert gpu_codec.last_batch_code == E_INVALID, what
                assert [c for c, _ in got] == [NOT_RUN] * len(entries), (what, got)
            else:
                arr = (s3shuffle.codec.FeedEntry * 2)()
                for k, e in enumerate(entries):
                    arr[k].stream, arr[k].d_comp, arr[k].comp_len, arr[k].d_dst, arr[k].dst_capacity = e[0]._s, e[1], e[2], e[3], e[4]
                    arr[k].status = 0
                assert gpu_codec._lib.s3s_dstream_feed_batch_device(gpu_codec._h, arr, n) == E_INVALID, what
                assert [arr[k].status for k in range(2)] == [0, 0]  # (a negative count: the library does not know how many there are)
            assert [s.position for s in (sa, sb, sc, sg, foreign)] == [0] * 5, what
        assert gpu_codec.feed_streams_device([]) == [] and gpu_codec.last_batch_code == 0
        assert gpu_codec._lib.s3s_dstream_feed_batch_device(gpu_codec._h, None, 1) == E_INVALID
        assert gpu_codec._lib.s3s_dstream_feed_batch_device(None, None, 0) == E_INVALID
        # one-shot calls and single feeds on the same context between two batched feeds
        got = gpu_codec.feed_streams_device([(sa, d[id(a)], 3000, d_dst[0], cap), (sb, d[id(b)], 3000, d_dst[1], cap)])
        assert [c for c, _ in got] == [0, 0] and got[0][1].consumed > 0
        assert gpu_codec.decompress_range_device(LZ4, ADLER, d[id(b)], int(b["index"][-1]), b["index"], b["sums"], d_dst[2], cap) == b["data"].size
        assert np.array_equal(dev.download(d_dst[2], b["data"].size), b["data"])
        mid = sa.feed_device(d[id(a)] + sa.position, 2000, d_dst[2], cap)
        assert mid.code == 0
        out_a = [dev.download(d_dst[0], got[0][1].out_len).copy(), dev.download(d_dst[2], mid.out_len).copy()]
        out_b = [dev.download(d_dst[1], got[1][1].out_len).copy()]
        got = gpu_codec.feed_streams_device([(sa, d[id(a)] + sa.position, int(a["index"][-1]) - sa.position, d_dst[0], cap),
                                             (sb, d[id(b)] + sb.position, int(b["index"][-1]) - sb.position, d_dst[1], cap)])
        assert [c for c, _ in got] == [0, 0] and got[0][1].at_end == got[1][1].at_end == 1
        out_a.append(dev.download(d_dst[0], got[0][1].out_len))
        out_b.append(dev.download(d_dst[1], got[1][1].out_len))
        assert np.array_equal(np.concatenate(out_a), a["data"]) and np.array_equal(np.concatenate(out_b), b["data"])
        assert sa.close(check=False) == 0 and sb.close(check=False) == 0
    finally:
        for s in (sa, sb, sc, sg, foreign):
            s.close(check=False)


# ---- 6. both decode variants -------------------------------------------------------------------------------------------------------
def test_ring_decoder_variant(gpu_codec, twin_codec, oracle, dev):
    """S3S_OPT_LZ4_DECODE_VARIANT = 3: the batch's decode launch is the decoder the option names"""
    default = gpu_codec.get_option(OPT_DECODE_VARIANT)
    for c in (gpu_codec, twin_codec):
        c.set_option(OPT_DECODE_VARIANT, 3)
    try:
        for codec in (LZ4, SNAPPY):
            _equivalence(gpu_codec, twin_codec, oracle, dev, codec, CRC, seed=12)
    finally:
        for c in (gpu_codec, twin_codec):
            c.set_option(OPT_DECODE_VARIANT, default)


# ---- 7. host buffers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_host_buffers(gpu_codec, twin_codec, oracle, dev, codec):
    """s3s_dstream_feed_batch against single s3s_dstream_feed calls, guard bytes around the host destination"""
    _equivalence(gpu_codec, twin_codec, oracle, dev, codec, ADLER, seed=13, host=True)


# ---- 8. width ----------------------------------------------------------------------------------------------------------------------
def test_sixty_four_streams(gpu_codec, twin_codec, oracle, dev):
    """64 streams with 64 KiB windows over one 16-partition image each: more windows than a workgroup has wavefronts in one
    segmented-cut launch, several pieces per window"""
    rng = np.random.default_rng(88)
    specs = []
    for k in range(4):  # four images, sixteen streams over each
        data, offs = _concat([corpus.chunk_corpus([3, 7, 0, 4][(k + p) % 4], int(n), rng) for p, n in enumerate(rng.integers(6000, 14000, 16))])
        img, index, sums = oracle.compress_map_output(LZ4, ADLER, data, offs)
        sp = dict(codec=LZ4, algo=ADLER, data=data, img=np.asarray(img, np.uint8), index=np.asarray(index, np.int64), sums=sums)
        sp["d_img"] = dev.upload(sp["img"])
        specs += [dict(sp) for _ in range(16)]
    cap = 1 << 16
    rig = Rig(gpu_codec, twin_codec, dev, specs, cap)
    for n in range(64):
        got = rig.round([(65536, cap if (i + n) % 3 else cap // 2) for i in range(64)])
        if all(r.at_end for _, r in got):
            break
    assert all(r.at_end for _, r in got) and n >= 2
    rig.finish()
