"""GPU: damaged ranges (tests/stream_damage.py) through s3s_dstream_* by a caller that follows the contract - it grows the
window to need_comp and dst to need_dst on S3S_E_CAPACITY - against the contract model and the one-shot call.  The cases and
schedules are the ones tests/test_isa_decode_stream_damage.py has put through the compiled kernels on the CPU (covered()).

For every case, schedule and checksum setting:
  termination   the caller ends within 5 x (units + 1) feeds: a feed consumes a unit, raises need_comp at most three times in a
                row, or answers S3S_E_CAPACITY once per unit
  bytes         what was handed out before the error is the oracle's decode of a prefix of whole valid units; a
                `valid-different` range without checksums decodes to the oracle's bytes and reaches at_end
  code          one code per (case, schedule), the model's: S3S_E_BAD_FRAME, or S3S_E_CHECKSUM with the damaged partition when
                the failing feed's window holds that partition's last byte; S3S_E_UNSUPPORTED for a unit that claims more than
                kBatchMaxBlock.  BAD_FRAME and CHECKSUM stick: the next feed and close() repeat them with the same partition.
                UNSUPPORTED is a refusal: nothing is consumed, the same feed gets the same answer, close() says the range was
                not read to its end
  bounds        need_comp <= the bytes left in the range (LZ4) / in the open partition (Snappy, LZF); need_dst <= kBatchMaxBlock
                and, when reported, the claimed decoded size of the unit at the position
  guard bands   dst lies in one device allocation with 1 MiB of a canary pattern on each side, the upper band starting where
                dst_capacity ends.  Nothing but a stray write changes the bytes outside [dst, dst + dst_capacity) - the test
                re-fills only that region - so a stray write stays until it is read: 4 KiB next to dst are read after every
                feed, and both whole bands after the first feed at a capacity, before the first feed at another capacity
                (at the old one: the larger dst would cover the old band) and at the end of every run
  parity        the one-shot call on the same bytes: success -> every schedule succeeds with the same bytes; code X -> X, except
                (a) where it says S3S_E_CHECKSUM and the failing feed's window does not hold the damaged partition's last byte:
                a stream cannot know the checksum of a partition that is still open, and answers what it does without
                checksums; (b) where it says S3S_E_CAPACITY because the range claims more decoded bytes than the 32 MiB + 256 KiB
                the test gives it (no 4 GiB allocation on a shared card for a claim of 2^32 - 1): the claim is above
                kBatchMaxBlock and the stream's answer is S3S_E_UNSUPPORTED
A feed that raises still fills its s3s_dstream_result (DecodeStream.last_result): consumed, out_len, need_comp, need_dst and
at_end of a failing feed are read from the library, not assumed."""
import numpy as np
import pytest

import stream_damage as sd
import test_isa_decode_stream_damage as cpu
from hipdev import Dev

pytestmark = pytest.mark.gpu

LZ4, SNAPPY, LZF = sd.LZ4, sd.SNAPPY, sd.LZF
OPT_DECODE_VARIANT = 5
BAND, NEAR, CANARY = 1 << 20, 4096, 0xA5
AMPLE = 1 << 18


class Guarded:
    """[1 MiB canary][dst, up to kBatchMaxBlock][1 MiB canary]: the upper band starts where the feed's capacity ends"""

    def __init__(self, dev):
        self.dev, self.size = dev, 2 * BAND + sd.K_MAX
        self.base = dev.alloc(self.size)
        dev.fill(self.base, CANARY, self.size)
        self.dst = self.base + BAND
        self.band = np.full(BAND, CANARY, np.uint8)

    def check(self, cap, whole, what):
        n = BAND if whole else NEAR
        lo = self.dev.download(self.dst - n, n)
        hi = self.dev.download(self.dst + cap, n)
        assert np.array_equal(lo, self.band[:n]), ("write in front of dst", what)
        assert np.array_equal(hi, self.band[:n]), ("write behind dst_capacity", what, int(np.flatnonzero(hi != CANARY)[0]))

    def wipe(self, cap):
        self.dev.fill(self.dst, CANARY, cap)


@pytest.fixture(scope="module")
def rig(gpu_codec, oracle):
    d = Dev()
    g = Guarded(d)
    yield dict(dev=d, g=g, model=sd.Model(oracle), img={}, one={})
    d.free()


def _upload(rig, c):
    if c.name not in rig["img"]:
        rig["img"][c.name] = rig["dev"].upload(np.frombuffer(c.img, np.uint8))
    return rig["img"][c.name]


def _algos(c):
    return (0, sd.CRC if c.image.crc else sd.ADLER)


def _one_shot(gpu_codec, rig, c, algo, d_big, big_cap):
    """s3s_decompress_range_device on the damaged range, with a destination as large as the range claims -> (code, partition, bytes)"""
    import s3shuffle

    refs = rig["model"].ref_sums(c.image, algo) if algo else None
    try:
        n = gpu_codec.decompress_range_device(c.codec, algo, _upload(rig, c), c.index[-1], c.index, refs, d_big, big_cap)
    except s3shuffle.CodecError as e:
        return e.code, e.partition, b""
    assert n <= AMPLE
    return 0, -1, rig["dev"].download(d_big, n).tobytes()


def _run(gpu_codec, rig, c, sched, algo, host=False, want=()):
    """the model's caller (Model.run) with the product's stream behind it -> (trace, bytes, the code close() gave)"""
    import s3shuffle

    dev, g, model = rig["dev"], rig["g"], rig["model"]
    d_img = _upload(rig, c)
    refs = model.ref_sums(c.image, algo) if algo else None
    state = rig.setdefault("state", dict(cap=None))  # (the capacity of the previous feed, of whichever run)
    s = s3shuffle.DecodeStream(gpu_codec, c.codec, algo, c.index, refs)

    def one(pos, w, cap, i=-1):
        r = dict(code=0, consumed=0, out_len=0, need_comp=0, need_dst=0, at_end=0, bad=-1, data=b"")
        if not host and state["cap"] not in (None, cap):
            g.check(state["cap"], True, (c.name, sched, algo, pos, "before the capacity changes"))
        try:
            if host:
                buf = np.full(cap + 2 * NEAR, CANARY, np.uint8)
                x = s.feed(np.frombuffer(c.img, np.uint8)[pos:pos + w], buf[NEAR:NEAR + cap], cap)
            else:
                x = s.feed_device(d_img + pos, w, g.dst, cap)
        except s3shuffle.CodecError as e:
            x = s.last_result  # (the struct the failing feed filled)
            assert x.code == e.code and x.bad_partition == e.partition, (c.name, sched, x.code, e.code)
        if True:
            r.update(code=x.code, consumed=x.consumed, out_len=x.out_len, need_comp=x.need_comp, need_dst=x.need_dst, at_end=x.at_end,
                     bad=x.bad_partition)
            assert 0 <= x.out_len <= cap and 0 <= x.consumed <= w
            if host:
                r["data"] = buf[NEAR:NEAR + x.out_len].tobytes()
            elif x.out_len:
                r["data"] = dev.download(g.dst, x.out_len).tobytes()
        if host:
            assert (buf[:NEAR] == CANARY).all() and (buf[NEAR + cap:] == CANARY).all(), ("write outside the host dst", c.name, sched, pos)
        else:
            g.check(cap, state["cap"] != cap, (c.name, sched, algo, pos, w, cap))
            if r["code"] == sd.E_CHECKSUM and 0 <= i < len(want) and not want[i][4]["decoded"]:  # the verdict came before any decode
                assert (dev.download(g.dst, min(cap, 1 << 16)) == CANARY).all(), ("decoded in the feed that reports the checksum", c.name, sched, pos)
            if r["out_len"] or r["code"] not in (0, sd.E_CAPACITY):
                g.wipe(cap)  # (a failing feed may have written inside [0, dst_capacity))
        state["cap"] = cap
        return r

    calls = []

    def feed(st, pos, w, cap):
        r = one(pos, w, cap, len(calls))
        calls.append(pos)
        st["pos"] = s.position
        return r

    try:
        trace, data = model.run(c, sched, algo, feed=feed, max_feeds=5 * (len(sd.su.units(c.codec, c.image.img, c.image.index)) + 1))
        pos, _, w, cap, last = trace[-1]
        if last["code"] not in (0, sd.E_CAPACITY):  # what the next feed says, and close()
            again = one(pos, w, cap)
            assert (again["code"], again["bad"], again["consumed"], again["out_len"]) == (last["code"], last["bad"], 0, 0), (c.name, sched, again)
        if not host:
            g.check(cap, True, (c.name, sched, algo, "end of the run"))
    finally:
        rc = s.close(check=False)
    return trace, data, rc


def _left(c, pos):
    """the bytes left in the range (LZ4) / in the partition that holds pos (Snappy, LZF)"""
    if c.codec == LZ4:
        return c.index[-1] - pos
    return next((e for e in c.index[1:] if e > pos), c.index[-1]) - pos


def _check_run(gpu_codec, rig, c, sched, algo, one_shot, host=False):
    model = rig["model"]
    want_trace, want_data = model.run(c, sched, algo)
    trace, data, closed = _run(gpu_codec, rig, c, sched, algo, host, want_trace)
    what = (c.name, c.cls, sched, algo, "host" if host else "device")
    for pos, _, w, cap, r in trace:  # bounds first: they hold whatever the model says
        assert r["need_comp"] <= _left(c, pos), ("need_comp beyond the bytes that are left", what, pos, r)
        assert r["need_dst"] <= sd.K_MAX, ("need_dst beyond the largest block a decoder takes", what, pos, r)
        if r["code"] != 0:
            assert r["consumed"] == r["out_len"] == 0, (what, r)
    words = ("code", "consumed", "out_len", "need_comp", "need_dst", "at_end", "bad", "data")
    got = [(pos, w, cap) + tuple(r[k] for k in words) for pos, _, w, cap, r in trace]
    exp = [(pos, w, cap) + tuple(r[k] for k in words) for pos, _, w, cap, r in want_trace]
    for i, (a, b) in enumerate(zip(got, exp)):
        assert a[:-1] == b[:-1], ("feed %d" % i, what, a[:-1], b[:-1])
        assert a[-1] == b[-1], ("decoded bytes of feed %d" % i, what)
    assert len(got) == len(exp), (what, len(got), len(exp))
    rig["runs"], rig["feeds"] = rig.get("runs", 0) + 1, rig.get("feeds", 0) + len(got)
    rig["codes"] = rig.get("codes", {})
    rig["codes"][trace[-1][4]["code"]] = rig["codes"].get(trace[-1][4]["code"], 0) + 1
    assert data == want_data
    last = trace[-1][4]
    code = last["code"]
    assert closed == (code if code in (sd.E_BAD_FRAME, sd.E_CHECKSUM) else 0 if last["at_end"] else sd.E_BAD_FRAME), (what, closed)
    # the partitions in front of the damaged one are verified, and delivered once the position has passed them
    if code == sd.E_CHECKSUM:
        assert last["bad"] == c.image.part, (what, last)
    if trace[-1][0] >= c.image.index[c.image.part]:
        front = model.front_bytes(c)
        assert data[:len(front)] == front, what
    # parity with the one-shot call
    o_code, o_part, o_data = one_shot
    if o_code == 0:
        assert code == 0 and last["at_end"] == 1 and data == o_data, ("the one-shot call decodes this range", what, code)
    elif o_code == sd.E_CAPACITY:
        claimed = _claimed(model.oracle, c)
        assert claimed is not None and claimed > sd.K_MAX + AMPLE and c.claim > sd.K_MAX and code == sd.E_UNSUPPORTED, (
            "the one-shot call says the range claims more than it was given", what, claimed, code)
    elif code != o_code:
        pos, _, w, _, _ = trace[-1]
        pend = c.index[o_part + 1] if o_part >= 0 else -1
        assert o_code == sd.E_CHECKSUM and pos + w < pend and code == model.run(c, sched, 0)[0][-1][4]["code"], (
            "the one-shot call says %d" % o_code, what, code)
    elif code == sd.E_CHECKSUM:
        assert last["bad"] == o_part, (what, last["bad"], o_part)


def _cases(oracle, codec, cls):
    """the cases the CPU file has put through the compiled code, each with all of its schedules"""
    return [(c, every) for c, _, every in cpu.covered(oracle) if c.codec == codec and c.cls == cls]


def _big(rig, oracle, selected):
    """the destination of the one-shot call: as large as the largest range claims to decode to, up to kBatchMaxBlock + 256 KiB"""
    cap = sd.K_MAX + AMPLE
    return rig["dev"].alloc(cap), cap


def _claimed(oracle, c):
    """the decoded bytes the damaged range claims, unit by unit (None: its chain breaks)"""
    units, _, _, verdict = sd.Model(oracle, bound=False).walk(c.codec, c.img, c.index, 0, c.index[-1])
    return sum(u[2] for u in units) if verdict is None else None


PARAMS = [(codec, cls, k) for codec in (LZ4, SNAPPY, LZF) for cls in sd.CLASSES if not (codec == LZF and cls == sd.OVERSIZED)
          for k in (0, 1)]


@pytest.mark.parametrize("codec,cls,k", PARAMS, ids=["%s-%s-%s" % (sd.CODEC_NAME[a], b, ("nosum", "sum")[k]) for a, b, k in PARAMS])
def test_feed_device(gpu_codec, oracle, rig, codec, cls, k):
    """every case of the class at every schedule: six window ends x three capacities; k: checksums off / on (CRC32 for the
    Snappy cut-position image, Adler32 elsewhere)"""
    selected = _cases(oracle, codec, cls)
    assert selected
    d_big, big_cap = _big(rig, oracle, selected)
    try:
        for c, scheds in selected:
            algo = _algos(c)[k]
            one = _one_shot(gpu_codec, rig, c, algo, d_big, big_cap)
            for s in scheds:
                _check_run(gpu_codec, rig, c, s, algo, one)
    finally:
        rig["dev"].release(d_big)
        _report(rig, "feed_device %s %s %s" % (sd.CODEC_NAME[codec], cls, ("nosum", "sum")[k]))


def _report(rig, what):
    print("%s: %d runs, %d feeds, final codes %s" % (what, rig.pop("runs", 0), rig.pop("feeds", 0), sorted(rig.pop("codes", {}).items())))


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_feed_host_buffers(gpu_codec, oracle, rig, codec):
    """the host-buffer feed on a thinned list: every third case, the whole range in one window and the unit-at-a-time caller,
    ample capacity, checksums on"""
    selected = [(c, s) for k, (c, _, s) in enumerate(cpu.covered(oracle)) if c.codec == codec and k % 3 == 0]
    d_big, big_cap = _big(rig, oracle, selected)
    try:
        for c, scheds in selected:
            algo = _algos(c)[1]
            one = _one_shot(gpu_codec, rig, c, algo, d_big, big_cap)
            for s in scheds:
                if s.where in ("whole", "unit-at-a-time") and s.cap_mode == "ample":
                    _check_run(gpu_codec, rig, c, s, algo, one, host=True)
    finally:
        rig["dev"].release(d_big)


def test_lz4_payload_cases_through_the_ring_decoder(gpu_codec, oracle, rig):
    """S3S_OPT_LZ4_DECODE_VARIANT = 3 (test_feed_device runs the default, 4): the same answers"""
    default = gpu_codec.get_option(OPT_DECODE_VARIANT)
    assert default == 4
    selected = _cases(oracle, LZ4, sd.PAYLOAD_INVALID)
    d_big, big_cap = _big(rig, oracle, selected)
    gpu_codec.set_option(OPT_DECODE_VARIANT, 3)
    try:
        for c, scheds in selected:
            assert max(c.claim, c.image.block) <= 32768  # (the ring decoder keeps 32 KiB blocks: every case is within them)
            for algo in _algos(c):
                one = _one_shot(gpu_codec, rig, c, algo, d_big, big_cap)
                for s in scheds:
                    _check_run(gpu_codec, rig, c, s, algo, one)
    finally:
        gpu_codec.set_option(OPT_DECODE_VARIANT, default)
        rig["dev"].release(d_big)
