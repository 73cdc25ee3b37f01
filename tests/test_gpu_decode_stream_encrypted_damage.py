"""GPU: the damaged ranges of tests/stream_damage.py, encrypted by the reference layer, through s3s_dstream_open_encrypted by a
caller that follows the contract (tests/stream_damage_encrypted.py: the contract model's prediction translated by the IV-unit
mapping).  Checksums off, feed_device, three of the 18 schedules (a window that ends behind the damaged field with ample
capacity; the whole range with the damaged unit's claimed size - 1; one byte at a time with exactly the capacity in front of
the damaged unit).

Thinned within classes: every third case of every (codec, class) in the fixed order - every class of the model kept, at least
a third of each class's cases.  KEPT pins the counts (of 458 cases: 157).

For every run: termination within 5 x (stored units + 1) feeds; every feed's code, consumed, out_len, need_comp, need_dst and
at_end and its decoded bytes are the model's; S3S_E_BAD_FRAME sticks (the next feed and close() repeat it, nothing consumed),
S3S_E_UNSUPPORTED is a refusal (nothing consumed, close() says the range was not read to its end); dst lies between two canary
bands, the upper one starting where dst_capacity ends: 4 KiB next to dst are read after every feed, both whole bands at the
end of every run."""
import numpy as np
import pytest

import stream_damage as sd
import stream_damage_encrypted as sde
from hipdev import Dev

pytestmark = pytest.mark.gpu

LZ4, SNAPPY, LZF = sd.LZ4, sd.SNAPPY, sd.LZF
BAND, NEAR, CANARY = 1 << 16, 4096, 0xA5
KEPT = {
    "lz4": {sd.HEADER_INVALID: 32, sd.TRUNCATED: 14, sd.PAYLOAD_INVALID: 13, sd.OVERSIZED: 2, sd.VALID_DIFFERENT: 2},
    "snappy": {sd.HEADER_INVALID: 20, sd.TRUNCATED: 9, sd.PAYLOAD_INVALID: 12, sd.OVERSIZED: 10, sd.VALID_DIFFERENT: 15},
    "lzf": {sd.HEADER_INVALID: 9, sd.TRUNCATED: 10, sd.PAYLOAD_INVALID: 8, sd.OVERSIZED: 0, sd.VALID_DIFFERENT: 1},
}


def test_kept_counts(oracle):
    """(no GPU work) the thinning keeps every class and at least a third of each class's cases"""
    kept = sd.counts(sde.thinned(oracle))
    assert kept == KEPT
    for codec, row in sd.counts(sd.cases(oracle)).items():
        for cls, n in row.items():
            assert 3 * KEPT[codec][cls] >= n and (KEPT[codec][cls] > 0) == (n > 0), (codec, cls, n)


@pytest.fixture(scope="module")
def rig(gpu_codec, oracle):
    d = Dev()
    size = 2 * BAND + sd.K_MAX
    base = d.alloc(size)
    d.fill(base, CANARY, size)
    gpu_codec.set_io_encryption(sde.KEY)
    yield dict(dev=d, dst=base + BAND, model=sd.Model(oracle))
    gpu_codec.set_io_encryption(None)
    d.free()


def _bands(rig, cap, n, what):
    dev, dst = rig["dev"], rig["dst"]
    assert np.all(dev.download(dst - n, n) == CANARY), ("write in front of dst", what)
    assert np.all(dev.download(dst + cap, n) == CANARY), ("write behind dst_capacity", what)


def _run(gpu_codec, rig, e, sched):
    import s3shuffle

    dev, dst = rig["dev"], rig["dst"]
    d_img = dev.upload(e.img)
    s = s3shuffle.DecodeStream(gpu_codec, e.c.codec, 0, e.eidx, encrypted=True)

    def one(pos, w, cap):
        try:
            x = s.feed_device(d_img + pos, w, dst, cap)
        except s3shuffle.CodecError as err:
            x = s.last_result
            assert x.code == err.code
        assert 0 <= x.out_len <= cap and 0 <= x.consumed <= w
        r = dict(code=x.code, consumed=x.consumed, out_len=x.out_len, need_comp=x.need_comp, need_dst=x.need_dst, at_end=x.at_end,
                 bad=x.bad_partition, data=dev.download(dst, x.out_len).tobytes() if x.out_len else b"")
        _bands(rig, cap, NEAR, (e.c.name, sched, pos, w, cap))
        if x.out_len or x.code not in (0, sd.E_CAPACITY):
            dev.fill(dst, CANARY, cap if x.code else x.out_len)  # (a failing feed may have written anywhere inside dst_capacity)
        return r

    def feed(st, pos, w, cap):
        assert s.position == pos
        r = one(pos, w, cap)
        st["pos"] = s.position
        return r

    try:
        trace, data = sde.run(e, sched, feed, 5 * (e.n_units + 1))
        pos, w, cap, last = trace[-1]
        if last["code"] not in (0, sd.E_CAPACITY):  # what the next feed says
            again = one(pos, w, cap)
            assert (again["code"], again["consumed"], again["out_len"]) == (last["code"], 0, 0), (e.c.name, sched, again)
            assert s.position == pos
        _bands(rig, cap, BAND, (e.c.name, sched, "end of the run"))
    finally:
        rc = s.close(check=False)
        dev.release(d_img)
    return trace, data, rc


PARAMS = [(codec, cls) for codec in (LZ4, SNAPPY, LZF) for cls in sd.CLASSES if not (codec == LZF and cls == sd.OVERSIZED)]
WORDS = ("code", "consumed", "out_len", "need_comp", "need_dst", "at_end", "bad")


@pytest.mark.parametrize("codec,cls", PARAMS, ids=["%s-%s" % (sd.CODEC_NAME[a], b) for a, b in PARAMS])
def test_feed_device(gpu_codec, oracle, rig, codec, cls):
    selected = [c for c in sde.thinned(oracle) if c.codec == codec and c.cls == cls]
    assert len(selected) == KEPT[sd.CODEC_NAME[codec]][cls] > 0
    model, runs, feeds, codes = rig["model"], 0, 0, {}
    for c in selected:
        e = sde.EncCase(c)
        for where, cap_mode in sde.SCHEDULES:
            sched = next(x for x in sd.schedules(c) if x.where == where and x.cap_mode == cap_mode)
            want, want_data = sde.run(e, sched, lambda st, pos, w, cap: sde.feed(model, e, st, w, cap), 5 * (e.n_units + 1))
            trace, data, closed = _run(gpu_codec, rig, e, sched)
            what = (c.name, cls, sched)
            for i, ((pos, w, cap, r), (xpos, xw, xcap, x)) in enumerate(zip(trace, want)):
                got_words, exp_words = (pos, w, cap) + tuple(r[k] for k in WORDS), (xpos, xw, xcap) + tuple(x[k] for k in WORDS)
                assert got_words == exp_words, ("feed %d" % i, what, got_words, exp_words)
                assert r["data"] == x["data"], ("decoded bytes of feed %d" % i, what)
                assert r["need_dst"] <= sd.K_MAX and (r["code"] == 0 or r["consumed"] == r["out_len"] == 0), (what, r)
            assert len(trace) == len(want) and data == want_data, (what, len(trace), len(want))
            last = trace[-1][3]
            assert closed == (sd.E_BAD_FRAME if last["code"] == sd.E_BAD_FRAME or not last["at_end"] else 0), (what, closed)
            if cls == sd.VALID_DIFFERENT:  # without checksums such a range decodes to the oracle's bytes and reaches the end
                assert last["code"] == 0 and last["at_end"] == 1, what
            runs, feeds = runs + 1, feeds + len(trace)
            codes[last["code"]] = codes.get(last["code"], 0) + 1
    print("encrypted feed_device %s %s: %d runs, %d feeds, final codes %s" % (sd.CODEC_NAME[codec], cls, runs, feeds, sorted(codes.items())))
