"""CPU: damaged ranges (tests/stream_damage.py) through the stream-mode discovery and the capacity cut of the reduce side,
COMPILED for gfx950 and run in the instruction interpreter (tests/isa/stream_kernel.py), against the contract model.

Every feed that the model's caller makes for a `header-invalid`, `truncated` or `oversized-claim` case is replayed: the window's
buffer ends with the window's last byte, so a header parse that looks past it is a fault of the interpreter's memory.  The
`payload-invalid` cases go through the compiled decoders (tests/isa/decode_kernel.py) with a destination of exactly the
claimed size.  This file is the gate of tests/test_gpu_decode_stream_damage.py: covered() is the list the hardware gets.

The class totals below are written down, not measured by the test: a change of the generator or of the model shows here."""
import os
import sys

import pytest

import stream_damage as sd

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa"))
import decode_kernel as dk  # noqa: E402
import stream_kernel as sk  # noqa: E402

LZ4, SNAPPY, LZF = sd.LZ4, sd.SNAPPY, sd.LZF
CODECS = pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])

# cases per codec and class (tests/stream_damage.py: cases())
TOTALS = {
    "lz4": {"header-invalid": 95, "truncated": 40, "payload-invalid": 37, "oversized-claim": 5, "valid-different": 5},
    "snappy": {"header-invalid": 59, "truncated": 26, "payload-invalid": 35, "oversized-claim": 30, "valid-different": 44},
    "lzf": {"header-invalid": 25, "truncated": 30, "payload-invalid": 24, "oversized-claim": 0, "valid-different": 3},
}


@pytest.fixture(scope="module")
def model(oracle):
    return sd.Model(oracle)


GATED = (sd.HEADER_INVALID, sd.TRUNCATED, sd.OVERSIZED)


def cpu_schedules(c, i):
    """The schedules of case number i that this file replays.  The interpreter runs ~10^4 times slower than the hardware and
    all 18 schedules (six window ends x three capacities) of all 458 cases take 165 s, against a budget of three times
    tests/test_isa_decode_stream.py (3 x 39 s), so the product is thinned on the schedule side; the mutation list is whole:
    `header-invalid`, `truncated` and `oversized-claim` cases keep every window end with two of the three capacities (window
    end w of case i leaves out capacity (i + w) mod 3; a Snappy `oversized-claim` case leaves out none), `payload-invalid`
    and `valid-different` cases, whose discovery answers status 0 throughout, keep every other window end (those with i + w
    even) with capacity (i + w) mod 3."""
    full = sd.schedules(c)
    n = len(sd.CAP_MODES)
    if c.cls == sd.OVERSIZED and c.codec == SNAPPY:
        return full
    if c.cls in GATED:
        return [full[w * n + m] for w in range(len(sd.WHERE)) for m in range(n) if m != (i + w) % n]
    return [full[w * n + (i + w) % n] for w in range(len(sd.WHERE)) if (i + w) % 2 == 0]


def covered(oracle):
    """[(case, the schedules run here, all of its schedules)] in the fixed order.  The gate of the hardware tests is the case:
    every case passes through compiled code in this file - test_discovery_and_cut replays every discovery and capacity cut of
    the schedules run here, test_payload_invalid_units_through_the_decoders puts the damaged unit of every `payload-invalid`
    case through the compiled decoder - and the hardware then takes all of its schedules.  The decode of the units around the
    damage, the checksums and the host code run on the hardware only."""
    return [(c, cpu_schedules(c, i), sd.schedules(c)) for i, c in enumerate(sd.cases(oracle))]


# ---- the model itself ------------------------------------------------------------------------------------------------------------
def test_every_case_is_classified_and_the_totals_are_the_written_ones(oracle):
    cases = sd.cases(oracle)
    assert all(c.cls in sd.CLASSES for c in cases) and len({c.name for c in cases}) == len(cases)
    assert sd.counts(cases) == TOTALS
    assert sum(sum(row.values()) for row in TOTALS.values()) == len(cases) == 458


def test_every_class_is_populated_for_every_codec(oracle):
    """oversized-claim is empty for LZF and has to be: a chunk's decoded size is a 16-bit field, 65535 < kBatchMaxBlock."""
    got = sd.counts(sd.cases(oracle))
    for codec, row in got.items():
        for cls, n in row.items():
            assert (n > 0) != (codec == "lzf" and cls == sd.OVERSIZED), (codec, cls, n)
    assert 0xFFFF < sd.K_MAX


def test_mutations_touch_what_they_record(oracle):
    for c in sd.cases(oracle):
        lo, hi = c.span
        base = c.image.img
        diff = [k for k in range(min(len(base), len(c.img))) if base[k] != c.img[k]]
        assert all(lo <= k < hi for k in diff), (c.name, lo, hi, diff[:4])
        assert diff or c.index != c.image.index, c.name
        assert c.unit[0] <= lo < c.unit[0] + c.unit[1], (c.name, c.unit, c.span)


@CODECS
def test_the_model_agrees_with_the_oracle_on_whole_ranges(oracle, model, codec):
    """the sequential walk against the oracle's own range decoder: the same verdict, and the same bytes where both decode"""
    import numpy as np

    for c in (x for x in sd.cases(oracle) if x.codec == codec):
        rc, out, _ = oracle.decompress_range(codec, 0, np.frombuffer(c.img, np.uint8), np.array(c.index, np.int64), None, 1 << 18)
        trace, data = model.run(c, sd.Schedule("whole", c.index[-1], "ample"), 0)
        code = trace[-1][4]["code"]
        if c.cls == sd.OVERSIZED:  # the oracle has no block limit: it runs out of the 256 KiB, or decodes, or objects to the payload
            assert rc in (sd.E_CAPACITY, sd.E_BAD_FRAME) and code in (sd.E_UNSUPPORTED, sd.E_BAD_FRAME), (c.name, rc, code)
        else:
            assert rc == code == (0 if c.cls == sd.VALID_DIFFERENT else sd.E_BAD_FRAME), (c.name, c.cls, rc, code)
            if rc == 0:
                assert out.tobytes() == data, c.name


# ---- the compiled kernels --------------------------------------------------------------------------------------------------------
_SEEN = {}


def _replay(model, c, pos, cur, w, cap):
    """one feed of the model's caller through the compiled kernels -> their answer (remembered by what the kernels see: many
    cases share the feeds in front of their damage)"""
    window = c.img[pos:pos + w]
    if c.codec == LZ4:
        key = (LZ4, window, c.index[-1] - pos, cap)
        if key not in _SEEN:
            _SEEN[key] = sk.feed_lz4(window, c.index[-1] - pos, cap)
    else:
        n, off, mid, pend = model.pieces(c.index, cur, pos, w)
        key = (c.codec, window, tuple(off), mid, pend, cap)
        if key not in _SEEN:
            _SEEN[key] = sk.feed_chunks(c.codec, window, off, mid, pend, cap)
    return _SEEN[key]


WORDS = ("stop", "need", "n_frames", "k", "consumed", "out_len", "need_dst")


PARAMS = [(codec, cls) for codec in (LZ4, SNAPPY, LZF) for cls in sd.CLASSES if not (codec == LZF and cls == sd.OVERSIZED)]


@pytest.mark.parametrize("codec,cls", PARAMS, ids=["%s-%s" % (sd.CODEC_NAME[a], b) for a, b in PARAMS])
def test_discovery_and_cut(oracle, model, codec, cls):
    """status, stop, need, n_frames, k, consumed, out_len and need_dst of every feed a contract-following caller makes.
    An `oversized-claim` Snappy chunk above kBatchMaxBlock is refused by discovery (status S3S_E_UNSUPPORTED): a feed never
    answers need_dst above kBatchMaxBlock.  (Without that rule in walk_piece_stream the compiled kernels answer status 0 and
    need_dst = 2147483647 / 2147483648 / 4294967295 for the three largest claims, and both assertions below fail.)"""
    feeds = 0
    for c, scheds, _ in covered(oracle):
        if c.codec != codec or c.cls != cls:
            continue
        for s in scheds:
            trace, _ = model.run(c, s, 0)
            assert len(trace) <= 5 * (len(sd.su.units(codec, c.image.img, c.image.index)) + 1), (c.name, s, len(trace))
            last = trace[-1][4]
            if cls == sd.VALID_DIFFERENT:
                assert last["code"] == 0 and last["at_end"] == 1, (c.name, s, last["code"])
            else:
                assert last["code"] == (sd.E_UNSUPPORTED if c.claim > sd.K_MAX else sd.E_BAD_FRAME), (c.name, s, last["code"])
            for pos, cur, w, cap, r in trace:
                want = r["kernel"]
                if want is None:
                    continue
                got = _replay(model, c, pos, cur, w, cap)
                feeds += 1
                assert got["need_dst"] <= sd.K_MAX, ("need_dst beyond the largest block a decoder takes", c.name, s, pos, w, cap, got)
                assert got["status"] == want["status"], ("parity with the model", c.name, s, pos, w, cap, got, want)
                if want["status"] == 0:
                    assert all(got[k] == want[k] for k in WORDS), (c.name, s, pos, w, cap, got, {k: want[k] for k in WORDS})
                    heads = [(u[0] - pos + u[3], u[1] - u[3], u[2]) for u in want["units"]]
                    assert [(f[0], f[1], f[2] & 0xFFFFFFFF) for f in got["frames"]] == heads, (c.name, s, pos)
    assert feeds > 0


def test_corruption_beats_a_refused_claim_whatever_the_order(oracle, model):
    """two damaged partitions in one window: a Snappy chunk that claims 2^32 - 1 bytes in one, a chunk length of 0 in the other.
    One lane per piece raises the status word; the answer is S3S_E_BAD_FRAME in both orders, never a matter of which lane came
    last (S3S_E_UNSUPPORTED does not fail the stream, so the two answers would differ in what the next feed says)."""
    image = next(i for i in sd.images(oracle) if i.name == "snappy")
    units = sd.su.units(SNAPPY, image.img, image.index)
    first = [next(u for u in units if u[0] >= image.index[p] and u[2] > 0) for p in (0, 1)]
    for big, bad in ((0, 1), (1, 0)):
        img = sd._set(image.img, first[big][0] + 4, sd._varint((1 << 32) - 1))
        img = sd._set(img, first[bad][0], bytes(4))
        c = sd.Case("two-partitions", image, img, image.index, first[big], (first[big][0] + 4, first[big][0] + 9))
        n, off, mid, pend = model.pieces(c.index, 0, 0, len(img))
        assert n == 2
        got = sk.feed_chunks(SNAPPY, img, off, mid, pend, 1 << 18)
        want = model.discover(SNAPPY, img, c.index, 0, 0, len(img), 1 << 18)
        assert got["status"] == want["status"] == sd.E_BAD_FRAME, (big, bad, got["status"], want["status"])
        alone = sd._set(image.img, first[big][0] + 4, sd._varint((1 << 32) - 1))
        assert sk.feed_chunks(SNAPPY, alone, off, mid, pend, 1 << 18)["status"] == sd.E_UNSUPPORTED


@CODECS
def test_payload_invalid_units_through_the_decoders(oracle, model, codec):
    """the feed that holds the damaged unit alone (the unit-at-a-time caller's): the cut table's k frames through the compiled
    decoder with a destination of exactly out_len bytes.  It answers a status, and a write outside [0, out_len) would be a
    fault of the interpreter's memory."""
    fmt = {LZ4: 0, SNAPPY: 1, LZF: 2}[codec]
    ran = 0
    for c in (x for x in sd.cases(oracle) if x.codec == codec and x.cls == sd.PAYLOAD_INVALID):
        trace, _ = model.run(c, sd.Schedule("unit-at-a-time", c.index[-1], "ample", True), 0)
        pos, cur, w, cap, r = trace[-1]
        assert r["code"] == sd.E_BAD_FRAME and r["kernel"]["status"] == 0 and r["kernel"]["k"] >= 1, (c.name, r)
        got = _replay(model, c, pos, cur, w, cap)
        assert got["status"] == 0 and all(got[k] == r["kernel"][k] for k in WORDS), (c.name, got)
        k = got["k"]
        outs = [0]
        for f in got["frames"][:k]:
            outs.append(outs[-1] + f[2])
        assert outs[-1] == got["out_len"]
        st, _ = dk.decode_range(c.img[pos:pos + w], got["frames"][:k], outs, fmt=fmt)
        assert st == sd.E_BAD_FRAME, (c.name, st)
        ran += 1
    assert ran == TOTALS[sd.CODEC_NAME[codec]][sd.PAYLOAD_INVALID]
