"""GPU: resumable Zstandard streams (s3s_dstream_open_zstd).  The frames are libzstd's streaming writer's, the spec-level
writer's and the library's own; the truth is the source bytes and the one-shot call; positions, need_comp and verdicts are the
contract model's (tests/stream_units_zstd.py).  Every damaged or refused input here goes through the host model under the
sanitizers in tests/test_zstd_stream_inputs_cpu.py first: the GPU runs only what was classified there."""
import zlib

import numpy as np
import pytest

import stream_units_zstd as U
import zstd_stream_lib as L
from hipdev import Dev

pytestmark = pytest.mark.gpu

ZSTD, LZ4 = 3, 1
ADLER, CRC = 1, 2
E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_UNSUPPORTED = -1, -2, -3, -4, -6
OPT_ZSTD_COMPRESS, OPT_VARIANT, OPT_STAGED = 9, 13, 15
GUARD = 256


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


def _opts(gpu_codec, variant, staged):
    gpu_codec.set_option(OPT_VARIANT, variant)
    gpu_codec.set_option(OPT_STAGED, staged)


@pytest.fixture()
def default_opts(gpu_codec):
    yield
    _opts(gpu_codec, 1, 0)


def feed_all(gpu_codec, dev, img, index, sums, algo, wlog, ends, cap, model=None, host=False, d_img=None):
    """The range through one stream; window k ends at the first of `ends` behind the position (then at need_comp when a feed asks).
    Every feed is compared with the contract model when one is given.  -> (decoded bytes, feeds)"""
    import s3shuffle

    total = int(index[-1])
    d_img = dev.upload(img) if d_img is None and not host else d_img
    d_dst = dev.alloc(cap + 2 * GUARD)
    h_dst = np.empty(cap, np.uint8)
    out, feeds = [], 0
    ends = sorted(set(int(e) for e in ends if 0 < e <= total) | {total})
    with s3shuffle.DecodeStream(gpu_codec, ZSTD, algo, index, sums if algo else None, window_log_max=wlog) as s:
        at_end = total == 0 and len(index) == 1
        need = 0
        while not at_end:
            pos = s.position
            end = pos + need if need else next((e for e in ends if e > pos), total)
            end = min(end, total)
            w = end - pos
            if host:
                r = s.feed(img[pos:end], h_dst, cap)
            else:
                dev.fill(d_dst, 0xA5, cap + 2 * GUARD)
                r = s.feed_device(d_img + pos, w, d_dst + GUARD, cap)
            feeds += 1
            assert feeds < 20000, "the stream makes no progress"
            assert r.code == 0, (r.code, pos, w, r.need_dst)
            assert s.position == pos + r.consumed and 0 <= r.consumed <= w and 0 <= r.out_len <= cap
            if model is not None:
                code, consumed, out_len, need_comp, _ = model.feed(w, cap)
                assert (code, consumed, need_comp) == (0, r.consumed, r.need_comp), (pos, w, (consumed, need_comp), (r.consumed, r.need_comp))
                assert out_len is None or out_len == r.out_len, (pos, w, out_len, r.out_len)
            if host:
                out.append(h_dst[:r.out_len].copy())
            else:
                got = dev.download(d_dst, cap + 2 * GUARD)
                assert (got[:GUARD] == 0xA5).all() and (got[GUARD + r.out_len:] == 0xA5).all(), "a byte outside dst[0, out_len) was written"
                out.append(got[GUARD:GUARD + r.out_len].copy())
            at_end = bool(r.at_end)
            if r.consumed == 0 and not at_end:
                assert r.need_comp > w, ("asked for no more than it had", pos, w, r.need_comp)
                assert r.need_comp <= 3 + U.MAX_BLOCK
                need = r.need_comp
            else:
                assert r.need_comp == 0
                need = 0
        assert s.position == total
        assert s.close() == 0
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), feeds


def _sum(algo, b):
    b = bytes(b)
    return (zlib.adler32(b) if algo == ADLER else zlib.crc32(b)) & 0xFFFFFFFF


_IMG = {}


def _image(window_log):
    """7 partitions: an empty one, one of 1 byte, one of two frames (two spills), one of >= 5 blocks, the rest ordinary."""
    if window_log not in _IMG:
        srcs = [np.zeros(0, np.uint8), L.source(6, 1), L.source(6, 100_000), L.source(3, 110_000), L.source(6, 30_001), L.source(4, 50_000),
                L.source(2, 45_003)]
        parts = []
        for p, s in enumerate(srcs):
            if p == 0:
                parts.append(np.zeros(0, np.uint8))
            elif p == 2:  # two spills: two frames
                parts.append(np.concatenate([L.compress(s[:60_000], 1, window_log), L.compress(s[60_000:], 3, window_log)]))
            elif p == 3:  # a flush every 20 000 bytes: at least 5 blocks whatever the window
                parts.append(L.compress(s, 1, window_log, flush=20_000))
                assert len([u for u in U.partition_units(parts[-1].tobytes()) if (u[1] & 15) >= U.RAW]) >= 5
            else:
                parts.append(L.compress(s, 1, window_log))
        index = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
        img = np.concatenate(parts)
        sizes = {}
        for p, part in enumerate(parts):
            if part.size:
                sizes.update({int(index[p]) + o: d for o, d in U.decoded_sizes(part.tobytes()).items()})
        _IMG[window_log] = (np.concatenate(srcs), img, index, parts, sizes)
    return _IMG[window_log]


def _wlog(window_log):
    return window_log or 21  # (level 3 at its default: the second spill of partition 2)


# ---- equivalence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, ADLER, CRC], ids=["nosum", "adler32", "crc32"])
@pytest.mark.parametrize("window_log", [10, 17, 0], ids=["wlog10", "wlog17", "default"])
def test_equivalence(gpu_codec, dev, default_opts, window_log, algo):
    data, img, index, parts, sizes = _image(window_log)
    total, wlog = int(index[-1]), _wlog(window_log)
    sums = np.array([_sum(algo, p) for p in parts], np.int64) if algo else None
    d_img = dev.upload(img)
    for variant, staged in ((1, 0), (0, 0), (1, 1), (0, 1)):  # keys 13 and 15 both ways: the one-shot call ...
        _opts(gpu_codec, variant, staged)
        one = gpu_codec.decompress_range(ZSTD, algo, img, index, sums, dst_capacity=data.size)
        assert np.array_equal(one, data), (variant, staged)
        # ... and a stream under the same setting
        out, _ = feed_all(gpu_codec, dev, img, index, sums, algo, wlog, range(65536, total, 65536), 1 << 20,
                          U.StreamModel(img, index, wlog, sizes), d_img=d_img)
        assert np.array_equal(out, data), (variant, staged)
    _opts(gpu_codec, 1, 0)
    bounds = U.boundaries(img, index, wlog)
    schedules = {"one feed": [total], "4 KiB": range(4096, total, 4096),
                 "unit by unit": [b + d for b in bounds for d in (-1, 0, 1)]}
    for name, ends in schedules.items():
        out, feeds = feed_all(gpu_codec, dev, img, index, sums, algo, wlog, ends, 1 << 20, U.StreamModel(img, index, wlog, sizes), d_img=d_img)
        assert np.array_equal(out, data), name
    if algo == CRC:  # host buffers
        out, _ = feed_all(gpu_codec, dev, img, index, sums, algo, wlog, range(65536, total, 65536), 1 << 20,
                          U.StreamModel(img, index, wlog, sizes), host=True)
        assert np.array_equal(out, data)


# ---- history only from the stream -----------------------------------------------------------------------------------------------
def test_history_comes_from_the_stream_alone(gpu_codec, dev, oracle):
    """200 KiB of noise twice in one window_log 18 frame: every match of the second half reaches 200 KiB back.  One block per
    feed, every feed into a fresh poisoned buffer with guard bands (feed_all), a one-shot decode of another image on the same
    context between two feeds."""
    import s3shuffle

    half = np.random.default_rng(5).integers(0, 256, 200 << 10, dtype=np.uint8)
    src = np.concatenate([half, half])
    frame = L.compress(src, level=3, window_log=18)
    assert frame.size < src.size * 0.6
    index = np.array([0, frame.size], np.int64)
    other_src = L.source(6, 300_000)
    other, oidx, _ = oracle.compress_map_output(LZ4, 0, other_src, np.array([0, other_src.size], np.int64))
    bounds = U.boundaries(frame, index, 18)
    d_img = dev.upload(frame)
    out = []
    with s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, None, window_log_max=18) as s:
        for b in bounds[1:]:
            pos = s.position
            d_dst = dev.alloc((128 << 10) + 2 * GUARD)  # a fresh buffer per feed: nothing of an earlier feed's output is near
            dev.fill(d_dst, 0x5A, (128 << 10) + 2 * GUARD)
            r = s.feed_device(d_img + pos, b - pos, d_dst + GUARD, 128 << 10)
            assert r.code == 0 and r.consumed == b - pos
            got = dev.download(d_dst, (128 << 10) + 2 * GUARD)
            assert (got[:GUARD] == 0x5A).all() and (got[GUARD + r.out_len:] == 0x5A).all()
            out.append(got[GUARD:GUARD + r.out_len].copy())
            dev.fill(d_dst, 0x5A, (128 << 10) + 2 * GUARD)  # what the feed wrote is gone before the next one
            dev.release(d_dst)
            assert np.array_equal(gpu_codec.decompress_range(LZ4, 0, other, oidx, None, dst_capacity=other_src.size), other_src)
        assert r.at_end
    assert np.array_equal(np.concatenate(out), src)


# ---- capacity ---------------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_at_block_boundaries(gpu_codec, dev):
    import s3shuffle

    src = L.source(6, 64 << 10)
    frame = L.compress(src, 1, 10)
    index = np.array([0, frame.size], np.int64)
    sizes = U.decoded_sizes(frame.tobytes())
    units = U.partition_units(frame.tobytes())
    blocks = [(o, sizes[o]) for o, k, _, _ in units if (k & 15) >= U.RAW]
    hdr = units[0][3]
    d_img = dev.upload(frame)
    d_dst = dev.alloc(1 << 17)
    for k in (1, 2, 7):
        exact = sum(d for _, d in blocks[:k])
        for cap, want in ((exact, k), (exact - 1, k - 1)):
            with s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, None, window_log_max=10) as s:
                r = s.feed_device(d_img, hdr, d_dst, cap)  # the frame header: a unit of no output
                assert (r.code, r.consumed, r.out_len) == (0, hdr, 0)
                r = s.feed_device(d_img + hdr, frame.size - hdr, d_dst, cap)
                if want == 0:  # below the first block
                    assert (r.code, r.consumed, r.out_len, r.need_dst) == (E_CAPACITY, 0, 0, blocks[0][1])
                    assert s.position == hdr
                    r = s.feed_device(d_img + hdr, frame.size - hdr, d_dst, blocks[0][1])  # enough room: it goes on
                    want = 1
                assert r.code == 0 and r.consumed == blocks[want][0] - hdr and r.out_len == sum(d for _, d in blocks[:want]), (k, cap)
                assert np.array_equal(dev.download(d_dst, r.out_len), src[:r.out_len])
                assert r.need_dst == 0 and r.need_dst <= 128 << 10
                s.close(check=False)


# ---- bounded memory -------------------------------------------------------------------------------------------------------------
def test_bounded_memory_one_8_mib_frame(gpu_codec, dev):
    """One 8 MiB frame at the default window through 256 KiB windows and a 256 KiB dst.  After every feed the device bytes the
    stream holds (s3s_dstream_held_bytes: the size it allocated) are at most Window_Size plus the state record - sized by the
    frame (window log 19), not by window_log_max (27 here) nor by the frame's length - 0 once the frame has ended, and a close
    in the middle of the range gives them back."""
    import s3shuffle

    src = np.concatenate([L.source(6, 1 << 20), L.source(3, 1 << 20)] * 4)
    frame = L.compress(src, 1)
    assert src.size == 8 << 20 and L.frame_window_log(frame) == 19
    index = np.array([0, frame.size], np.int64)
    record = 9984  # sizeof(ZStreamState) = 9 864 rounded to 256
    bound = (1 << 19) + record
    lib = gpu_codec._lib
    base = lib.s3s_dstream_held_bytes(None)
    d_img, d_dst = dev.upload(frame), dev.alloc(256 << 10)
    for stop_at in (None, frame.size // 2):  # to the end; closed in the middle of the range
        out, held = [], []
        s = s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, None, window_log_max=27)
        assert s.held_device_bytes == 0
        need = 0
        while True:
            pos = s.position
            w = min(max(256 << 10, need), frame.size - pos)
            r = s.feed_device(d_img + pos, w, d_dst, 256 << 10)
            assert r.code == 0
            out.append(dev.download(d_dst, r.out_len).copy())
            need = r.need_comp if r.consumed == 0 else 0
            held.append(s.held_device_bytes)
            assert held[-1] <= bound and lib.s3s_dstream_held_bytes(None) - base == held[-1], (pos, held[-1])
            if r.at_end:
                assert held[-1] == 0  # the frame has ended
                break
            assert held[-1] == bound  # a frame is open: its record and its window, whatever it has produced beyond
            if stop_at is not None and s.position >= stop_at:
                break
        got = np.concatenate(out)
        assert np.array_equal(got, src[:got.size]) and (stop_at is not None or got.size == src.size)
        assert len(held) >= (4 if stop_at else 32)
        rc = s.close(check=False)
        assert rc == (0 if stop_at is None else E_BAD_FRAME)
        assert lib.s3s_dstream_held_bytes(None) == base  # close released it, also in the middle of the range


# ---- the library's own frames and the conformance corpus ---------------------------------------------------------------------
def test_library_writer_frames_block_by_block(gpu_codec, dev):
    data = np.concatenate([L.source(6, 300_000), L.source(3, 150_000), L.source(0, 5000)])
    offs = np.array([0, 300_000, 450_000, 455_000], np.int64)
    gpu_codec.set_option(OPT_ZSTD_COMPRESS, 1)
    try:
        img, index, sums = gpu_codec.compress_map_output(ZSTD, ADLER, data, offs)
    finally:
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)
    img = np.asarray(img, np.uint8)
    out, feeds = feed_all(gpu_codec, dev, img, index, sums, ADLER, 27, U.boundaries(img, index), 1 << 17, U.StreamModel(img, index, 27))
    assert np.array_equal(out, data) and feeds >= 8


def test_conformance_corpus_block_by_block(gpu_codec, dev):
    """The inputs of tests/test_gpu_zstd_conformance.py, one partition per stream, a feed per unit.  The contract model names
    the frames outside the feature (content checksum, dictionary id field): those are refused, nothing is skipped."""
    import s3shuffle

    cases, expect = L.conformance_cases()
    n_ok = 0
    for c, want in zip(cases, expect):
        part = np.frombuffer(c.data, np.uint8)
        index = np.array([0, part.size], np.int64)
        if want == 0:
            out, _ = feed_all(gpu_codec, dev, part, index, None, 0, 27, U.boundaries(part, index), 1 << 17, U.StreamModel(part, index, 27))
            assert out.tobytes() == c.content, c.name
            n_ok += 1
            continue
        d_img = dev.upload(part)
        d_dst = dev.alloc(1 << 17)
        code = 0
        with s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, None, window_log_max=27) as s:
            for _ in range(4 * len(c.data) + 8):
                pos = s.position
                try:
                    r = s.feed_device(d_img + pos, part.size - pos, d_dst, 1 << 17)
                except s3shuffle.CodecError as e:
                    code = e.code
                    break
                assert r.consumed > 0 and not r.at_end, c.name
            s.close(check=False)
        assert code == want, (c.name, code, want)
        dev.release(d_img)
        dev.release(d_dst)
    assert n_ok >= 200


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_are_not_sticky_and_consume_nothing(gpu_codec, dev):
    import s3shuffle

    crafted = L.crafted()
    good, good_content = crafted["fcs"][0], crafted["fcs"][1]
    for name in ("checksum", "dictionary_id", "window_above", "skippable_big"):
        bad = crafted[name][0]
        img = np.frombuffer(good + bad, np.uint8)
        index = np.array([0, len(good), len(good) + len(bad)], np.int64)
        d_img = dev.upload(img)
        d_dst = dev.alloc(4096 + 2 * GUARD)
        dev.fill(d_dst, 0xA5, 4096 + 2 * GUARD)
        s = s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, None, window_log_max=10)
        for _ in range(2):  # the same feed gets the same answer
            with pytest.raises(s3shuffle.CodecError) as e:
                s.feed_device(d_img, img.size, d_dst + GUARD, 4096)
            assert e.value.code == E_UNSUPPORTED, name
            r = s.last_result
            assert (r.consumed, r.out_len, r.need_dst) == (0, 0, 0) and s.position == 0
        assert (dev.download(d_dst, 4096 + 2 * GUARD) == 0xA5).all()
        r = s.feed_device(d_img, len(good), d_dst + GUARD, 4096)  # a window that does not show the header goes on
        assert r.code == 0 and r.consumed == len(good) and dev.download(d_dst + GUARD, r.out_len).tobytes() == good_content
        assert s.close(check=False) == E_BAD_FRAME  # the range was not read to its end
        # the one-shot call works after it
        assert gpu_codec.decompress_range(ZSTD, 0, np.frombuffer(good, np.uint8), np.array([0, len(good)], np.int64), None,
                                          dst_capacity=4096).tobytes() == good_content


def test_the_other_opens_still_refuse_zstandard(gpu_codec):
    import s3shuffle

    index = np.array([0, 100], np.int64)
    with pytest.raises(s3shuffle.CodecError) as e:
        s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index)
    assert e.value.code == E_UNSUPPORTED
    for wlog in (9, 28, 0, -1):
        with pytest.raises(s3shuffle.CodecError) as e:
            s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, window_log_max=wlog)
        assert e.value.code == E_INVALID, wlog
    for wlog in (10, 27):
        s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, window_log_max=wlog).close(check=False)
    good, content = L.crafted()["fcs"][:2]
    gpu_codec.set_io_encryption(bytes(range(16)))
    try:
        with pytest.raises(s3shuffle.CodecError) as e:
            s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, window_log_max=19)
        assert e.value.code == E_UNSUPPORTED
        with pytest.raises(s3shuffle.CodecError) as e:
            s3shuffle.DecodeStream(gpu_codec, ZSTD, 0, index, encrypted=True)
        assert e.value.code == E_UNSUPPORTED
    finally:
        gpu_codec.set_io_encryption(None)
    assert gpu_codec.decompress_range(ZSTD, 0, np.frombuffer(good, np.uint8), np.array([0, len(good)], np.int64), None,
                                      dst_capacity=4096).tobytes() == content


# ---- damage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", L.DAMAGE_NAMES)
def test_damage(gpu_codec, dev, name):
    """Field-targeted mutations (tests/zstd_stream_lib.py: damage_cases, classified on the CPU): the feed ends, the class of the
    code is right, it sticks or not as the contract says, nothing is reported consumed, the guard bands hold, close answers."""
    import s3shuffle

    img, index, sums, algo, want, prefix = L.damage_cases()[name]
    total = int(index[-1])
    d_img = dev.upload(img)
    cap = 1 << 17
    d_dst = dev.alloc(cap + 2 * GUARD)
    one_feed_want = want
    for sched in ("one feed", "unit by unit"):
        want = L.DAMAGE_WANT_UNIT_BY_UNIT.get(name, one_feed_want) if sched == "unit by unit" else one_feed_want
        s = s3shuffle.DecodeStream(gpu_codec, ZSTD, algo, index, sums if algo else None, window_log_max=10)
        out, code, need = [], 0, 0
        for _ in range(4000):
            pos = s.position
            if pos == total:
                break
            w = total - pos if sched == "one feed" else min(total - pos, need or 1)
            dev.fill(d_dst, 0xA5, cap + 2 * GUARD)
            try:
                r = s.feed_device(d_img + pos, w, d_dst + GUARD, cap)
            except s3shuffle.CodecError as e:
                code = e.code
                r = s.last_result
                assert (r.consumed, r.out_len) == (0, 0) and s.position == pos
                assert (dev.download(d_dst, GUARD) == 0xA5).all() and (dev.download(d_dst + GUARD + cap, GUARD) == 0xA5).all()
                if code == E_CHECKSUM:
                    assert e.partition == r.bad_partition == L.DAMAGE_BAD_PARTITION.get(name, 1)
                break
            got = dev.download(d_dst, cap + 2 * GUARD)
            assert (got[:GUARD] == 0xA5).all() and (got[GUARD + r.out_len:] == 0xA5).all()
            out.append(got[GUARD:GUARD + r.out_len].copy())
            if r.at_end:
                break
            need = r.need_comp if r.consumed == 0 else 0
            assert r.consumed > 0 or r.need_comp > w
        assert code == want, (name, sched, code, want)
        got = np.concatenate(out) if out else np.zeros(0, np.uint8)
        assert got.size <= prefix.size and np.array_equal(got, prefix[:got.size]), (name, sched)  # what was handed out before is the source's
        # stickiness: BAD_FRAME and CHECKSUM stay, UNSUPPORTED repeats because nothing changed
        with pytest.raises(s3shuffle.CodecError) as e:
            s.feed_device(d_img + s.position, min(w, total - s.position), d_dst + GUARD, cap)
        assert e.value.code == want
        assert s.close(check=False) == (E_BAD_FRAME if want == E_UNSUPPORTED else want)
    # the context is intact: the one-shot call on a good image
    good, content = L.crafted()["fcs"][:2]
    assert gpu_codec.decompress_range(ZSTD, 0, np.frombuffer(good, np.uint8), np.array([0, len(good)], np.int64), None,
                                      dst_capacity=4096).tobytes() == content
