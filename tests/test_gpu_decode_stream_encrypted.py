"""GPU: the streaming reduce side under Spark IO encryption (s3s_dstream_open_encrypted).  Plain images come from the oracle's
writers, the stored ones from the reference layer over them (tests/spark_crypto_ref.py through tests/stream_units_encrypted.py);
the truth is the source bytes, the one-shot encrypted call and su.expected_feed over the stored unit list (the plain units
shifted by the IVs in front of them, plus every non-empty partition's IV as a 16-byte unit of no output)."""
import ctypes

import numpy as np
import pytest

import corpus
import stream_units as su
import stream_units_encrypted as sue
from hipdev import Dev

pytestmark = pytest.mark.gpu

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
ADLER, CRC, CRC32C = 1, 2, 3
E_INVALID, E_CAPACITY, E_BAD_FRAME, E_CHECKSUM, E_UNSUPPORTED = -1, -2, -3, -4, -6
BLOCK = {LZ4: 32768, SNAPPY: 32768, LZF: 65535}  # decoded bytes of the largest unit the oracle's writers produce
CANARY, BAND = 0xA5, 4096


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def keyed(gpu_codec):
    """-> set(key): switches the layer on; it is off again when the test ends, whichever way"""
    yield gpu_codec.set_io_encryption
    gpu_codec.set_io_encryption(None)


def _code(exc_info):
    return exc_info.value.code


def _concat(parts):
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.uint8), offs


class Banded:
    """dst between two canary bands: [BAND canary][dst, cap][BAND canary]"""

    def __init__(self, dev, cap):
        self.dev, self.cap = dev, cap
        self.base = dev.alloc(cap + 2 * BAND)
        dev.fill(self.base, CANARY, cap + 2 * BAND)
        self.dst = self.base + BAND

    def check(self, cap=None):
        cap = self.cap if cap is None else cap
        assert np.all(self.dev.download(self.base, BAND) == CANARY), "write in front of dst"
        assert np.all(self.dev.download(self.dst + cap, self.cap - cap + BAND) == CANARY), "write behind dst_capacity"


def _expected(codec, ulist, eidx, pos, w, cap):
    return sue.expected_feed_none(eidx, pos, w, cap) if codec == NONE else su.expected_feed(ulist, pos, w, cap)


def run_stream(codec_ctx, dev, codec, algo, eidx, sums, d_img, ulist, window, cap, band, first=None, follow_rest=False, max_feeds=100_000):
    """Feeds the stored range with windows of `window` bytes (the first one `first`; grown to need_comp when told; follow_rest:
    the rest of the range after a feed that consumed) into band.dst[:cap] -> (decoded bytes, results).  Every feed must take
    exactly what expected_feed says."""
    import s3shuffle

    total = int(eidx[-1])
    out, results, win = [], [], (window if first is None else first)
    with s3shuffle.DecodeStream(codec_ctx, codec, algo, eidx, sums if algo else None, encrypted=True) as s:
        while True:
            pos = s.position
            w = min(win, total - pos)
            r = s.feed_device(d_img + pos, w, band.dst, cap)
            assert len(results) < max_feeds, "the stream makes no progress"
            assert r.code == 0, (r.code, r.need_dst, pos, w)
            want = _expected(codec, ulist, eidx, pos, w, cap)
            assert (r.consumed, r.out_len) == want, (pos, w, cap, (r.consumed, r.out_len), want)
            assert s.position == pos + r.consumed
            results.append((pos, w, r.consumed, r.out_len, r.need_comp, r.at_end))
            if r.out_len:
                out.append(dev.download(band.dst, r.out_len).copy())
            if r.at_end:
                assert s.position == total
                break
            if r.consumed == 0:
                assert total - pos >= r.need_comp > w, ("need_comp", pos, w, r.need_comp)
                win = r.need_comp
            else:
                assert r.need_comp == 0
                win = total if follow_rest else window
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), results


# ---- 1. equivalence ------------------------------------------------------------------------------------------------------
_EQ = {}


def _equivalence_image(oracle, codec, algo, key_bytes):
    """twelve partitions: two empty ones, one stored as its IV alone (16 bytes: an empty stream), a 1-byte and a 17-byte one.
    The larger partitions are trimmed by up to 15 source bytes each so that the stored partition starts cover at least 8
    residues mod 16 (the stored size of a partition is its own stream's, whatever surrounds it); enough incompressible bytes
    for the stored image to cross 40 KiB + 5."""
    if "src" not in _EQ:
        rng = np.random.default_rng(1813)
        sizes = [0, 30_001, 1, 0, 25_003, 12_345, 0, 9_999, 17, 20_011, 3_001, 4_444]
        kinds = [7, 0, 3, 0, 7, 0, 5, 3, 0, 4, 7, 0]
        _EQ["src"] = [corpus.chunk_corpus(kinds[p], n, rng) for p, n in enumerate(sizes)]
    if codec not in _EQ:
        parts, seen, at = [], set(), 0
        for p, full in enumerate(_EQ["src"]):
            pick = None
            for k in range(16 if full.size >= 3000 else 1):
                body = full[:full.size - k]
                stored = int(oracle.compress_map_output(codec, 0, body, np.array([0, body.size], np.int64))[1][-1]) + (16 if body.size or p == 3 else 0)
                if pick is None or ((at + stored) % 16 not in seen and (at + pick[1]) % 16 in seen):
                    pick = (body, stored)
            parts.append(pick[0])
            if pick[1]:
                seen.add(at % 16)
            at += pick[1]
        data, offs = _concat(parts)
        img, index, _ = oracle.compress_map_output(codec, 0, data, offs)
        _EQ[codec] = (data, img, index)
    data, img, index = _EQ[codec]
    if (codec, algo, key_bytes) not in _EQ:
        ivs = sue.ivs_for(len(index) - 1, 40 + key_bytes)
        enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[key_bytes], ivs, iv_only={3}, algo=algo)
        starts = {int(eidx[p]) % 16 for p in range(len(eidx) - 1) if eidx[p + 1] > eidx[p]}
        assert len(starts) >= 8 and int(eidx[-1]) > 40 * 1024 + 5 and int(eidx[4] - eidx[3]) == 16, (sorted(starts), int(eidx[-1]))
        assert sum(1 for p in range(len(eidx) - 1) if eidx[p + 1] == eidx[p]) == 2
        ulist = sue.stored_units(codec, img.tobytes(), eidx) if codec != NONE else None
        _EQ[(codec, algo, key_bytes)] = (enc, eidx, sums, ulist)
    return (data,) + _EQ[(codec, algo, key_bytes)]


EQ_PARAMS = [(NONE, CRC, 16), (NONE, 0, 24), (NONE, ADLER, 32), (LZ4, ADLER, 16), (LZ4, CRC, 24), (LZ4, CRC32C, 32), (LZ4, 0, 16),
             (SNAPPY, CRC, 16), (SNAPPY, 0, 24), (SNAPPY, ADLER, 32), (LZF, CRC32C, 16), (LZF, 0, 24), (LZF, CRC, 32)]


@pytest.mark.parametrize("codec,algo,key_bytes", EQ_PARAMS, ids=["%s-%s-aes%d" % ({0: "none", 1: "lz4", 2: "snappy", 4: "lzf"}[c], ("nosum", "adler32", "crc32", "crc32c")[a], 8 * k)
                                                                 for c, a, k in EQ_PARAMS])
def test_equivalence(gpu_codec, oracle, dev, keyed, codec, algo, key_bytes):
    data, enc, eidx, sums, ulist = _equivalence_image(oracle, codec, algo, key_bytes)
    keyed(sue.KEYS[key_bytes])
    total = int(eidx[-1])
    d_img = dev.upload(enc)
    d_one = dev.alloc(data.size)
    assert gpu_codec.decompress_range_device(codec, algo, d_img, total, eidx, sums, d_one, data.size) == data.size
    assert np.array_equal(dev.download(d_one, data.size), data)  # the one-shot encrypted call on the same bytes
    one_unit = BLOCK[codec] if codec != NONE else 5_000  # (a byte at a time is ~10^5 feeds: test_every_cut_none has the small capacities)
    band = Banded(dev, 65536)
    for window in (4099, 16 * 1024 - 1, 16 * 1024 + 1, 40 * 1024 + 5):
        for cap in (65536, one_unit):
            bound = 4 * len(ulist) + 2 if codec != NONE else total // min(window, cap) + 2 * len(eidx) + 2
            dev.fill(band.dst, CANARY, band.cap)  # (the run before wrote up to ITS capacity)
            out, results = run_stream(gpu_codec, dev, codec, algo, eidx, sums, d_img, ulist, window, cap, band, max_feeds=bound)
            assert np.array_equal(out, data), (window, cap)
            assert sum(r[2] for r in results) == total
            assert [r[5] for r in results].count(1) == 1 and results[-1][5] == 1  # at_end only at the end
            band.check(cap)


# ---- 2. every cut ------------------------------------------------------------------------------------------------------------
def _cut_image(oracle, codec):
    """the every-cut images of tests/test_gpu_decode_stream.py (at most 12 KB), encrypted"""
    if codec == LZ4:
        rng = np.random.default_rng(5)
        data, offs = _concat([corpus.chunk_corpus(3, 3 * 4096 - 100, rng), corpus.chunk_corpus(7, 2 * 4096 + 9, rng)])
        img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs, 4096)
        algo, kb = ADLER, 16
    elif codec == SNAPPY:
        rng = np.random.default_rng(6)
        data, offs = _concat([corpus.chunk_corpus(3, 2 * 4096 + 5, rng), corpus.chunk_corpus(7, 4096 + 900, rng)])
        img, index, _ = oracle.compress_map_output(SNAPPY, 0, data, offs, 4096)
        algo, kb = CRC, 24
    elif codec == LZF:
        data, offs, img, index, _ = su.lzf_cut_image(oracle, CRC32C)
        algo, kb = CRC32C, 32
    else:
        rng = np.random.default_rng(1812)
        data, offs = _concat([rng.integers(0, 256, n, dtype=np.uint8) for n in (0, 81, 1, 0, 98, 45, 0)])
        img, index, _ = oracle.compress_map_output(NONE, 0, data, offs)
        algo, kb = ADLER, 16
    enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[kb], sue.ivs_for(len(index) - 1, 60 + codec), algo=algo)
    assert int(eidx[-1]) <= 12_100 and (codec != NONE or int(eidx[-1]) == 289)
    return data, enc, eidx, sums, sue.stored_units(codec, img.tobytes(), eidx), algo, kb


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF, NONE], ids=["lz4", "snappy", "lzf", "none"])
def test_every_cut(gpu_codec, oracle, dev, keyed, codec):
    """for every cut c the first window is [0, c), then the caller follows need_comp and otherwise presents the rest of the
    range: a window end on every byte of every IV, a window start on every residue of a key stream block"""
    data, enc, eidx, sums, ulist, algo, kb = _cut_image(oracle, codec)
    keyed(sue.KEYS[kb])
    total = int(eidx[-1])
    d_img = dev.upload(enc)
    band = Banded(dev, data.size + 64)
    residues = set()
    for c in range(1, total):
        out, results = run_stream(gpu_codec, dev, codec, algo, eidx, sums, d_img, ulist, total, band.cap, band, first=c, follow_rest=True,
                                  max_feeds=8)
        assert np.array_equal(out, data), c
        for pos, *_ in results[1:]:
            p = max(q for q in range(len(eidx) - 1) if eidx[q] <= pos and eidx[q + 1] > eidx[q])
            if pos > eidx[p]:
                residues.add((pos - int(eidx[p]) - 16) % 16)
    band.check()
    if codec == NONE:  # its units are bytes: the second window starts wherever the first one ended
        assert residues == set(range(16))
    else:  # a window starts on a unit boundary: every one of them was a window start
        want = {(st - 16 - int(eidx[p])) % 16 for st, ln, dec in ulist for p in range(len(eidx) - 1) if eidx[p] + 16 < st < eidx[p + 1]}
        assert residues >= want and want, (sorted(residues), sorted(want))


def test_every_cut_none_small_capacities(gpu_codec, oracle, dev, keyed):
    """S3S_CODEC_NONE with dst_capacity 1 .. 33 from position 0: the key stream restarts at every residue"""
    data, enc, eidx, sums, ulist, algo, kb = _cut_image(oracle, NONE)
    keyed(sue.KEYS[kb])
    total = int(eidx[-1])
    d_img = dev.upload(enc)
    band = Banded(dev, 64)
    for cap in range(1, 34):
        out, results = run_stream(gpu_codec, dev, NONE, algo, eidx, sums, d_img, ulist, total, cap, band, max_feeds=total + 16)
        assert np.array_equal(out, data), cap
        for pos, w, consumed, out_len, _, _ in results:  # the analytic expectation is su.expected_feed's
            assert (consumed, out_len) == su.expected_feed(ulist, pos, w, cap)
        band.check(cap)


def test_none_one_byte_capacity_under_windows_across_a_tile(gpu_codec, oracle, dev, keyed):
    """S3S_CODEC_NONE with dst_capacity 1 - one unit - under windows of 16 KiB + 1, which cross the pass's 16 KiB tile: an image
    trimmed to 17 KB so that a byte per feed stays a few seconds (the equivalence images take 5 000 bytes as their small capacity)"""
    rng = np.random.default_rng(1814)
    data, offs = _concat([rng.integers(0, 256, n, dtype=np.uint8) for n in (9_001, 0, 7_003, 901)])
    img, index, _ = oracle.compress_map_output(NONE, 0, data, offs)
    enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[24], sue.ivs_for(4, 77), algo=CRC)
    keyed(sue.KEYS[24])
    total = int(eidx[-1])
    assert total > 16 * 1024 + 1
    band = Banded(dev, 64)
    out, results = run_stream(gpu_codec, dev, NONE, CRC, eidx, sums, dev.upload(enc), None, 16 * 1024 + 1, 1, band, max_feeds=data.size + 8)
    assert np.array_equal(out, data) and len(results) == data.size  # (an IV goes with the byte behind it)
    band.check(1)


# ---- 3. counter carries across feeds ----------------------------------------------------------------------------------------
def test_counter_carries_across_feeds(gpu_codec, oracle, dev, keyed):
    rng = np.random.default_rng(33)
    data, offs = _concat([rng.integers(0, 256, n, dtype=np.uint8) for n in (700, 0, 613, 650)])
    img, index, _ = oracle.compress_map_output(NONE, 0, data, offs)
    ivs = np.array([[0xFF] * 16, [1] * 16, [0] * 8 + [0xFF] * 7 + [0xF0], [0xFF] * 15 + [0xFE]], np.uint8)
    for kb in (16, 32):
        keyed(sue.KEYS[kb])
        enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[kb], ivs, algo=CRC)
        band = Banded(dev, 128)
        out, results = run_stream(gpu_codec, dev, NONE, CRC, eidx, sums, dev.upload(enc), None, 100, 128, band, max_feeds=40)
        assert np.array_equal(out, data)
        band.check()


# ---- 4. verdicts -------------------------------------------------------------------------------------------------------------
def _raw_feed(s, d_comp, comp_len, d_dst, cap):
    import s3shuffle

    res = s3shuffle.codec.StreamResult()
    rc = s._lib.s3s_dstream_feed_device(s._s, ctypes.c_void_p(d_comp), comp_len, ctypes.c_void_p(d_dst), cap, ctypes.byref(res))
    return int(rc), res


def _verdict_image(oracle, algo):
    rng = np.random.default_rng(12)
    data, offs = _concat([corpus.chunk_corpus(7, 5_000, rng), corpus.chunk_corpus(0, 40_000, rng), np.zeros(0, np.uint8), corpus.chunk_corpus(7, 3_000, rng)])
    img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs)
    enc, eidx, sums = sue.encrypt(img, index, sue.KEYS[16], sue.ivs_for(4, 9), algo=algo)
    return data, img, index, enc, eidx, sums


def test_flipped_cipher_byte_is_a_wrong_checksum_of_its_partition(gpu_codec, oracle, dev, keyed):
    import s3shuffle

    data, img, index, enc, eidx, sums = _verdict_image(oracle, CRC)
    keyed(sue.KEYS[16])
    p0, p1, total = int(eidx[1]), int(eidx[2]), int(eidx[-1])
    bad = enc.copy()
    bad[p1 - 300] ^= 0x40  # in the last frame's literals: the third feed's window
    d_img = dev.upload(bad)
    band = Banded(dev, data.size + 64)
    s = s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, eidx, sums, encrypted=True)
    for end in (p0 + 7, p0 + (p1 - p0) // 2):  # (the first window ends inside partition 1's IV)
        pos = s.position
        r = s.feed_device(d_img + pos, end - pos, band.dst, band.cap)
        assert r.code == 0 and r.consumed > 0 and s.position <= end
    pos = s.position
    dev.fill(band.dst, CANARY, band.cap)
    for _ in range(2):  # the feed that consumes the partition's last byte, and every later one
        rc, res = _raw_feed(s, d_img + pos, total - pos, band.dst, band.cap)
        assert (rc, res.bad_partition, res.consumed, res.out_len, res.at_end) == (E_CHECKSUM, 1, 0, 0, 0)
        assert s.position == pos
    assert np.all(dev.download(band.dst, band.cap) == CANARY)  # the verdict came before the decode
    band.check()
    assert s.close(check=False) == E_CHECKSUM
    with pytest.raises(s3shuffle.CodecError) as e:  # the one-shot call: the same class, the same partition
        gpu_codec.decompress_range_device(LZ4, CRC, d_img, total, eidx, sums, band.dst, band.cap)
    assert _code(e) == E_CHECKSUM and e.value.partition == 1


def test_corrupt_frames_short_partitions_and_a_range_that_ends_in_an_iv(gpu_codec, oracle, dev, keyed):
    import s3shuffle

    data, img, index, enc, eidx, _ = _verdict_image(oracle, 0)
    keyed(sue.KEYS[16])
    band = Banded(dev, data.size + 64)

    def stream_code(b, idx, window):
        d = dev.upload(b)
        s = s3shuffle.DecodeStream(gpu_codec, LZ4, 0, idx, encrypted=True)
        total = int(idx[-1])
        with pytest.raises(s3shuffle.CodecError) as e:
            for _ in range(100):
                pos = s.position
                r = s.feed_device(d + pos, min(window, total - pos), band.dst, band.cap)
                assert r.code == 0 and (r.consumed > 0 or r.need_comp > 0) and not r.at_end
                window = max(window, r.need_comp)
        last = (s.position, min(window, total - s.position))
        r = s.last_result
        assert (r.consumed, r.out_len) == (0, 0)
        with pytest.raises(s3shuffle.CodecError) as e2:  # the error sticks
            s.feed_device(d + s.position, 1, band.dst, band.cap)
        assert _code(e2) == _code(e) == s.close(check=False)
        with pytest.raises(s3shuffle.CodecError) as e3:  # the one-shot call: the same class
            gpu_codec.decompress_range_device(LZ4, 0, d, total, idx, None, band.dst, band.cap)
        assert _code(e3) == _code(e)
        return _code(e), last

    # a flipped byte in the cipher text of an LZ4Block magic (the second frame of partition 1)
    u = sue.stored_units(LZ4, img.tobytes(), eidx)
    victim = [x for x in u if x[0] > eidx[1] and x[2] > 0][1][0]
    broken = enc.copy()
    broken[victim + 2] ^= 0xFF
    assert stream_code(broken, eidx, 16 * 1024 + 1)[0] == E_BAD_FRAME
    # a partition of 7 stored bytes between two good ones
    seven = np.concatenate([enc[:eidx[1]], enc[eidx[1]:eidx[1] + 7], enc[eidx[2]:]])
    sidx = np.array([0, eidx[1], eidx[1] + 7, eidx[1] + 7, eidx[1] + 7 + eidx[4] - eidx[3]], np.int64)
    assert stream_code(seven, sidx, 3000)[0] == E_BAD_FRAME
    # a range that ends inside the last partition's IV: the failing feed's window ends at the end of the range
    cut = int(eidx[3]) + 9
    code, (pos, w) = stream_code(enc[:cut].copy(), np.array([0, eidx[1], eidx[2], eidx[3], cut], np.int64), 16 * 1024 - 1)
    assert code == E_BAD_FRAME and pos + w == cut
    band.check()


# ---- 5. refusals and coexistence -------------------------------------------------------------------------------------------
def test_refusals_and_coexistence(gpu_codec, oracle, dev, keyed):
    import s3shuffle

    data, enc, eidx, sums, ulist = _equivalence_image(oracle, LZ4, CRC, 24)
    total = int(eidx[-1])
    with pytest.raises(s3shuffle.CodecError) as e:  # the layer is off
        s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, eidx, sums, encrypted=True)
    assert _code(e) == E_INVALID
    keyed(sue.KEYS[24])
    with pytest.raises(s3shuffle.CodecError) as e:
        s3shuffle.DecodeStream(gpu_codec, ZSTD, CRC, eidx, sums, encrypted=True)
    assert _code(e) == E_UNSUPPORTED
    with pytest.raises(s3shuffle.CodecError) as e:  # the plain open keeps its answer: old callers fall back on it
        s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, eidx, sums)
    assert _code(e) == E_UNSUPPORTED
    d_img = dev.upload(enc)
    band = Banded(dev, 100_000)
    # a key change between two feeds, to the same key too: feeds answer E_INVALID, close still works
    for again in (sue.KEYS[24], sue.KEYS[16], None):
        keyed(sue.KEYS[24])
        s = s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, eidx, sums, encrypted=True)
        r = s.feed_device(d_img, 20_000, band.dst, band.cap)
        assert r.code == 0 and r.consumed > 0
        keyed(again)
        for _ in range(2):
            with pytest.raises(s3shuffle.CodecError) as e:
                s.feed_device(d_img + s.position, 20_000, band.dst, band.cap)
            assert _code(e) == E_INVALID
        assert s.close(check=False) == E_BAD_FRAME  # (not read to its end)
    # a one-shot encrypted decode of ANOTHER image between two feeds: the stream's output does not change
    keyed(sue.KEYS[24])
    o_data, o_enc, o_eidx, o_sums, _ = _equivalence_image(oracle, SNAPPY, 0, 24)
    out, win = [], 20_001
    with s3shuffle.DecodeStream(gpu_codec, LZ4, CRC, eidx, sums, encrypted=True) as s:
        while True:
            pos = s.position
            r = s.feed_device(d_img + pos, min(win, total - pos), band.dst, band.cap)
            assert r.code == 0 and (r.consumed > 0 or r.need_comp > win)
            win = r.need_comp if r.consumed == 0 else 20_001  # (a 32 KiB frame is longer than the window: the caller grows it)
            out.append(dev.download(band.dst, r.out_len).copy())
            assert np.array_equal(gpu_codec.decompress_range(SNAPPY, 0, o_enc, o_eidx, None, dst_capacity=o_data.size), o_data)
            if r.at_end:
                break
    assert np.array_equal(np.concatenate(out), data)
    band.check()
    # the host-buffer feed
    dst = np.full(70_000 + 2 * BAND, CANARY, np.uint8)
    out, win = [], 16 * 1024 + 1
    with gpu_codec.decode_stream(LZ4, CRC, eidx, sums, encrypted=True) as s:
        while True:
            pos = s.position
            r = s.feed(enc[pos:min(pos + win, total)], dst[BAND:BAND + 70_000])
            assert r.code == 0 and (r.consumed, r.out_len) == su.expected_feed(ulist, pos, min(win, total - pos), 70_000)
            assert r.consumed > 0 or r.need_comp > win
            win = r.need_comp if r.consumed == 0 else 16 * 1024 + 1
            out.append(dst[BAND:BAND + r.out_len].copy())
            if r.at_end:
                break
    assert np.array_equal(np.concatenate(out), data)
    assert np.all(dst[:BAND] == CANARY) and np.all(dst[BAND + 70_000:] == CANARY)
