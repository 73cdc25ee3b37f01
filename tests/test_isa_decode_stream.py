"""CPU: the stream-mode discovery and the capacity cut of the reduce side (s3s_dstream_feed*), COMPILED for gfx950 and run
through the instruction interpreter (tests/isa/stream_kernel.py) on the cut-position images of tests/test_gpu_decode_stream.py.
The window's buffer is exactly as long as the window, so a kernel that reads a byte at or beyond comp_len faults in the
interpreter's memory; what a feed takes is compared with the stop rule restated in tests/stream_units.py."""
import os
import sys

import numpy as np
import pytest

import corpus
import stream_units as su

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa"))
import stream_kernel as sk  # noqa: E402

LZ4, SNAPPY, LZF = 1, 2, 4
BIG = 1 << 40


def _concat(parts):
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return np.concatenate(parts).astype(np.uint8), offs


def _image(oracle, codec):
    """the images of test_every_cut_position_* (tests/test_gpu_decode_stream.py)"""
    if codec == LZ4:
        rng = np.random.default_rng(5)
        data, offs = _concat([corpus.chunk_corpus(3, 3 * 4096 - 100, rng), corpus.chunk_corpus(7, 2 * 4096 + 9, rng)])
        img, index, _ = oracle.compress_map_output(LZ4, 1, data, offs, 4096)
    elif codec == SNAPPY:
        rng = np.random.default_rng(6)
        data, offs = _concat([corpus.chunk_corpus(3, 2 * 4096 + 5, rng), corpus.chunk_corpus(7, 4096 + 900, rng)])
        img, index, _ = oracle.compress_map_output(SNAPPY, 2, data, offs, 4096)
    else:
        data, _, img, index, _ = su.lzf_cut_image(oracle, 3)
    return img.tobytes(), [int(x) for x in index], data


def pieces(index, pos, length):
    """the host's side of a feed (decode_stream.hip): the pieces of partitions inside the window [pos, pos + length),
    window-relative -> (piece offsets, the first piece starts inside a stream, where the last piece's partition ends)"""
    wend, cur = pos + length, 0
    while cur < len(index) - 1 and index[cur + 1] < pos:
        cur += 1
    while cur < len(index) - 1 and index[cur + 1] <= pos and index[cur + 1] > index[cur]:
        cur += 1  # (a partition that ends exactly at pos is behind the position; an empty one AT pos is passed by this feed)
    ps = []
    p = cur
    while p < len(index) - 1 and (index[p] < wend or index[p + 1] <= wend):
        ps.append(p)
        p += 1
    off = [max(index[ps[0]] - pos, 0)] + [min(index[q + 1] - pos, length) for q in ps]
    return off, pos > index[ps[0]], index[ps[-1] + 1] - pos


def _feed(codec, img, index, pos, length, cap):
    window = img[pos:pos + length]
    if codec == LZ4:
        return sk.feed_lz4(window, len(img) - pos, cap)
    off, mid, pend = pieces(index, pos, length)
    return sk.feed_chunks(codec, window, off, mid, pend, cap)


def _cuts(codec, ulist, n):
    """every offset around every unit's start (inside the magic / stream header, inside each length field, one byte short of a
    unit, on its end) and a sparse sweep in between"""
    c = set(range(1, 24)) | {n - 1}
    for start, ln, _ in ulist:
        c |= {start + d for d in (-2, -1, 0, 1, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16, 17, 20, 21, 22)} | {start + ln - 1}
    c |= set(range(29, n, 311))
    return sorted(x for x in c if 0 < x < n)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_first_window_ends_at_a_cut_second_is_the_rest(oracle, codec):
    img, index, data = _image(oracle, codec)
    n = len(img)
    ulist = su.units(codec, img, index)
    for c in _cuts(codec, ulist, n):
        r = _feed(codec, img, index, 0, c, BIG)
        want = su.expected_feed(ulist, 0, c, BIG)
        assert r["status"] == 0 and (r["consumed"], r["out_len"]) == want, (c, r, want)
        assert r["stop"] == want[0] and r["k"] == r["n_frames"]
        if want[0] < c:  # the window ends inside a unit: its length as far as the window shows it
            visible, ln, _ = su.unit_at(codec, img, want[0], c, codec == SNAPPY and want[0] in index[:-1])
            assert not visible and r["need"] == ln, (c, r["need"], ln)
        else:
            assert r["need"] == 0
        # the frames in front of the stop are the range's units that decode to something, in order
        got = [(f[0], f[1], f[2]) for f in r["frames"]]
        head = {LZ4: 21, SNAPPY: 4}.get(codec)
        exp = [u for u in ulist if u[0] + u[1] <= want[0] and not (codec == SNAPPY and u[1] == 16 and u[2] == 0)]
        assert len(got) == len(exp)
        for f, u in zip(got, exp):
            h = head if head is not None else (7 if img[u[0] + 2] == 1 else 5)
            assert f == (u[0] + h, u[1] - h, u[2]), (c, f, u)
        pos = want[0]
        r2 = _feed(codec, img, index, pos, n - pos, BIG)
        assert r2["status"] == 0 and r2["consumed"] == n - pos and r2["need"] == 0 and r["out_len"] + r2["out_len"] == len(data), (c, r2)


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_capacity_cut(oracle, codec):
    """frames_cut_kernel: the largest k with frame_out[k] <= dst_capacity; consumed = where unit k starts"""
    img, index, data = _image(oracle, codec)
    ulist = su.units(codec, img, index)
    decoded = sorted({0, 1, 299, 300, 301, 4095, 4096, 4097, 8192, 12187, 12188, 12189, len(data) - 1, len(data), len(data) + 1, 65534, 65535, 65536})
    for cap in decoded:
        r = _feed(codec, img, index, 0, len(img), cap)
        want = su.expected_feed(ulist, 0, len(img), cap)
        assert r["status"] == 0 and (r["consumed"], r["out_len"]) == want, (cap, r, want)
        nxt = [u for u in ulist if u[0] >= want[0] and u[2] > 0]
        assert r["need_dst"] == (nxt[0][2] if want[0] < len(img) else 0), (cap, r)


def test_truncated_and_corrupt_windows(oracle):
    """the stop rule is not a licence: a unit that crosses the end of the RANGE, and a bad magic in the middle of a window,
    raise the status as in the one-shot kernels"""
    for codec in (LZ4, SNAPPY, LZF):
        img, index, _ = _image(oracle, codec)
        n = len(img)
        ulist = su.units(codec, img, index)
        short = n - 5  # the range itself ends 5 bytes early: window == what is left of it
        idx = index[:-1] + [short]
        r = _feed(codec, img[:short], idx, 0, short, BIG)
        assert r["status"] == -3, (codec, r)
        victim = ulist[len(ulist) // 2][0]
        broken = bytearray(img)
        broken[victim + (2 if codec != SNAPPY else 0)] ^= 0xFF
        r = _feed(codec, bytes(broken), index, 0, n, BIG)
        assert r["status"] == -3, (codec, r)
        r = _feed(codec, bytes(broken), index, 0, victim, BIG)  # a window that ends in front of the damage does not see it
        assert r["status"] == 0 and r["consumed"] == victim


def test_lz4_windows_of_several_tiles(oracle):
    """the tile-speculative chain: the stop in the second and third 64 KiB tile, a frame larger than a tile cut by the window,
    and magic bytes inside a payload in front of the stop"""
    rng = np.random.default_rng(21)
    inner = oracle.compress_stream(LZ4, rng.integers(0, 256, 3000, dtype=np.uint8), 1024)
    data, offs = _concat([corpus.chunk_corpus(0, 200_000, rng), np.resize(inner, 40_000), corpus.chunk_corpus(7, 60_000, rng)])
    img, index, _ = oracle.compress_map_output(LZ4, 0, data, offs)
    img, index = img.tobytes(), [int(x) for x in index]
    ulist = su.units(LZ4, img, index)
    n = len(img)
    assert n > 3 * 65536
    for c in (65535, 65536, 65537, 65536 + 32789 + 10, 131072, 131073, 3 * 65536 + 5, n - 1, n):
        r = sk.feed_lz4(img[:c], n, BIG)
        want = su.expected_feed(ulist, 0, c, BIG)
        assert r["status"] == 0 and (r["consumed"], r["out_len"]) == want, (c, r, want)
    # a window that starts in the middle of the range (on a unit boundary) and ends inside a later tile
    pos = ulist[3][0]
    r = sk.feed_lz4(img[pos:pos + 140_000], n - pos, 100_000)
    assert r["status"] == 0 and (r["consumed"], r["out_len"]) == su.expected_feed(ulist, pos, 140_000, 100_000)
    # one frame of 200 000 bytes (larger than a tile), the window ending inside it: nothing whole, need = header + payload
    import struct
    payload = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    frame = b"LZ4Block" + bytes([0x10 | 8]) + struct.pack("<iiI", len(payload), len(payload), oracle.xxh32(np.frombuffer(payload, np.uint8)) & 0x0FFFFFFF) + payload
    stream = frame + img[:ulist[1][0]]
    for c in (70_000, 131_072, len(frame) - 1):
        r = sk.feed_lz4(stream[:c], len(stream), BIG)
        assert (r["status"], r["consumed"], r["need"], r["n_frames"]) == (0, 0, len(frame), 0), (c, r)
    r = sk.feed_lz4(stream[:len(frame) + 30], len(stream), BIG)
    assert (r["status"], r["consumed"], r["out_len"], r["need"]) == (0, len(frame), 200_000, ulist[0][1]), r
