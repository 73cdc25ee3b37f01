"""CPU: the batched feed (s3s_dstream_feed_batch*).  The symbols, the binding and the refusal that needs no device; and the
batch kernels COMPILED for gfx950 and run through the instruction interpreter (tests/isa/stream_batch_kernel.py), three
windows per launch, on the cut-position images of tests/test_isa_decode_stream.py.  Every window's buffer is exactly as long
as the window, so a kernel that reads a byte at or beyond its window's comp_len faults in the interpreter's memory; what every
window takes is compared with the stop rule restated in tests/stream_units.py."""
import ctypes
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import stream_units as su
import test_isa_decode_stream as single

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa"))
import stream_batch_kernel as sbk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
SYMBOLS = ["s3s_dstream_feed_batch_device", "s3s_dstream_feed_batch"]
LZ4, SNAPPY, LZF = 1, 2, 4
BIG = 1 << 40


# ---- symbols and binding -------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols(codec_lib):
    header = open(HEADER).read()
    import s3shuffle

    exported = subprocess.run(["nm", "-D", "--defined-only", s3shuffle.library_path()], check=True, capture_output=True, text=True).stdout
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert re.search(r"\bT %s\b" % sym, exported), sym
        assert getattr(codec_lib, sym).argtypes, sym  # bound by s3shuffle.codec.load_library
    assert "typedef struct s3s_dstream_feed_entry" in header
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()
    section = header[header.index("the batched feed (ABI 11"):]
    assert header.index("int s3s_cstream_close") < header.index("the batched feed (ABI 11")  # behind the streaming map side
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for needle in ("ONE WINDOW OF EACH OF SEVERAL STREAMS", "would have produced for that stream alone", "S3S_STATUS_NOT_RUN", "the same stream twice",
                   "do not overlap", "three host waits per call whatever n is", "committed before the decode's verdict is known",
                   "fed one by one through the single feed", "s3s_dstream_open_zstd", "the sum of comp_len + dst_capacity"):
        assert needle in flat, needle


def test_entry_struct_matches_the_binding(tmp_path):
    from s3shuffle import codec

    assert [f[0] for f in codec.FeedEntry._fields_] == ["stream", "d_comp", "comp_len", "d_dst", "dst_capacity", "result", "status", "pad"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3shuffle_codec.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(s3s_dstream_feed_entry), offsetof(s3s_dstream_feed_entry, result),\n'
                   '  offsetof(s3s_dstream_feed_entry, status), sizeof(s3s_dstream_result)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(codec.FeedEntry), codec.FeedEntry.result.offset, codec.FeedEntry.status.offset, ctypes.sizeof(codec.StreamResult)]
    assert got[0] == 88
    for m in ("feed_streams", "feed_streams_device"):
        assert hasattr(codec.Codec, m), m


def test_null_context_is_refused_before_any_device_work(codec_lib):
    from s3shuffle import codec

    arr = (codec.FeedEntry * 2)()
    arr[0].status = arr[1].status = 7
    for fn in (codec_lib.s3s_dstream_feed_batch_device, codec_lib.s3s_dstream_feed_batch):
        assert fn(None, arr, 2) == -1
        assert fn(None, None, 0) == -1
    assert [arr[0].status, arr[1].status] == [7, 7]  # (nothing is known about the entries of a call without a context)


# ---- the compiled kernels, three windows per launch -----------------------------------------------------------------------------
def _window(codec, img, index, pos, length, cap):
    w = dict(window=img[pos:pos + length], dst_capacity=cap)
    if codec == LZ4:
        w["range_left"] = len(img) - pos
    else:
        w["piece_off"], w["first_mid"], w["last_pend"] = single.pieces(index, pos, length)
    return w


def _check(codec, img, index, ulist, shapes, got):
    head = {LZ4: 21, SNAPPY: 4}.get(codec)
    for (pos, length, cap), r in zip(shapes, got):
        what = (pos, length, cap, {k: v for k, v in r.items() if k not in ("frames", "out_abs")})
        want = su.expected_feed(ulist, pos, length, cap)
        assert r["status"] == 0 and (r["consumed"], r["out_len"]) == want, (what, want)
        stop = su.expected_feed(ulist, pos, length, BIG)[0]
        assert r["stop"] == stop, what
        if stop < length:  # the window ends inside a unit: its length as far as the window shows it
            visible, ln, _ = su.unit_at(codec, img, pos + stop, pos + length, codec == SNAPPY and pos + stop in index[:-1])
            assert not visible and r["need"] == ln, (what, ln)
        else:
            assert r["need"] == 0, what
        # the frames in front of the stop are the range's units that decode to something; those in front of the cut keep their
        # payload (as an address relative to the window's) and get their place in dst, the others are empty
        exp = [u for u in ulist if pos <= u[0] and u[0] + u[1] <= pos + stop and not (codec == SNAPPY and u[1] == 16 and u[2] == 0)]
        assert r["n_frames"] == len(exp) == len(r["frames"]), what
        if r["n_frames"]:
            nxt = [u for u in exp if u[0] >= pos + want[0] and u[2] > 0]
            assert r["need_dst"] == (nxt[0][2] if r["k"] < r["n_frames"] else 0), what
        out = 0
        for j, (f, u) in enumerate(zip(r["frames"], exp)):
            h = head if head is not None else (7 if img[u[0] + 2] == 1 else 5)
            if j < r["k"]:
                assert f[:3] == (u[0] - pos + h, u[1] - h, u[2]) and r["out_abs"][j] == out, (what, j, f, u)
                out += u[2]
            else:
                assert f[:3] == (0, 0, 0) and f[4] == 0x10 and r["out_abs"][j] == 0, (what, j, f)
        assert out == want[1], what


@pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
def test_three_windows_per_launch(oracle, codec):
    """a window that ends inside a header next to one that ends on a unit boundary and one of length 1; capacities one byte below
    a unit, exactly a unit, 0 and ample; windows that start in the middle of the range"""
    img, index, data = single._image(oracle, codec)
    n = len(img)
    ulist = su.units(codec, img, index)
    u1 = ulist[1] if codec != SNAPPY else ulist[2]  # (Snappy: unit 0 is the stream header)
    first = next(u for u in ulist if u[2] > 0)
    ends = sorted({u[0] + u[1] for u in ulist})
    batches = [
        [(0, u1[0] + 3, BIG), (0, ends[1], BIG), (0, 1, BIG)],
        [(0, n, first[2] - 1), (0, n, first[2]), (0, n, 0)],
        [(0, n, first[2] + 1), (ends[1], n - ends[1], BIG), (ends[2], 1, BIG)],
        [(ends[0], n - ends[0], 2 * first[2]), (0, n, BIG), (ends[-2], n - ends[-2], BIG)],
        [(0, ends[2] - 1, BIG), (0, ends[2], 5000), (0, ends[2] + 1, 9000)],
    ]
    for c in range(2, n, max(1, n // 40)):  # a sparse sweep of cuts, three at a time with different capacities
        batches.append([(0, c, BIG), (0, min(n, c + 7), 4096), (ends[0], max(1, min(n - ends[0], c)), 8191)])
    for shapes in batches:
        got = sbk.feed_batch(codec, [_window(codec, img, index, *s) for s in shapes])
        _check(codec, img, index, ulist, shapes, got)


def test_a_window_that_left_the_batch_gets_empty_frames(oracle):
    """the `skip` of LzRange: a window with an error of its own in phase 2 (a wrong checksum, a capacity verdict) keeps its
    place in the frame table, with empty frames; its neighbours are rebased as ever"""
    img, index, data = single._image(oracle, LZ4)
    ulist = su.units(LZ4, img, index)
    wins = [_window(LZ4, img, index, 0, len(img), BIG) for _ in range(3)]
    wins[1]["skip_after_cut"] = True
    got = sbk.feed_batch(LZ4, wins)
    assert all(f[:3] == (0, 0, 0) and f[4] == 0x10 for f in got[1]["frames"]) and set(got[1]["out_abs"]) == {0}
    for i in (0, 2):
        _check(LZ4, img, index, ulist, [(0, len(img), BIG)], [got[i]])
    assert got[0]["frames"] == got[2]["frames"] and got[0]["n_frames"] == got[1]["n_frames"] > 0


def test_corruption_stays_with_its_window(oracle):
    """the status word is per window: a bad magic, a unit that crosses the end of the range, and - Snappy - corruption (-1) that
    wins over a refused claim (-2) whichever lane comes last; the healthy window next to them is untouched"""
    img, index, _ = single._image(oracle, LZ4)
    ulist = su.units(LZ4, img, index)
    bad = bytearray(img)
    bad[ulist[2][0]] ^= 1
    short = dict(_window(LZ4, img, index, 0, len(img) - 5, BIG), range_left=len(img) - 5)
    got = sbk.feed_batch(LZ4, [_window(LZ4, bytes(bad), index, 0, len(img), BIG), _window(LZ4, img, index, 0, len(img), BIG), short])
    assert [r["status"] for r in got] == [-3, 0, -3]
    _check(LZ4, img, index, ulist, [(0, len(img), BIG)], [got[1]])
    img, index, _ = single._image(oracle, SNAPPY)
    ulist = su.units(SNAPPY, img, index)
    # a partition whose one chunk claims 2^32 - 1 decoded bytes (refused), and behind it one with a zero chunk length (corrupt)
    claim = img[:16] + b"\0\0\0\5" + b"\xff\xff\xff\xff\x0f"
    zero = img[:16] + b"\0\0\0\0"
    refused = dict(window=claim, dst_capacity=BIG, piece_off=[0, len(claim)], first_mid=False, last_pend=len(claim))
    both = dict(window=claim + zero, dst_capacity=BIG, piece_off=[0, len(claim), len(claim) + len(zero)], first_mid=False,
                last_pend=len(claim) + len(zero))
    other = dict(window=zero + claim, dst_capacity=BIG, piece_off=[0, len(zero), len(claim) + len(zero)], first_mid=False,
                 last_pend=len(claim) + len(zero))
    got = sbk.feed_batch(SNAPPY, [refused, _window(SNAPPY, img, index, 0, len(img), BIG), both, other])
    assert [r["status"] for r in got] == [-6, 0, -3, -3], [r["status"] for r in got]
    _check(SNAPPY, img, index, ulist, [(0, len(img), BIG)], [got[1]])


def test_lz4_window_above_a_tile_with_a_frame_across_the_tile_edge(oracle):
    """4 KiB blocks of incompressible bytes: the image is longer than 64 KiB, a frame straddles the tile edge, and the windows
    end in the second tile - inside a header, on a unit boundary, in a payload - next to a short one"""
    rng = np.random.default_rng(31)
    data = rng.integers(0, 256, 18 * 4096 + 77, dtype=np.uint8)
    img, index, _ = oracle.compress_map_output(LZ4, 1, data, np.array([0, 9 * 4096, data.size], np.int64), 4096)
    img, index = img.tobytes(), [int(x) for x in index]
    ulist = su.units(LZ4, img, index)
    across = [u for u in ulist if u[0] < 65536 < u[0] + u[1]]
    assert len(img) > 65536 + 4096 and across and 21 < 65536 - across[0][0]
    after = [u for u in ulist if u[0] >= 65536]
    shapes = [(0, after[1][0] + 9, BIG), (0, after[2][0], 40000), (0, 1, BIG)]
    _check(LZ4, img, index, ulist, shapes, sbk.feed_batch(LZ4, [_window(LZ4, img, index, *s) for s in shapes]))
    shapes = [(0, len(img), BIG), (across[0][0], len(img) - across[0][0], 4096 * 3 + 5), (0, across[0][0] + 30, BIG)]
    _check(LZ4, img, index, ulist, shapes, sbk.feed_batch(LZ4, [_window(LZ4, img, index, *s) for s in shapes]))


@pytest.mark.parametrize("algo", [1, 2, 3], ids=["adler32", "crc32", "crc32c"])
def test_seed_step_over_the_flattened_piece_table(oracle, algo):
    """one lane per piece needs its window's base: windows of 1, 3 and 2 pieces, an empty piece among them"""
    rng = np.random.default_rng(algo)
    sum_of = {1: zlib.adler32, 2: zlib.crc32}.get(algo)
    if sum_of is None:
        sum_of = lambda b: oracle.crc32c(np.frombuffer(b, np.uint8))  # noqa: E731
    lengths = [[700], [0, 16384, 5], [65521 * 2 + 3, 1]]
    fronts, bodies = [], []
    for lens in lengths:
        for n in lens:
            fronts.append(rng.integers(0, 256, int(rng.integers(0, 900)), dtype=np.uint8).tobytes())
            bodies.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    seeds = [sum_of(f) for f in fronts]
    own = [sum_of(b) for b in bodies]
    got = sbk.checksum_seed_batch(algo, lengths, seeds, own)
    assert got == [sum_of(f + b) for f, b in zip(fronts, bodies)]
