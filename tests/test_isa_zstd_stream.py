"""The compiled kernels of a resumable Zstandard stream under the ISA interpreter (tests/isa/zstd_stream_kernel.py): the
smallest two-block window_log 10 frame, cut between the blocks, then unit by unit with every one-byte-short window, from
buffers of exactly their sizes - the device-only paths (the scalar bit cache, the 64-lane state save and load, the ring
preload from the staging area, the one-lane-per-piece walk) below a real GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))

import stream_units_zstd as U
import zstd_stream_lib as L


def _frame():
    src = L.source(6, 1500)  # text with back-references: two blocks of at most 1 KiB, Huffman literals and sequences
    frame = L.compress(src, 1, 10).tobytes()
    units = U.partition_units(frame)
    assert [u[1] & 15 for u in units] == [U.FRAME, U.COMP, U.COMP] and units[-1][1] & U.LAST
    return src.tobytes(), frame, units


def test_two_block_frame_cut_between_the_blocks(oracle):
    import zstd_stream_kernel as zk

    src, frame, units = _frame()
    cut = units[2][0]
    s = zk.Stream(frame, 10)
    st, consumed, need, out1 = s.feed(cut)  # the window ends exactly where block 2 starts
    assert (st, consumed, need) == (0, cut, 0) and s.open and len(s.hist) == min(1024, len(out1)) and s.produced == len(out1)
    st, consumed, need, out2 = s.feed(len(frame))
    assert (st, consumed, need) == (0, len(frame) - cut, 0) and not s.open
    assert out1 + out2 == src
    # the second block does use what the first left behind: without the saved state it is refused, never decoded to something else
    t = zk.Stream(frame, 10)
    t.pos, t.open, t.state, t.hist, t.window, t.produced = cut, True, bytes(zk.STATE_BYTES), b"", 1024, 0
    st, _, _, _ = t.feed(len(frame))
    assert st == -3


def test_unit_by_unit_with_one_byte_short_windows(oracle):
    import zstd_stream_kernel as zk

    src, frame, units = _frame()
    s = zk.Stream(frame, 10)
    model = U.StreamModel(frame, [0, len(frame)], 10)
    out, wend = b"", 1
    for _ in range(40):
        if s.pos == len(frame):
            break
        st, consumed, need, got = s.feed(wend)
        code, m_consumed, _, m_need, _ = model.feed(wend - (s.pos - consumed))
        assert (st, consumed, need) == (code, m_consumed, m_need), (wend, (st, consumed, need), (code, m_consumed, m_need))
        out += got
        if consumed:
            wend = min(len(frame), s.pos + 1)
        else:  # one byte short of what it asked for first: the same answer must come back
            wend = s.pos + need - 1 if wend < s.pos + need - 1 else s.pos + need
    assert s.pos == len(frame) and out == src


def test_refusal_and_corruption_at_the_header(oracle):
    import zstd_stream_kernel as zk

    c = L.crafted()
    for name, want in (("checksum", -6), ("window_above", -6), ("g_repeat", -3)):
        f = c[name][0]
        st, consumed, _, got = zk.Stream(f, 10).feed(len(f))
        assert (st, consumed, got) == (want, 0, b""), name
    src, frame, units = _frame()
    st, _, _, _ = zk.Stream(frame[:-1], 10).feed(len(frame) - 1)  # the last block runs past the partition's end
    assert st == -3
