"""The contract model of a Zstandard stream (tests/stream_units_zstd.py, written from RFC 8878) against the host build of the
library's unit walk (tests/model/zstd_stream_model.cpp, `units` mode, under ASan / UBSan from windows of exactly their size):
unit lists, stop offsets, need_comp and the verdicts must agree on the same inputs."""
import numpy as np

import stream_units_zstd as U
import zstd_stream_lib as L
import zstd_writer as W


def _compare(records, tmp_path):
    got = L.run_units(records, str(tmp_path))
    for (win, pend, open_, wlog), g in zip(records, got):
        want = L.model_units(win, pend, open_, wlog)
        assert g == want, (len(win), pend, open_, wlog, g[:3], want[:3])
    return got


def _frames():
    out = [v[0] for v in L.crafted().values()]
    src = L.source(6, 64 << 10)
    out.append(L.compress(src, level=1, window_log=10).tobytes())
    return out


def test_whole_partitions(tmp_path):
    recs = [(f, len(f), False, 10) for f in _frames()] + [(f, len(f), False, 27) for f in _frames()]
    _compare(recs, tmp_path)


def test_every_one_byte_short_window(tmp_path):
    """For every unit of every frame: the windows that end one byte short of the unit's header steps and of its end, the exact
    ones and one byte more - with the frame open or not as the position says."""
    recs = []
    for f in _frames():
        try:
            units = U.partition_units(f, 27)
        except (U.Bad, U.Refused, AssertionError):
            continue
        units = units[:40]
        for off, kind, payload, n in units:
            open_ = (kind & 15) >= U.RAW
            for end in {off + 1, off + 2, off + 3, off + 5, off + 6, off + 7, off + 8, off + n - 1, off + n, off + n + 1}:
                if off < end <= len(f):
                    recs.append((f[off:end], len(f) - off, open_, 27))
    assert len(recs) > 1000
    got = _compare(recs, tmp_path)
    needs = [g[2] for g in got if g[0] == 0]
    assert needs and max(needs) <= 3 + U.MAX_BLOCK


def test_refusals_and_malformed(tmp_path):
    c = L.crafted()
    recs = []
    for name in ("checksum", "dictionary_id", "window_above", "skippable_big"):
        f = c[name][0]
        recs.append((f, len(f), False, 10))
        assert L.model_units(f, len(f), False, 10)[0] == -2, name
    ok = c["fcs"][0]
    units = U.partition_units(ok)
    last = units[-1]
    cases = {
        "block past the partition's end": (ok, len(ok) - 1),                       # the last block's payload crosses it
        "the partition ends with a frame open": (ok[:last[0]], last[0]),
        "truncated range inside a header": (ok[:3], 3),
        "reserved block type": (ok[:units[1][0]] + bytes([ok[units[1][0]] | 6]) + ok[units[1][0] + 1:], len(ok)),
        "reserved header bit": (ok[:4] + bytes([ok[4] | 8]) + ok[5:], len(ok)),
        "bad magic": (b"\x00" + ok[1:], len(ok)),
    }
    for name, (win, pend) in cases.items():
        win = win[:pend]
        assert L.model_units(win, pend, False, 27)[0] == -1, name
        recs.append((win, pend, False, 27))
    # the same bytes with the partition going on behind the window are a place to stop, not corruption
    recs.append((ok[:len(ok) - 1], len(ok), False, 27))
    assert L.model_units(ok[:len(ok) - 1], len(ok), False, 27)[0] == len(units) - 1
    _compare(recs, tmp_path)


def test_stream_model_walks_a_range():
    """StreamModel (what the GPU tests compare positions with) over a range of several partitions, against the unit lists."""
    a, b = L.crafted()["fcs"][0], L.crafted()["several_frames"][0]
    img = a + b + a
    offs = [0, len(a), len(a), len(a) + len(b), len(img)]
    ends = U.boundaries(img, offs)
    m = U.StreamModel(img, offs, 12)
    seen = [0]
    while not m.at_end:
        nxt = min(e for e in ends if e > m.pos)
        code, consumed, _, need, _ = m.feed(nxt - m.pos - 1)
        assert code == 0 and consumed == 0 and (need > 0 or nxt - m.pos - 1 == 0)
        code, consumed, _, need, _ = m.feed(nxt - m.pos)
        assert code == 0 and consumed > 0 and need == 0
        seen.append(m.pos)
    assert seen == ends
