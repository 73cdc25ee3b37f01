"""The resumable Zstandard decoder (spark-s3-shuffle_amd/csrc/zstd_stream_core.h) on the CPU, feed by feed, under ASan / UBSan
(tests/model/zstd_stream_model.cpp, a stand-alone program): every frame is decoded with a cut after every unit - also with
windows one byte short of and one byte past every unit - and with random cut sets, from buffers of exactly their sizes, with
the state record and the history moved to fresh allocations between feeds.  The output must be libzstd's."""
import numpy as np
import pytest

import zstd_stream_lib as L
from oracle import zstd_ref


def _check(cases, tmp_path):
    r = L.run_decode(cases, str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "%d cases, 0 wrong" % len(cases) in r.stdout


def _schedules(frame, content, code, wlog, rng, cap_kib=0):
    """One case per schedule: a feed per unit, one byte short / past, three random cut sets, one feed."""
    n = len(frame)
    out = [(frame, content, code, wlog, 0, 1, []), (frame, content, code, wlog, 0, 2, []), (frame, content, code, wlog, 0, 0, [])]
    for _ in range(3):
        cuts = sorted(set(int(x) for x in rng.integers(1, max(n, 2), min(12, n))))
        out.append((frame, content, code, wlog, 0, 0, cuts))
    if cap_kib:
        out.append((frame, content, code, wlog, cap_kib << 10, 0, []))
    return out


@pytest.mark.parametrize("level", [1, 3])
@pytest.mark.parametrize("window_log,n", [(10, 64 << 10), (17, 256 << 10), (0, 512 << 10)])
@pytest.mark.parametrize("flush", [0, 20000])
def test_libzstd_streaming_frames(tmp_path, level, window_log, n, flush):
    rng = np.random.default_rng([level, window_log, flush])
    cases = []
    for kind in (3, 6):
        src = L.source(kind, n)
        frame = L.compress(src, level=level, window_log=window_log, flush=flush)
        assert np.array_equal(zstd_ref.decompress(frame, src.size), src)  # libzstd's own decode is the reference
        wlog = L.frame_window_log(frame)
        assert wlog == (window_log or {1: 19, 3: 21}[level])
        if window_log == 10:
            assert len(L.unit_ends(frame)) > 40  # blocks of at most 1 KiB: dozens per frame
        cases += _schedules(frame.tobytes(), src.tobytes(), L.OK, wlog, rng, cap_kib=200)
        # a window_log_max one below the frame's refuses it at its header
        if wlog > 10:
            cases.append((frame.tobytes(), None, L.E_UNSUPPORTED, wlog - 1, 0, 0, []))
    _check(cases, tmp_path)


def test_history_is_only_what_the_stream_keeps(tmp_path):
    """200 KiB of noise twice in a window_log 18 frame: every match of the second half is 200 KiB back, across blocks and feeds."""
    half = np.random.default_rng(5).integers(0, 256, 200 << 10, dtype=np.uint8)
    src = np.concatenate([half, half])
    frame = L.compress(src, level=3, window_log=18)
    assert len(frame) < src.size * 0.6  # (the second half did become matches)
    _check([(frame.tobytes(), src.tobytes(), L.OK, 18, 0, 1, []), (frame.tobytes(), src.tobytes(), L.OK, 18, 140 << 10, 0, [])], tmp_path)


def test_library_writer_frames(tmp_path):
    import zstd_encode_model_lib as E

    m = E.load()
    rng = np.random.default_rng(11)
    cases = []
    for kind, n in ((6, 300 << 10), (3, 150 << 10), (0, 5000)):
        src = L.source(kind, n)
        frame = E.encode_frame(m, src)
        frame = np.asarray(frame, dtype=np.uint8)
        assert np.array_equal(zstd_ref.decompress(frame, src.size), src)
        cases += _schedules(frame.tobytes(), src.tobytes(), L.OK, 27, rng)
    _check(cases, tmp_path)


def test_crafted_state_across_every_cut(tmp_path):
    rng = np.random.default_rng(3)
    cases = []
    for name, (frame, content, code, wlog) in L.crafted().items():
        if content is not None:
            ref = zstd_ref.decompress(np.frombuffer(frame, np.uint8), len(content) + 16)
            assert ref is not None and ref.tobytes() == content, name
        cases += _schedules(frame, content, code, wlog, rng)
    _check(cases, tmp_path)
