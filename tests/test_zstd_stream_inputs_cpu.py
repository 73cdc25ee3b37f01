"""CPU: every damaged or refused input of tests/test_gpu_decode_stream_zstd.py through the host build of the resumable decoder
under ASan / UBSan (tests/model/zstd_stream_model.cpp) before a GPU sees it: the verdict the GPU test expects is the one the
host model gives from exact-size buffers, and what was handed out before the verdict is a prefix of the source."""
from collections import Counter

import numpy as np

import zstd_stream_lib as L


def _check(cases, tmp_path):
    r = L.run_decode(cases, str(tmp_path))
    assert r.returncode == 0, "\n".join(l for l in r.stdout.splitlines() if "WRONG" in l)[-3000:] + r.stderr[-6000:]
    assert "%d cases, 0 wrong" % len(cases) in r.stdout


def test_damage_cases_are_classified(tmp_path):
    cases = []
    for name in L.DAMAGE_NAMES:
        img, index, sums, algo, want, prefix = L.damage_cases()[name]
        if want == L.E_CHECKSUM:  # (the shuffle checksum is the library's host side, not the decoder's: the bytes are the undamaged frame's or a case of their own)
            continue
        a, b = int(index[1]), int(index[2])
        part = img[a:b].tobytes()
        content = prefix.tobytes()[len(L.crafted()["fcs"][1]):len(prefix) - len(L.crafted()["fcs"][1])]
        for mode in (0, 1, 2):
            cases.append((part, content, want, 10, 0, mode, []))
    assert len(cases) >= 3 * 17
    _check(cases, tmp_path)


def test_conformance_cases_are_classified(tmp_path):
    cases, expect = L.conformance_cases()
    # a feed per unit; a partition that decodes to megabytes in thousands of units (the host model copies the history from
    # allocation to allocation at every feed) takes three cuts instead
    recs = []
    for c, want in zip(cases, expect):
        small = len(c.content or b"") <= 256 << 10 and len(c.data) <= 256 << 10
        recs.append((c.data, c.content if want == 0 else None, want, 27, 0, 1 if small else 0, [] if small else [len(c.data) * q // 4 for q in (1, 2, 3)]))
    _check(recs, tmp_path)
    tally = Counter(expect)
    assert tally[0] >= 200 and tally[L.E_BAD_FRAME] >= 15 and tally[L.E_UNSUPPORTED] >= 3
    # nothing is skipped on the GPU: a frame outside the feature is an input with an expected refusal
    for c, want in zip(cases, expect):
        if c.rc != 0:
            assert want != 0, c.name


def test_refusal_cases_are_classified(tmp_path):
    c = L.crafted()
    recs = [(c[n][0], None, L.E_UNSUPPORTED, 10, 0, m, []) for n in ("checksum", "dictionary_id", "window_above", "skippable_big") for m in (0, 1)]
    _check(recs, tmp_path)
