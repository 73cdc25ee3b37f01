"""CPU: the staged Zstandard path as its host build runs it - scan of the headers, entropy of every block on its
own (in reverse order, so that nothing can lean on an earlier block's having run), place, copy, execute per frame, then the
per-partition walk that steps over the frames that completed and decodes the others (tests/model/zstd_staged_model.cpp around
csrc/zstd_decode_core.h).  libzstd's streaming frames and crafted frames with Repeat_Mode tables, Treeless literals, repeat
offsets and matches across block boundaries must complete on the staged path; invalid frames must be flagged and get the
serial decoder's verdict; the bytes are the source's either way."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_staged_lib as S  # noqa: E402

B = S.B
N_GENERATED = 400


@pytest.fixture(scope="module")
def model():
    return S.load()


def _complete(r, want_blocks, frames=1):
    assert r.rc == 0 and r.serial_rc == 0
    assert r.frames == frames and r.dependent_frames == 0 and r.frame_dependent == [0] * frames, "the frame table is not complete"
    assert r.table_blocks == want_blocks and r.staged_blocks == want_blocks, "the frame did not complete on the staged path"


# ---- libzstd's frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flushed", [False, True])
@pytest.mark.parametrize("kind", S.KINDS)
def test_libzstd_frames(model, kind, flushed):
    comp, src = S.libzstd_frame(kind, flushed)
    heads, size = S.block_headers(comp)
    assert size == comp.size
    assert len(heads) == (129 if flushed else 5), "libzstd cut the frame differently: %d blocks" % len(heads)
    assert S.staged_blocks(comp) == len(heads)
    r = S.decode(model, comp, src.size)
    _complete(r, len(heads))
    assert np.array_equal(r.out, src)
    if flushed and kind in (2, 6):
        assert r.treeless == 127, "the frame no longer leans on block 0's tree"
    if kind == 4:
        assert r.records == 0 and r.lit_bytes > 0 and (r.treeless > 0) == flushed
    if kind == 3:
        assert r.lit_bytes == 0 and r.records > 0
    assert r.repeats == 0  # (libzstd level 1 writes no Repeat_Mode table here: the crafted frames below do)


def test_libzstd_frame_with_a_window_log(model):
    """Window 2^19 said in the header (zstd-jni's frames): any window is eligible."""
    from oracle import zstd_ref

    src = S.source(6)
    comp = zstd_ref.compress_stream(src, 1, window_log=19)
    r = S.decode(model, comp, src.size)
    _complete(r, len(S.block_headers(comp)[0]))
    assert np.array_equal(r.out, src)


# ---- crafted frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.VALID_CASES)
def test_crafted_frames(model, case):
    from oracle import zstd_ref

    data, content, blocks = S.crafted(case)
    ref = zstd_ref.decompress(data, content.size + 64)
    assert ref is not None and np.array_equal(ref, content), "libzstd does not read the crafted frame as the writer meant it"
    assert blocks == len(S.block_headers(data)[0]) >= 3
    r = S.decode(model, data, content.size)
    _complete(r, blocks)
    assert np.array_equal(r.out, content)
    if case.startswith("a_"):
        n = len(case.split("_")[1].split("+"))
        assert r.repeats == 2 * n, "blocks 4 and 5 repeat the tables of block 1"
    if case == "b":
        assert r.treeless == 2
    # one byte less room: the staged frame would pass the capacity, so it is flagged and the serial decoder answers
    r = S.decode(model, data, content.size - 1)
    assert r.rc == r.serial_rc == -2 and r.dependent_frames == 1 and r.staged_blocks == 0


def test_two_frames_in_one_partition(model):
    import zstd_block_parallel_lib as Z
    import zstd_writer as W

    a, ca, na = S.crafted("c")
    b, cb, nb = S.crafted("a_ll+of+ml_fse")
    r = S.decode(model, np.concatenate([a, b]), ca.size + cb.size)
    _complete(r, na + nb, frames=2)
    assert np.array_equal(r.out, np.concatenate([ca, cb]))
    # a block-independent frame of the product's writer in front: key 13's path claims it, the staged walk starts behind it
    w, ws = Z.writer_frame("b+1"), Z.writer_sources()["b+1"][0]
    r = S.decode(model, np.concatenate([w, a]), ws.size + ca.size, block_path=True)
    _complete(r, na)
    assert r.path_blocks == 2 and np.array_equal(r.out, np.concatenate([ws, ca]))
    # ... and without that path the staged one takes both frames
    r = S.decode(model, np.concatenate([w, a]), ws.size + ca.size, block_path=False)
    _complete(r, 2 + na, frames=2)
    assert r.path_blocks == 0 and np.array_equal(r.out, np.concatenate([ws, ca]))
    # a checksum frame, a skippable frame behind: the walk stops there, what lies behind is the serial decoder's
    f = W.Frame(checksum=True)
    f.raw(b"with a checksum").raw(b" in two blocks")
    chk, cchk = f.finish()
    for behind, more in ((np.frombuffer(chk, np.uint8), np.frombuffer(cchk, np.uint8)),
                         (np.frombuffer(W.skippable(b"skip me") + bytes(b), np.uint8), cb)):
        r = S.decode(model, np.concatenate([a, behind]), ca.size + more.size)
        _complete(r, na)
        assert np.array_equal(r.out, np.concatenate([ca, more]))


@pytest.mark.parametrize("case", S.INVALID_CASES)
def test_invalid_frames(model, case):
    data, content, _ = S.crafted(case)
    assert content is None
    r = S.decode(model, data, 4096)
    assert r.rc == r.serial_rc == -3, "the verdict is the serial decoder's"
    assert r.staged_blocks == 0
    if case in S.FLAGGED_CASES:
        assert r.frames == 1 and r.frame_dependent == [1], "the staged path must flag the frame"
    else:
        assert r.frames == 0, "not eligible from its headers"
    # behind a valid frame: that one completes, the invalid one decides the partition
    ok, cok, nok = S.crafted("d")
    r = S.decode(model, np.concatenate([ok, data]), 4096)
    assert r.rc == r.serial_rc == -3 and r.frame_dependent[0] == 0
    # ... and in front of one: the valid frame behind it is left to the serial decoder too, which never gets there
    r = S.decode(model, np.concatenate([data, ok]), 4096)
    assert r.rc == r.serial_rc == -3 and r.staged_blocks == 0


def test_budget_scales_with_the_call(model):
    """The nseq claim fits a staging sized for a larger call: then the frame is taken, fails in the entropy stage and is flagged."""
    data, _, _ = S.crafted("g_nseq")
    r = S.decode(model, data, 4096, budget=1 << 20)
    assert r.rc == r.serial_rc == -3 and r.frames == 1 and r.frame_dependent == [1]


# ---- the conformance corpus --------------------------------------------------------------------------------------------------------
def test_conformance_corpus(model):
    import zstd_conformance as C

    cases = C.fixed_corpus() + [C.generated_case(seed) for seed in range(N_GENERATED)]
    inside, demand = 0, np.zeros(3, np.int64)
    for c in cases:
        if not c.data:
            continue
        comp = np.frombuffer(c.data, np.uint8)
        cap = len(c.content) if c.content is not None else 1 << 17
        for budget in (comp.size, 1 << 22):  # staging sized for the partition alone, and for a call of 4 MiB
            r = S.decode(model, comp, cap, budget=budget)
            assert r.rc != -1000, "%s: the staged path and the serial decoder disagree" % c.name
            assert r.rc == r.serial_rc == c.rc, c.name
            if c.content is not None:
                assert r.out.tobytes() == c.content, c.name
        if c.content is not None:  # with room in the staging every frame the header walk finds completes
            assert r.staged_blocks == S.staged_blocks(c.data), c.name
            if len(c.content) <= 8 * comp.size + 4096 and comp.size >= 12:
                inside += comp.size
                demand += np.array([r.table_blocks, r.lit_bytes, r.records])
    # one call that holds every valid partition inside the single pass's guess (tests/test_gpu_zstd_staged.py) has staging for
    # all of them, so there the count is exact as well
    assert np.all(demand <= np.array(S.staging_caps(model, inside))), (demand, S.staging_caps(model, inside))


# ---- the sanitizer run ----------------------------------------------------------------------------------------------------------------
def test_sanitized_program(tmp_path):
    """The lists above through a stand-alone AddressSanitizer + UBSan program: source, staging and destination on the heap at
    exactly their sizes; it asserts bytes, verdicts and the counts below."""
    import zstd_block_parallel_lib as Z
    import zstd_conformance as C

    cases = []
    for kind in S.KINDS:
        for flushed in (False, True):
            comp, src = S.libzstd_frame(kind, flushed)
            cases.append((comp, src, src.size, False, 1, 0, 129 if flushed else 5))
    for case in S.VALID_CASES:
        data, content, blocks = S.crafted(case)
        cases.append((data, content, content.size, False, 1, 0, blocks))
        cases.append((data, None, content.size - 1, False, 1, 1, 0))
    for case in S.INVALID_CASES:
        data, _, _ = S.crafted(case)
        flagged = case in S.FLAGGED_CASES
        cases.append((data, None, 4096, False, 1 if flagged else 0, 1 if flagged else 0, 0))
    a, ca, na = S.crafted("c")
    w, ws = Z.writer_frame("b+1"), Z.writer_sources()["b+1"][0]
    cases.append((np.concatenate([w, a]), np.concatenate([ws, ca]), ws.size + ca.size, True, 1, 0, na))
    cases.append((np.concatenate([w, a]), np.concatenate([ws, ca]), ws.size + ca.size, False, 2, 0, na + 2))
    model = S.load()
    for c in C.fixed_corpus() + [C.generated_case(seed) for seed in range(100)]:
        if not c.data:
            continue
        comp = np.frombuffer(c.data, np.uint8)
        cap = len(c.content) if c.content is not None else 1 << 17
        r = S.decode(model, comp, cap)  # (the counts of the plain build: the program must repeat them under the sanitizers)
        cases.append((comp, None if c.content is None else np.frombuffer(c.content, np.uint8), cap, False, r.frames, r.dependent_frames, r.staged_blocks))
    path = os.path.join(str(tmp_path), "cases.bin")
    S.write_cases(path, cases)
    r = subprocess.run([S.asan_program(), path], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d cases ok" % len(cases) in r.stdout


# ---- interface ---------------------------------------------------------------------------------------------------------------------------
def test_interface_constants():
    from s3shuffle import codec

    header = open(os.path.join(S.ROOT, "include", "s3shuffle_codec.h")).read()
    assert int(re.search(r"S3S_OPT_ZSTD_DECODE_STAGED\s*=\s*(\d+)", header).group(1)) == 15 == codec.OPT_ZSTD_DECODE_STAGED
    assert int(re.search(r"S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS\s*=\s*(\d+)", header).group(1)) == 16 == codec.OPT_ZSTD_DECODE_STAGED_BLOCKS
    assert int(re.search(r"#define S3S_ABI_VERSION (\d+)", header).group(1)) == 11
    assert hasattr(codec.Codec, "zstd_decode_staged_blocks")
