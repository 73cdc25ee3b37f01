"""CPU: the block-parallel Zstandard path as its host build runs it - scan of the headers, every block of a
candidate frame decoded on its own, then the per-partition walk that steps over the frames that completed and decodes the
others (tests/model/zstd_block_parallel_model.cpp around csrc/zstd_decode_core.h).  Frames of the product's own writer must
complete on the block path; frames whose blocks lean on what is in front of them must be found dependent and come out of the
serial decoder; the bytes are the source's / libzstd's either way, and the verdict is always the serial decoder's."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_block_parallel_lib as Z  # noqa: E402

B = Z.B
ROOT = Z.ROOT


@pytest.fixture(scope="module")
def model():
    return Z.load()


def libzstd(frame, cap):
    from oracle import zstd_ref

    return zstd_ref.decompress(frame, cap)


# ---- the writer's frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b+1", "2b", "2b+1", "mixed"])
def test_writer_frames_decode_block_wise(model, name):
    src, n_blocks = Z.writer_sources()[name]
    frame = Z.writer_frame(name)
    assert bytes(frame[:6]) == b"\x28\xb5\x2f\xfd\xc0\x38" and int.from_bytes(bytes(frame[6:14]), "little") == src.size
    heads = Z.block_headers(frame)
    assert len(heads) == n_blocks == -(-src.size // B)
    if name == "mixed":  # an RLE, a Raw and a Compressed block (and the one byte behind them, a block of its own)
        assert [t for _, t, _ in heads[:3]] == [1, 0, 2]
    r = Z.decode(model, frame, src.size)
    assert r.rc == 0 and r.serial_rc == 0
    assert r.candidates == 1 and r.eligible == 1
    assert r.table_blocks == n_blocks and r.independent_blocks == n_blocks and r.dependent_frames == 0
    assert r.path_blocks == n_blocks, "the frame did not complete on the block path"
    assert r.outside_slot == 0
    assert np.array_equal(r.out, src)


def test_two_frames_in_one_partition(model):
    """The segments form: concatenated frames, each judged on its own; and a writer frame behind a frame without a content size
    has no known output position, so it stays with the serial decoder."""
    from oracle import zstd_ref

    a, b = Z.writer_frame("b+1"), Z.writer_frame("2b+1")
    sa, sb = Z.writer_sources()["b+1"][0], Z.writer_sources()["2b+1"][0]
    r = Z.decode(model, np.concatenate([a, b]), sa.size + sb.size)
    assert r.rc == 0 and r.candidates == 2 and r.dependent_frames == 0 and r.path_blocks == 5 and r.outside_slot == 0
    assert np.array_equal(r.out, np.concatenate([sa, sb]))
    streamed = zstd_ref.compress_stream(sa[:70_000])
    r = Z.decode(model, np.concatenate([streamed, b]), 70_000 + sb.size)
    assert r.rc == 0 and r.candidates == 0 and r.path_blocks == 0
    assert np.array_equal(r.out, np.concatenate([sa[:70_000], sb]))
    # a dependent frame between two independent ones: the walk decodes exactly that one
    c, content_c, _ = Z.crafted("a")
    r = Z.decode(model, np.concatenate([a, c, b]), sa.size + content_c.size + sb.size)
    assert r.rc == 0 and r.candidates == 3 and r.frame_dependent == [0, 1, 0] and r.path_blocks == 5 and r.outside_slot == 0
    assert np.array_equal(r.out, np.concatenate([sa, content_c, sb]))


# ---- frames that must fall back ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_crafted_frames(model, case):
    frame, content, independent = Z.crafted(case)
    assert frame[5] == 0x38 and len(Z.block_headers(frame)) in (2, 3)
    ref = libzstd(frame, content.size)
    assert ref is not None and np.array_equal(ref, content), "libzstd does not read the crafted frame as the writer meant it"
    r = Z.decode(model, frame, content.size)
    assert r.rc == 0 and r.serial_rc == 0 and r.outside_slot == 0
    assert r.candidates == 1 and r.eligible == 1, "the headers alone cannot tell"
    assert r.frame_dependent == [0 if independent else 1]
    assert r.path_blocks == (len(Z.block_headers(frame)) if independent else 0)
    assert np.array_equal(r.out, ref)


def test_block_larger_than_its_slot(model):
    """(g) A block that is not the last and decodes to more than 128 KiB.  RFC 8878 has no such frame (Block_Maximum_Size), and
    the serial decoder has always refused it; libzstd 1.4.8 happens to decode it.  So this is the one case of the list whose
    bytes cannot be libzstd's: what must hold is that the block path writes nothing outside the block's slot, flags the frame
    dependent, and leaves the verdict - unchanged - to the serial decoder."""
    frame, _, _ = Z.crafted("g")
    assert len(Z.block_headers(frame)) == 3
    r = Z.decode(model, frame, 4 * B)
    assert r.rc == r.serial_rc == -3
    assert r.candidates == 1 and r.frame_dependent == [1] and r.path_blocks == 0 and r.outside_slot == 0


# ---- more frame cases ----------------------------------------------------------------------------------------------------------------
def test_libzstd_frame_is_kept_out_by_its_window(model):
    frame, src = Z.libzstd_frame()
    assert len(Z.block_headers(frame, at=9)) == 3  # magic, descriptor, 4-byte content size (single segment: no window byte)
    r = Z.decode(model, frame, src.size)
    assert r.rc == 0 and r.candidates == 0 and r.table_blocks == 0 and np.array_equal(r.out, src)
    # the window rule off: a candidate whose blocks do lean on each other
    r = Z.decode(model, frame, src.size, window_rule=False)
    assert r.rc == 0 and r.candidates == 1 and r.eligible == 1 and r.frame_dependent == [1] and r.path_blocks == 0 and r.outside_slot == 0
    assert np.array_equal(r.out, src)


@pytest.mark.parametrize("window", [(7, 1), (7, 7)])
def test_window_with_a_mantissa(model, window):
    frame, content = Z.raw_frame(window)
    assert frame[5] == (0x39 if window[1] == 1 else 0x3F)
    r = Z.decode(model, frame, content.size)
    assert r.rc == 0 and r.candidates == 0 and np.array_equal(r.out, content)


def test_window_below_the_block_size(model):
    """Window 2^16 under two Raw blocks of 128 KiB.  The rule is Window_Size <= 131072 and says nothing about blocks larger than
    the window (libzstd refuses the frame; the serial decoder, which ignores the window, accepts it), so the frame is eligible
    and its blocks are independent: both paths give the same bytes."""
    frame, content = Z.raw_frame((6, 0), strict=False)
    assert frame[5] == 0x30
    r = Z.decode(model, frame, content.size)
    assert r.rc == 0 and r.serial_rc == 0 and r.candidates == 1 and r.dependent_frames == 0 and r.path_blocks == 2
    assert np.array_equal(r.out, content)


def test_block_headers_must_end_with_the_frame(model):
    frame, src = Z.writer_frame("2b+1"), Z.writer_sources()["2b+1"][0]
    for damaged in (np.concatenate([frame, [0]]).astype(np.uint8), frame[:-1]):  # one byte behind the last block, one byte missing
        r = Z.decode(model, damaged, src.size)
        assert r.candidates == 1 and r.eligible == 0 and r.path_blocks == 0 and r.outside_slot == 0
        assert r.rc == r.serial_rc == -3, "the verdict is the serial decoder's"


def test_eligibility_from_the_header(model):
    """Content checksum, dictionary id field and a single block keep a frame out."""
    import zstd_writer as W

    rng = np.random.default_rng(4)
    for kw, sizes in ((dict(checksum=True), (B, 100)), (dict(did_bytes=1, did=0), (B, 100)), (dict(), (B,)), (dict(), (100,))):
        f = W.Frame(fcs_bytes=8, window=Z.WINDOW_128K, **kw)
        for n in sizes:
            f.raw(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        frame, content = f.finish()
        r = Z.decode(model, np.frombuffer(frame, np.uint8), len(content))
        assert r.rc == 0 and r.candidates == 0 and bytes(r.out) == content
    # a Raw block that is not the last and not full: the content size and the block count cannot both be right
    f = W.Frame(fcs_bytes=8, window=Z.WINDOW_128K)
    f.raw(b"x" * (B - 1)).raw(b"y" * B)
    frame, content = f.finish()
    r = Z.decode(model, np.frombuffer(frame, np.uint8), len(content))
    assert r.rc == 0 and r.candidates == 1 and r.eligible == 0 and r.path_blocks == 0 and bytes(r.out) == content


# ---- the sanitizer run ------------------------------------------------------------------------------------------------------------------
def test_sanitized_program(tmp_path):
    """The same list through a stand-alone AddressSanitizer + UBSan program: source and destination on the heap at exactly
    their sizes; it asserts bytes, verdicts, the counts below and that no block wrote outside its slot."""
    import subprocess

    cases = []
    for name, (src, n_blocks) in Z.writer_sources().items():
        cases.append((Z.writer_frame(name), src, True, 1, 0, n_blocks))
    for case in "abcdef":
        frame, content, independent = Z.crafted(case)
        cases.append((frame, content, True, 1, 0 if independent else 1, len(Z.block_headers(frame)) if independent else 0))
    cases.append((Z.crafted("g")[0], None, True, 1, 1, 0))
    lz, lsrc = Z.libzstd_frame()
    cases.append((lz, lsrc, True, 0, 0, 0))
    cases.append((lz, lsrc, False, 1, 1, 0))
    for window in ((7, 1), (7, 7)):
        frame, content = Z.raw_frame(window)
        cases.append((frame, content, True, 0, 0, 0))
    frame, content = Z.raw_frame((6, 0), strict=False)
    cases.append((frame, content, True, 1, 0, 2))
    w = Z.writer_frame("2b+1")
    cases.append((np.concatenate([w, [0]]).astype(np.uint8), None, True, 1, 1, 0))
    cases.append((w[:-1], None, True, 1, 1, 0))
    path = os.path.join(str(tmp_path), "cases.bin")
    Z.write_cases(path, cases)
    r = subprocess.run([Z.asan_program(), path], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "%d cases ok" % len(cases) in r.stdout


# ---- interface ---------------------------------------------------------------------------------------------------------------------------
def test_interface_constants():
    from s3shuffle import codec

    header = open(os.path.join(ROOT, "include", "s3shuffle_codec.h")).read()
    assert int(re.search(r"S3S_OPT_ZSTD_DECODE_VARIANT\s*=\s*(\d+)", header).group(1)) == 13 == codec.OPT_ZSTD_DECODE_VARIANT
    assert int(re.search(r"S3S_OPT_ZSTD_DECODE_BLOCKS\s*=\s*(\d+)", header).group(1)) == 14 == codec.OPT_ZSTD_DECODE_BLOCKS
    assert int(re.search(r"#define S3S_ABI_VERSION (\d+)", header).group(1)) == 11
    keys = [int(m) for m in re.findall(r"^\s+S3S_OPT_\w+ = (\d+)", header, re.M)]
    assert sorted(keys) == list(range(1, 15)), "two options share a key, or one is missing"
    assert hasattr(codec.Codec, "zstd_decode_blocks")
