"""CPU: randomly mutated Zstandard frames (tests/zstd_mutants.py, 2 000 per family) through the host builds of the three decode
paths that promise the serial decoder's answer - one workgroup per block, staged (6k, with and without the block
path in front) and the resumable stream decoder (6l) - and through their stand-alone ASan / UBSan programs.  A frame a stage does
not finish cleanly must only be flagged and judged again by the serial decoder: verdict, length and bytes are compared exactly,
mutant by mutant.  tests/test_gpu_zstd_mutants.py runs a subset of the same mutants on the device; nothing goes there that has
not passed here."""
import collections
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import zstd_block_parallel_lib as ZB
import zstd_model_lib as ZM
import zstd_mutants as M
import zstd_staged_lib as S
import zstd_stream_lib as L
import stream_units_zstd as U
from oracle import zstd_ref

SEED = 1
COUNT = 2000
STREAM_CAP = 1 << 17  # dst_capacity of every feed: one block always fits
STAGED_FAMILIES = ("flushed4k", "flushed1500", "crafted", "two_frames")

# Serial decoder accepts, the stream answers S3S_E_BAD_FRAME, libzstd accepts: the documented offset-beyond-window case (a
# stream keeps Window_Size bytes of history, the one-shot decoder has the whole frame, libzstd its whole output buffer).
STREAM_LEFTOVERS = {
    ("writer", 512): "Window_Descriptor 0x38 -> 0x1a (10 KiB) over blocks of 128 KiB: the blocks' own matches reach further back",
}


def window_log_max(family):
    return 10 if family == "wlog10" else 19


class Judged:
    pass


_judged = {}


def judged(family):
    """The family's mutants with the serial model's answers (one family is kept at a time: the accepted outputs are large)."""
    if family not in _judged:
        _judged.clear()
        j = Judged()
        j.family = family
        j.mutants = M.mutants(family, SEED, COUNT)
        model = ZM.load()
        j.at_cap = [M.serial_at(model, np.frombuffer(b, np.uint8), cap) for _, b, _, cap in j.mutants]
        _judged[family] = j
    return _judged[family]


@pytest.fixture(scope="module", params=M.FAMILIES)
def fam(request):
    return judged(request.param)


def test_the_generator_is_deterministic():
    a = M.mutants("crafted", SEED, 50)
    assert a == M.mutants("crafted", SEED, 50) and a[:20] == M.mutants("crafted", SEED, 20), "a prefix must not depend on the count"
    assert a != M.mutants("crafted", SEED + 1, 50)
    assert [len(M.seeds(f)) for f in M.FAMILIES] == [5, 5, 5, 5, 5, len(S.VALID_CASES), 5]
    for family, lo, hi in (("flushed4k", 10, 11), ("flushed1500", 14, 15), ("stream300k", 3, 3), ("writer", 3, 3), ("wlog10", 40, 400)):
        for frame, size in M.seeds(family):  # (a flushed frame ends with an empty last block)
            heads, consumed = S.block_headers(frame)
            assert consumed == len(frame) and lo <= len(heads) <= hi, (family, len(heads))
    caps = collections.Counter("size" if c == s else "more" if c == s + 4096 else "one less" if c == s - 1 else "less"
                               for _, _, s, c in M.mutants("flushed4k", SEED, COUNT))
    assert caps["size"] + caps["more"] > 0.7 * COUNT and caps["one less"] > 0.08 * COUNT and caps["less"] > 0.08 * COUNT


def test_paths_agree_with_the_serial_decoder(fam):
    """Block-parallel and staged verdict, length and bytes are the serial model's; where libzstd accepts as well, its bytes."""
    bm, gm = ZB.load(), S.load()
    verdicts = collections.Counter()
    n_staged = n_staged13 = n_path = n_same = n_strict = n_lenient = 0
    for (index, data, size, cap), (rc, out) in zip(fam.mutants, fam.at_cap):
        comp = np.frombuffer(data, np.uint8)
        where = (fam.family, index)
        verdicts[rc] += 1
        rb = ZB.decode(bm, comp, cap)  # (asserts the guard band)
        assert rb.rc == rc == rb.serial_rc, where
        assert rb.outside_slot == 0, where
        assert rc != 0 or np.array_equal(rb.out, out), where
        n_path += rb.path_blocks > 0
        for block_path in (False, True):
            rg = S.decode(gm, comp, cap, block_path=block_path)
            assert rg.rc != -1000, where
            assert rg.rc == rc == rg.serial_rc, where
            assert rc != 0 or np.array_equal(rg.out, out), where
            assert block_path or rg.path_blocks == 0
            if block_path:
                assert rg.path_blocks == rb.path_blocks, where
                n_staged13 += rg.staged_blocks > 0
            else:
                n_staged += rg.staged_blocks > 0
        ref = zstd_ref.decompress(comp, cap)
        if rc == 0 and ref is not None:
            assert np.array_equal(ref, out), where
            n_same += 1
        elif rc == 0:
            n_lenient += 1
        elif ref is not None:
            n_strict += 1
    print("%s: %d mutants, verdicts %s; blocks completed on the staged path in %d (%d behind the block path), on the block path in %d; "
          "libzstd: same bytes %d, decodes what the product refuses %d, refuses what the product decodes %d"
          % (fam.family, COUNT, dict(sorted(verdicts.items())), n_staged, n_staged13, n_path, n_same, n_strict, n_lenient))
    # not vacuous
    assert set(verdicts) <= {0, -2, -3, -6}
    assert verdicts[0] >= 0.10 * COUNT, "too few mutants are accepted: change the family's mix"
    assert COUNT - verdicts[0] >= 0.40 * COUNT, "too few mutants are refused: change the family's mix"
    assert n_same >= 0.08 * COUNT
    if fam.family in STAGED_FAMILIES:
        assert n_staged >= 0.10 * COUNT and n_staged13 >= 0.10 * COUNT, "the staged path completes too little"
    if fam.family == "writer":
        assert n_path >= 0.10 * COUNT, "the block path completes too little"


def _outside_the_stream(data, wlog):
    """The test's own header walk: does a frame of the partition carry a content checksum, a dictionary id or a window above
    window_log_max?  (Only asked of partitions the serial decoder accepts: the walk finds every frame.)"""
    at = 0
    while at < len(data):
        n, check, did, skip = S.frame_header_bytes(data, at)
        if skip:
            at += n
            continue
        if check or did or U.window_size(bytes(data[at:at + n])) > 1 << wlog:
            return True
        at += S.block_headers(data, at)[1]
    return False


def test_stream_model_against_the_serial_decoder(fam, tmp_path):
    """One feed per unit, and seeded cuts (under ASan / UBSan: the stream model is the sanitized program).  What a stream hands
    out before its verdict depends on the cuts; its verdict and, when it accepts, its bytes do not."""
    model = ZM.load()
    wlog = window_log_max(fam.family)
    free = [M.serial_free(model, np.frombuffer(b, np.uint8)) for _, b, _, _ in fam.mutants]
    cuts = M.seeded_cuts(fam.family, SEED, fam.mutants)
    leftovers = set()
    for mode in (1, 0):
        rep = L.run_report([(b, wlog, STREAM_CAP, mode, c if mode == 0 else []) for (_, b, _, _), c in zip(fam.mutants, cuts)], str(tmp_path))
        kinds = collections.Counter()
        for (index, data, _, _), (rc, out), (code, n, crc) in zip(fam.mutants, free, rep):
            where = (fam.family, index, "a feed per unit" if mode else "seeded cuts")
            assert code in (L.OK, L.E_BAD_FRAME, L.E_UNSUPPORTED), where  # (no capacity code: a block always fits a feed)
            if code == L.OK:
                assert rc == 0 and n == out.size and crc == zlib.crc32(out.tobytes()), where
                kinds["both accept"] += 1
            elif rc != 0:
                assert code == L.E_UNSUPPORTED or code == rc, where
                kinds["both refuse"] += 1
            elif code == L.E_UNSUPPORTED:
                assert _outside_the_stream(data, wlog), where
                kinds["outside the stream's feature"] += 1
            elif zstd_ref.decompress(np.frombuffer(data, np.uint8), out.size + 64) is None:
                kinds["bad frame for the stream and for libzstd"] += 1
            else:
                leftovers.add((fam.family, index))
                kinds["offset beyond the window"] += 1
        print(fam.family, "a feed per unit:" if mode else "seeded cuts:", dict(kinds))
        assert kinds["both accept"] >= 0.10 * COUNT
    assert leftovers == {k for k in STREAM_LEFTOVERS if k[0] == fam.family}, leftovers
    assert len(STREAM_LEFTOVERS) <= 0.01 * COUNT * len(M.FAMILIES)


def _run(cmd):
    r = subprocess.run(cmd, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    return r.stdout


def test_sanitized_programs(fam, tmp_path):
    """The same mutants from heap buffers of exactly their sizes into destinations of exactly their capacities: the serial core
    (zstd_asan_corpus --cap), the block-parallel model (ZB_MAIN) and the staged model (ZG_MAIN, with and without the block path
    in front), each a stand-alone program run directly.  (The stream model's program is the previous test.)  The case files are
    verdict only: a mutant has no expected frame or block counts."""
    exe = os.path.join(ZM.HERE, "model", "zstd_asan_corpus")
    src = os.path.join(ZM.HERE, "model", "zstd_asan_corpus.cpp")
    if not os.path.exists(exe) or max(os.path.getmtime(src), os.path.getmtime(S.CORE)) > os.path.getmtime(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        src, "-o", exe], check=True)
    path = os.path.join(str(tmp_path), "cases.bin")
    n = len(fam.mutants)
    # the serial core: the size pass answers first there, so the expected code is the one-shot call's
    model = ZM.load()
    with open(path, "wb") as f:
        for (_, data, _, cap), (rc, out) in zip(fam.mutants, fam.at_cap):
            size_rc = M.size_pass(model, np.frombuffer(data, np.uint8))[0] if rc != 0 else 0
            want = size_rc if size_rc != 0 else rc
            content = out.tobytes() if rc == 0 else b""
            f.write(struct.pack("<IIiq", len(data), len(content), want, cap) + data + content)
    assert "%d cases, 0 wrong" % n in _run([exe, "--cap", path])
    with open(path, "wb") as f:
        f.write(struct.pack("<I", n))
        for (_, data, _, cap), (rc, out) in zip(fam.mutants, fam.at_cap):
            f.write(struct.pack("<qqiiiiq", len(data), out.size if rc == 0 else -1, 1, -1, -1, -1, cap) + data + (out.tobytes() if rc == 0 else b""))
    assert "%d cases ok" % n in _run([ZB.asan_program(), path])
    with open(path, "wb") as f:
        f.write(struct.pack("<I", 2 * n))
        for (_, data, _, cap), (rc, out) in zip(fam.mutants, fam.at_cap):
            for with13 in (0, 1):
                f.write(struct.pack("<qqqiiii", len(data), out.size if rc == 0 else -1, cap, with13, -1, -1, -1) + data + (out.tobytes() if rc == 0 else b""))
    assert "%d cases ok" % (2 * n) in _run([S.asan_program(), path])
    os.remove(path)
