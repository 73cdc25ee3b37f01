"""The host build of the block-parallel Zstandard path (tests/model/zstd_block_parallel_model.cpp) and the frames its tests
share: frames of the host build of the product's writer, frames crafted with tests/zstd_writer.py whose second block does one
thing a block on its own cannot (or just can), and a few whose headers are off.  TEST INFRASTRUCTURE."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import zstd_encode_model_lib as E
import zstd_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "zstd_block_parallel_model.cpp")
CORE = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", "zstd_decode_core.h")
B = 1 << 17
WINDOW_128K = (7, 0)  # window descriptor 0x38


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(CORE)) > os.path.getmtime(out)


def load():
    so = os.path.join(HERE, "model", "zstd_block_parallel_model.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    m = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    m.zb_decode.argtypes = [vp, i64, vp, i64, ctypes.c_int, ctypes.POINTER(i64), vp, vp, ctypes.c_int32]
    return m


def asan_program():
    exe = os.path.join(HERE, "model", "zstd_block_parallel_asan")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DZB_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    return exe


class Result:
    pass


def decode(model, comp, cap, window_rule=True):
    """The full path of the model on one partition.  The destination has exactly `cap` bytes in front of a guard band."""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    guard = 64
    out = np.full(max(cap, 0) + guard, 0xA5, dtype=np.uint8)
    total = ctypes.c_int64(-1)
    info = np.zeros(8, np.int64)
    dep = np.full(16, -1, np.int32)
    r = Result()
    r.rc = int(model.zb_decode(comp.ctypes.data, comp.size, out.ctypes.data, cap, 1 if window_rule else 0, ctypes.byref(total), info.ctypes.data,
                               dep.ctypes.data, 16))
    assert np.all(out[cap:] == 0xA5), "wrote past the destination"
    r.candidates, r.eligible, r.table_blocks, r.independent_blocks, r.dependent_frames, r.path_blocks, r.outside_slot, r.serial_rc = (int(v) for v in info)
    r.frame_dependent = [int(v) for v in dep[:r.candidates]]
    r.out = out[:total.value].copy() if r.rc == 0 else None
    return r


def block_headers(frame, at=14):
    """[(last, type, Block_Size)] of a frame whose header has `at` bytes."""
    frame = bytes(frame)
    out = []
    while True:
        h = int.from_bytes(frame[at:at + 3], "little")
        last, t, size = h & 1, (h >> 1) & 3, h >> 3
        out.append((last, t, size))
        at += 3 + (1 if t == 1 else size)
        if last:
            return out


# ---- sources ------------------------------------------------------------------------------------------------------------------
_cache = {}


def text(n, seed=17):
    key = ("text", seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(200)]
        _cache[key] = np.frombuffer(b" ".join(words[int(i)] for i in rng.integers(0, 200, 120_000)), dtype=np.uint8)
    t = _cache[key]
    assert n <= t.size
    return t[:n]


def writer_sources():
    """name -> (source, expected block count): the content sizes around the block size, and one frame of an RLE, a Raw and
    a Compressed block with one more byte behind them."""
    if "sources" not in _cache:
        rng = np.random.default_rng(5)
        mixed = np.concatenate([np.full(B, 0x33, np.uint8), rng.integers(0, 256, B, dtype=np.uint8), text(B + 1)])
        _cache["sources"] = {"b+1": (text(B + 1), 2), "2b": (text(2 * B), 2), "2b+1": (text(2 * B + 1), 3), "mixed": (mixed, 4)}
    return _cache["sources"]


def writer_frame(name):
    key = ("wframe", name)
    if key not in _cache:
        _cache[key] = E.encode_frame(E.load(), writer_sources()[name][0])
    return _cache[key]


def _filler(n, lits=b"filler-"):
    """A compressed block of exactly n bytes that stands alone: its literals, then a long run of the last one."""
    rest = n - len(lits)
    a = min(rest, 65000)
    seqs = [(len(lits), a, 1)]
    if rest - a:
        assert rest - a >= 3
        seqs.append((0, rest - a, 1))
    return lits, seqs


def crafted(case):
    """(frame, content or None when the frame is invalid, is block-independent) of the frames of the issue's list: window 2^17,
    8-byte content size, block 0 decodes to one full block, block 1 does the one thing the case is about."""
    key = ("crafted", case)
    if key in _cache:
        return _cache[key]
    f = W.Frame(fcs_bytes=8, window=WINDOW_128K, strict=case != "g")
    first = np.random.default_rng(3).integers(0, 256, B, dtype=np.uint8).tobytes()
    independent = False
    if case == "a":    # Offset_Value 1: the first repeat offset (1 at the start of a frame)
        f.raw(first).compressed(b"abcdefgh", [(8, 40, -1)])
    elif case == "b":  # a match whose source begins one byte in front of the block
        f.raw(first).compressed(b"abcdefgh", [(3, 9, 4)])
    elif case == "c":  # a match whose source is the block's first byte, overlapping forward: legal on its own
        f.raw(first).compressed(b"abcdefgh", [(3, 40, 3)])
        independent = True
    elif case == "d":  # treeless literals: the tree of block 0
        lits = bytes(text(B - 40))  # (mostly literals: the frame keeps the ratio of ordinary data, not that of a run)
        f.compressed(lits, [(B - 40, 40, 1)], lit="huf", lit_sf=3, streams=4)
        f.compressed(lits[:1500], [(700, 30, 20)], lit="treeless", lit_sf=2, streams=4)
    elif case == "e":  # the literal-length table of block 0 again
        lits, seqs = _filler(B - 48)
        seqs = [(2, 20, 2), (5, 28, 3)] + [(len(lits) - 7, seqs[0][1], 1)] + seqs[1:]
        f.compressed(lits, seqs, modes=("fse", "predef", "predef"))
        f.compressed(b"0123456789", [(2, 20, 2), (5, 30, 3)], modes=("repeat", "predef", "predef"))
    elif case == "f":  # a block that is not the last and decodes to one byte less than a block
        f.raw(first).compressed(*_filler(B - 1)).raw(b"the end")
    elif case == "g":  # ... and one that decodes to one byte more: no valid frame has it (a block is at most 128 KiB)
        f.raw(first).compressed(*_filler(B + 1)).raw(b"the end")
    else:
        raise KeyError(case)
    frame, content = f.finish()
    res = (np.frombuffer(frame, np.uint8), None if case == "g" else np.frombuffer(content, np.uint8), independent)
    _cache[key] = res
    return res


def libzstd_frame():
    """300 KB written by libzstd in one call: single segment, content size in the header, matches across its blocks."""
    if "libzstd" not in _cache:
        from oracle import zstd_ref

        piece = np.random.default_rng(9).integers(0, 256, 50_000, dtype=np.uint8)
        src = np.tile(piece, 6)
        _cache["libzstd"] = (zstd_ref.compress(src, 3), src)
    return _cache["libzstd"]


def raw_frame(window, sizes=(B, B), strict=True):
    """Raw blocks of the given sizes under the given window descriptor."""
    rng = np.random.default_rng(21)
    f = W.Frame(fcs_bytes=8, window=window, strict=strict)
    for n in sizes:
        f.raw(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    frame, content = f.finish()
    return np.frombuffer(frame, np.uint8), np.frombuffer(content, np.uint8)


def write_cases(path, cases):
    """cases: [(source bytes, content or None, window rule, candidate frames, dependent frames, blocks on the path)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for comp, content, rule, cand, dep, blocks in cases:
            comp = np.ascontiguousarray(comp, dtype=np.uint8)
            f.write(struct.pack("<qqiiii", comp.size, -1 if content is None else content.size, 1 if rule else 0, cand, dep, blocks))
            f.write(comp.tobytes())
            if content is not None:
                f.write(np.ascontiguousarray(content, dtype=np.uint8).tobytes())
