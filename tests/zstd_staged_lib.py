"""The host build of the staged Zstandard path (tests/model/zstd_staged_model.cpp) and the frames its tests
share: libzstd's streaming frames (plain and flushed every 4 KiB), frames crafted with tests/zstd_writer.py - Repeat_Mode
tables and Treeless literals that lean on a block two compressed blocks back, repeat offsets and matches across block
boundaries - and invalid ones.  TEST INFRASTRUCTURE."""
import ctypes
import os
import struct
import subprocess

import numpy as np

import zstd_writer as W

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "zstd_staged_model.cpp")
CORE = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", "zstd_decode_core.h")
B = 1 << 17
KINDS = (2, 3, 4, 6, 7)
FLUSH = 4096


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(CORE)) > os.path.getmtime(out)


def load():
    so = os.path.join(HERE, "model", "zstd_staged_model.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    m = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    m.zg_decode.argtypes = [vp, i64, vp, i64, ctypes.c_int, i64, ctypes.POINTER(i64), vp, vp, ctypes.c_int32]
    m.zg_caps.argtypes = [i64, vp]
    m.zg_caps.restype = None
    return m


def staging_caps(model, comp_bytes):
    """(block table entries, literal bytes, records) of the staging of a call that holds comp_bytes compressed bytes"""
    caps = np.zeros(3, np.int64)
    model.zg_caps(comp_bytes, caps.ctypes.data)
    return tuple(int(v) for v in caps)


def asan_program():
    exe = os.path.join(HERE, "model", "zstd_staged_asan")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DZG_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    return exe


class Result:
    pass


def decode(model, comp, cap, block_path=False, budget=None):
    """The full path of the model on one partition.  The destination has exactly `cap` bytes in front of a guard band."""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    guard = 64
    out = np.full(max(cap, 0) + guard, 0xA5, dtype=np.uint8)
    total = ctypes.c_int64(-1)
    info = np.zeros(10, np.int64)
    dep = np.full(16, -1, np.int32)
    r = Result()
    r.rc = int(model.zg_decode(comp.ctypes.data, comp.size, out.ctypes.data, cap, 1 if block_path else 0, comp.size if budget is None else budget,
                               ctypes.byref(total), info.ctypes.data, dep.ctypes.data, 16))
    assert np.all(out[cap:] == 0xA5), "wrote past the destination"
    (r.frames, r.table_blocks, r.dependent_frames, r.staged_blocks, r.path_blocks, r.serial_rc, r.lit_bytes, r.records, r.treeless,
     r.repeats) = (int(v) for v in info)
    r.frame_dependent = [int(v) for v in dep[:r.frames]]
    r.out = out[:total.value].copy() if r.rc == 0 else None
    return r


# ---- a header walk of the test's own ---------------------------------------------------------------------------------------------
def frame_header_bytes(frame, at=0):
    """(header bytes, has checksum, has dictionary id, skippable payload or None) of the frame at `at`."""
    frame = bytes(frame)
    magic = int.from_bytes(frame[at:at + 4], "little")
    if magic & 0xFFFFFFF0 == 0x184D2A50:
        return 8 + int.from_bytes(frame[at + 4:at + 8], "little"), False, False, True
    assert magic == 0xFD2FB528
    fhd = frame[at + 4]
    single, did, fcs = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    n = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0) if fcs == 0 else (2, 4, 8)[fcs - 1])
    return n, bool(fhd & 4), did != 0, False


def block_headers(frame, at=0):
    """([(last, type, Block_Size)], frame bytes) of the Zstandard frame at `at`."""
    frame = bytes(frame)
    hb, check, _, skip = frame_header_bytes(frame, at)
    assert not skip
    p, out = at + hb, []
    while True:
        h = int.from_bytes(frame[p:p + 3], "little")
        last, t, size = h & 1, (h >> 1) & 3, h >> 3
        out.append((last, t, size))
        p += 3 + (1 if t == 1 else size)
        if last:
            return out, p + (4 if check else 0) - at


def staged_blocks(partition):
    """Blocks the staged path is expected to complete in one partition when nothing is in front of it: the frames from the
    start up to the first one it cannot take by its header (skippable, checksum, dictionary id, fewer than two blocks)."""
    partition = bytes(partition)
    at, n = 0, 0
    while at < len(partition):
        _, check, did, skip = frame_header_bytes(partition, at)
        if skip or check or did:
            break
        heads, size = block_headers(partition, at)
        if len(heads) < 2:
            break
        n += len(heads)
        at += size
    return n


# ---- libzstd's frames ------------------------------------------------------------------------------------------------------------
_cache = {}


def source(kind, n=512 << 10):
    key = ("src", kind, n)
    if key not in _cache:
        import corpus

        _cache[key] = corpus.chunk_corpus(kind, n, np.random.default_rng(100 + kind))
    return _cache[key]


def compress_flushed(data, level=1, chunk=FLUSH):
    """One libzstd streaming frame with ZSTD_e_flush after every `chunk` bytes: a block per chunk, history across them."""
    from oracle import zstd_ref

    z = zstd_ref.lib()
    d = np.ascontiguousarray(data, dtype=np.uint8)
    cctx = z.ZSTD_createCCtx()
    try:
        z.ZSTD_CCtx_setParameter(cctx, zstd_ref.ZSTD_c_compressionLevel, level)
        cap = int(z.ZSTD_compressBound(d.size)) + 16 * (d.size // chunk + 2) + 1024
        out = np.empty(cap, dtype=np.uint8)
        ob = zstd_ref._Buf(out.ctypes.data, cap, 0)
        pos = 0
        while pos < d.size:
            n = min(chunk, d.size - pos)
            ib = zstd_ref._Buf(d.ctypes.data + pos, n, 0)
            while True:
                r = z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), zstd_ref.ZSTD_e_flush)
                assert not z.ZSTD_isError(r)
                if r == 0 and ib.pos == ib.size:
                    break
            pos += n
        ib = zstd_ref._Buf(d.ctypes.data, 0, 0)
        while True:
            r = z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), zstd_ref.ZSTD_e_end)
            assert not z.ZSTD_isError(r)
            if r == 0:
                break
        return out[:ob.pos].copy()
    finally:
        z.ZSTD_freeCCtx(cctx)


def libzstd_frame(kind, flushed, n=512 << 10):
    key = ("lz", kind, flushed, n)
    if key not in _cache:
        from oracle import zstd_ref

        src = source(kind, n)
        _cache[key] = (compress_flushed(src) if flushed else zstd_ref.compress_stream(src, 1), src)
    return _cache[key]


# ---- crafted frames --------------------------------------------------------------------------------------------------------------
def _hist(n=300, seed=1):
    return bytes(np.random.default_rng([seed, 5]).integers(0, 256, n, dtype=np.uint8))


def _text(n, seed=3):
    rng = np.random.default_rng([seed, 77])
    p = np.array([2.0 ** (i * 5 % 7) for i in range(40)])
    return bytes((rng.choice(40, n, p=p / p.sum()) + 48).astype(np.uint8))


SEQS_A = [(0, 3, 5), (3, 10, 30), (17, 36, -1), (40, 70, 60)]


def _repeat_frame(fields, first):
    """Block 0 history; block 1 defines LL / OF / ML in mode `first`; a raw block and a block without sequences; block 4 takes
    another set of tables (so the defining block is two compressed blocks back); block 5 repeats `fields` of block 1."""
    f = W.Frame()
    f.raw(_hist())
    if first == "rle":
        seqs = [(5, 7, 9), (5, 7, 9), (5, 7, 9)]
        lits = b"abcdefghijklmnopqrstu"
    else:
        seqs = SEQS_A
        lits = _text(70)
    f.compressed(lits, seqs, modes=(first,) * 3)
    f.raw(b"a raw block between")
    f.compressed(b"only literals", [])
    # block 4: a compressed block with sequences that repeats `fields` too and defines the others anew (predef <-> fse)
    other = "fse" if first == "predef" else "predef"
    f.compressed(lits, seqs, modes=tuple("repeat" if k in fields else other for k in range(3)))
    f.compressed(b"nothing here", [])
    f.compressed(lits, seqs, modes=tuple("repeat" if k in fields else other for k in range(3)))
    return f


def crafted(case):
    """name -> (partition bytes, content or None when it must be refused, expected staged blocks)"""
    key = ("crafted", case)
    if key in _cache:
        return _cache[key]
    blocks = None
    if case.startswith("a_"):  # Repeat_Mode: a_<fields>_<mode of the defining block>
        _, fields, first = case.split("_")
        f = _repeat_frame([{"ll": 0, "of": 1, "ml": 2}[x] for x in fields.split("+")], first)
        data, content = f.finish()
    elif case == "b":  # treeless literals whose tree is two blocks back
        t = _text(1500)
        f = W.Frame()
        f.compressed(t, [(700, 30, 20)], lit="huf", lit_sf=2, streams=4)
        f.compressed(b"raw literals in between", [(4, 9, 100)])
        f.raw(b"and a raw block")
        f.compressed(t[:900], [(100, 12, 7)], lit="treeless", lit_sf=2, streams=4)
        f.compressed(t[200:260], [], lit="treeless", lit_sf=0, streams=1)
        data, content = f.finish()
    elif case == "c":  # repeat codes 1, 2, 3 at the start of a block, literal length 0 and not: the previous block's history
        f = W.Frame()
        f.raw(_hist(400))
        f.compressed(b"0123456789", [(2, 8, 100), (2, 9, 200), (2, 10, 300)])
        f.compressed(b"abcdefghijkl", [(0, 5, -1), (0, 6, -2), (0, 7, -3), (3, 5, -1), (3, 6, -2), (3, 7, -3), (0, 4, 57), (0, 9, -3)])
        f.compressed(b"xy", [(1, 5, -3), (0, 5, -1)])
        data, content = f.finish()
    elif case == "d":  # a match that starts in the previous block, one that reaches the frame's first byte, an overlapping one across a boundary
        f = W.Frame()
        f.raw(b"The quick brown fox jumps over the lazy dog")
        f.compressed(b"AB", [(1, 20, 10), (1, 43 - 0, 43 + 1 + 20 + 1)])
        f.compressed(b"", [(0, 50, 3), (0, 30, 1)])
        data, content = f.finish()
    elif case == "e":  # RLE literals with RLE tables, and a zero-length last raw block
        f = W.Frame()
        f.raw(_hist(100))
        f.compressed(b"z" * 15, [(5, 7, 9), (5, 7, 9), (5, 7, 9)], lit="rle", modes=("rle", "rle", "rle"))
        f.raw(b"")
        data, content = f.finish()
    elif case == "fcs":  # a stated Frame_Content_Size that the blocks do add up to
        f = W.Frame(fcs_bytes=4)
        f.raw(_hist(60))
        f.compressed(b"abcdef", [(3, 5, 20), (2, 6, 9)])
        f.raw(_hist(40, seed=2))
        data, content = f.finish()
    elif case in ("g_fcs_large", "g_fcs_small"):  # blocks that decode cleanly, one byte short of / beyond the stated Frame_Content_Size
        f = W.Frame(fcs_bytes=4, strict=False)
        f.raw(_hist(60))
        f.compressed(b"abcdef", [(3, 5, 20), (2, 6, 9)])
        f.fcs_value = len(f.out) + (1 if case == "g_fcs_large" else -1)
        data, content = f.finish()
        content = None
    elif case == "g_offset":  # an offset one byte beyond the history
        f = W.Frame(strict=False)
        f.raw(_hist(50))
        f.compressed(b"abc", [(3, 5, 54)])
        data, content = f.finish()
        content = None
    elif case == "g_rep3":  # repeat code 3 with rep0 == 1 and literal length 0: offset 0
        f = W.Frame(strict=False)
        f.raw(_hist(50))
        f.compressed(b"abc", [(0, 5, -3)])
        data, content = f.finish()
        content = None
    elif case == "g_bit":  # a sequence stream with a bit left over
        f = W.Frame()
        f.raw(_hist(50))
        f.compressed(b"abcdef", [(3, 5, 20), (2, 6, 9)])
        data, content = f.finish()
        body = f.blocks[1][1]
        stream = int.from_bytes(body[9:], "little") << 1  # (1 + 6 bytes of raw literals, Number_of_Sequences, modes: then the stream)
        new = body[:9] + stream.to_bytes((stream.bit_length() + 7) // 8, "little")
        data = data[:len(data) - len(body) - 3] + (1 | 2 << 1 | len(new) << 3).to_bytes(3, "little") + new
        content = None
    elif case == "g_repeat":  # Repeat_Mode with nothing in front
        f = W.Frame(strict=False)
        f.raw(_hist(50))
        f.compressed(b"abcdef", [(3, 5, 20)], modes=("repeat", "predef", "predef"))
        data, content = f.finish()
        content = None
    elif case == "g_regen":  # a regenerated size above what the compressed literals can hold
        t = _text(200)
        f = W.Frame()
        f.raw(_hist(50))
        f.compressed(t, [], lit="huf", lit_sf=2, streams=4)
        data, content = f.finish()
        data = bytearray(data)
        at = len(data) - len(f.blocks[1][1])
        v = int.from_bytes(data[at:at + 4], "little")
        comp = v >> 18
        assert 8 * comp + 257 < 1 << 14
        v = (v & 0xF) | ((8 * comp + 257) << 4) | (comp << 18)
        data[at:at + 4] = v.to_bytes(4, "little")
        data, content = bytes(data), None
    elif case == "g_nseq":  # an nseq claim that passes the staging budget
        f = W.Frame()
        f.raw(_hist(50))
        f.compressed(b"abcdef", [(3, 5, 20)], modes=("rle", "rle", "rle"))
        data, content = f.finish()
        body = f.blocks[1][1]
        assert body[7] == 1  # (1-byte raw literals header, 6 literals, then Number_of_Sequences)
        new = body[:7] + b"\xff\xff\xff" + body[8:]
        data = bytearray(data[:len(data) - len(body) - 3])
        data += (1 | 2 << 1 | len(new) << 3).to_bytes(3, "little") + new
        data, content = bytes(data), None
        blocks = 0
    else:
        raise KeyError(case)
    if blocks is None:
        blocks = staged_blocks(data) if content is not None else 0
    res = (np.frombuffer(data, np.uint8), None if content is None else np.frombuffer(content, np.uint8), blocks)
    _cache[key] = res
    return res


REPEAT_CASES = ["a_ll_fse", "a_of_fse", "a_ml_fse", "a_ll+of+ml_fse", "a_ll+of+ml_rle", "a_ll+of+ml_predef", "a_of_predef", "a_ml_rle"]
VALID_CASES = REPEAT_CASES + ["b", "c", "d", "e", "fcs"]
INVALID_CASES = ["g_offset", "g_rep3", "g_bit", "g_fcs_large", "g_fcs_small", "g_repeat", "g_regen", "g_nseq"]
FLAGGED_CASES = INVALID_CASES[:5]  # taken by the header walk and flagged by a later stage; the others are not eligible


def write_cases(path, cases):
    """cases: [(source bytes, content or None, capacity, block path in front, staged frames, dependent frames, staged blocks)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for comp, content, cap, with13, frames, dep, blocks in cases:
            comp = np.ascontiguousarray(comp, dtype=np.uint8)
            f.write(struct.pack("<qqqiiii", comp.size, -1 if content is None else content.size, cap, 1 if with13 else 0, frames, dep, blocks))
            f.write(comp.tobytes())
            if content is not None:
                f.write(np.ascontiguousarray(content, dtype=np.uint8).tobytes())
