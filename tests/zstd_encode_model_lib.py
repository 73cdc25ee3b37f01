"""The host build of the product's Zstandard writer core (tests/model/zstd_encode_model.cpp) for the tests that have libzstd
and the product's decoder read its frames: a shared object for ctypes (built on demand next to its source) and an
AddressSanitizer program that writes the frames of a file of cases from heap buffers of exactly the permitted sizes."""
import ctypes
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "zstd_encode_model.cpp")
CORE = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", "zstd_encode_core.h")
BLOCK = 1 << 17
FRAME_HEADER = 14


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(CORE)) > os.path.getmtime(out)


def load():
    so = os.path.join(HERE, "model", "zstd_encode_model.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    m = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    m.ze_frame_bound.restype = i64
    m.ze_frame_bound.argtypes = [i64]
    m.ze_encode_frame.restype = i64
    m.ze_encode_frame.argtypes = [vp, i64, vp, i64]
    m.ze_encode_crafted.restype = i64
    m.ze_encode_crafted.argtypes = [vp, i64, vp, i64, vp, i64, vp, i64]
    return m


def asan_program():
    exe = os.path.join(HERE, "model", "zstd_encode_asan")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DZE_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    return exe


def pack_seqs(seqs):
    """[(literal length, match length, offset)] -> the writer's packed form."""
    return np.array([ll | ml << 18 | off << 36 for ll, ml, off in seqs], dtype=np.uint64)


def execute(lits, seqs):
    """What the sequences and literals decode to (block without history)."""
    lits = bytes(lits)
    out = bytearray()
    lp = 0
    for ll, ml, off in seqs:
        out += lits[lp:lp + ll]
        lp += ll
        assert 0 < off <= len(out) and ml >= 3
        at = len(out) - off
        if off >= ml:
            out += out[at:at + ml]
        else:
            out += (bytes(out[at:]) * (ml // off + 1))[:ml]
    out += lits[lp:]
    return np.frombuffer(bytes(out), dtype=np.uint8)


def encode_frame(model, src):
    src = np.ascontiguousarray(src, dtype=np.uint8)
    cap = int(model.ze_frame_bound(src.size))
    out = np.empty(max(cap, 1), dtype=np.uint8)
    r = int(model.ze_encode_frame(src.ctypes.data, src.size, out.ctypes.data, cap))
    assert 0 <= r <= cap
    return out[:r].copy()


def encode_crafted(model, lits, seqs):
    """(frame, content) of one block written from the given sequences."""
    lits = np.ascontiguousarray(np.frombuffer(bytes(lits), dtype=np.uint8))
    content = execute(lits.tobytes(), seqs)
    packed = pack_seqs(seqs)
    cap = int(model.ze_frame_bound(content.size))
    out = np.empty(cap, dtype=np.uint8)
    r = int(model.ze_encode_crafted(content.ctypes.data, content.size, packed.ctypes.data if len(seqs) else None, len(seqs),
                                    lits.ctypes.data, lits.size, out.ctypes.data, cap))
    assert 0 < r <= cap
    return out[:r].copy(), content


def run_asan(cases, workdir):
    """cases: [("parse", content)] or [("crafted", content, seqs, lits)] -> the frames the sanitised program wrote."""
    path_in, path_out = os.path.join(workdir, "cases.bin"), os.path.join(workdir, "frames.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            content = np.ascontiguousarray(c[1], dtype=np.uint8)
            if c[0] == "parse":
                f.write(struct.pack("<IQQQ", 0, content.size, 0, 0))
                f.write(content.tobytes())
            else:
                packed, lits = pack_seqs(c[2]), bytes(c[3])
                f.write(struct.pack("<IQQQ", 1, content.size, len(packed), len(lits)))
                f.write(content.tobytes() + packed.tobytes() + lits)
    r = subprocess.run([asan_program(), path_in, path_out], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    frames = []
    with open(path_out, "rb") as f:
        for _ in cases:
            (sz,) = struct.unpack("<q", f.read(8))
            frames.append(np.frombuffer(f.read(max(sz, 0)), dtype=np.uint8))
    return frames


def first_block(frame):
    """(block type, literals type, size format, weight header byte) of the frame's first block; size format = Huffman
    literals: the field itself (0: 1 stream; 1, 2, 3: 4 streams, header of 3, 4, 5 bytes), Raw / RLE literals: bytes of the header."""
    h = int.from_bytes(bytes(frame[FRAME_HEADER:FRAME_HEADER + 3]), "little")
    btype = (h >> 1) & 3
    if btype != 2:
        return btype, None, None, None
    b = bytes(frame[FRAME_HEADER + 3:FRAME_HEADER + 16])
    lt, sf = b[0] & 3, (b[0] >> 2) & 3
    wh = None
    if lt == 2:
        wh = b[(3, 3, 4, 5)[sf]]
    else:
        sf = (1, 2, 1, 3)[sf]
    return btype, lt, sf, wh
