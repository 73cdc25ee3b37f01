"""The host build of the window form of the AES-CTR pass (tests/model/aes_ctr_stream_model.cpp over the product's
aes_ctr_stream_core.h) for tests/test_aes_ctr_stream_cpu.py: a shared object for ctypes and an AddressSanitizer / UBSan program
that runs a file of windows with heap buffers of exactly the window's size.  Also the pieces of a window as the streaming
reduce side cuts them, restated."""
import ctypes
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "aes_ctr_stream_model.cpp")
CORES = [os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", f) for f in ("aes_ctr_core.h", "aes_ctr_stream_core.h")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(f) for f in [SRC] + CORES) > os.path.getmtime(out)


_MODEL = None


def load():
    global _MODEL
    if _MODEL is None:
        so = os.path.join(HERE, "model", "aes_ctr_stream_model.so")
        if _stale(so):
            subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + [SRC, "-o", so], check=True)
        m = ctypes.CDLL(so)
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        m.acw_window.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int32, i64, i64, vp, vp, vp]
        m.acw_window.restype = i64
        _MODEL = m
    return _MODEL


def asan_program():
    exe = os.path.join(HERE, "model", "aes_ctr_stream_asan")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-DACW_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS + [SRC, "-o", exe],
                       check=True)
    return exe


def pieces(index, start, end):
    """The pieces of partitions of the stored window [start, end) -> (first partition, E, front): E window-relative with
    E[0] = 0 and E[-1] = end - start; front = stored bytes of the first piece's partition in front of the window."""
    index = [int(x) for x in index]
    n = len(index) - 1
    cur = next(p for p in range(n) if index[p + 1] > start)
    E, p = [0], cur
    while p < n and index[p] < end:
        E.append(min(index[p + 1], end) - start)
        p += 1
    return cur, E, start - index[cur]


def plain_offsets(index, cur, E, front):
    """Q: where the plain bytes of every piece go - a piece whose IV is not whole in the window (or whose partition is shorter
    than one) has none."""
    Q = [0]
    for i in range(len(E) - 1):
        ln = E[i + 1] - E[i]
        if i == 0 and front > 0:
            Q.append(Q[-1] + ln)
        else:
            Q.append(Q[-1] + (ln - 16 if ln >= 16 else 0))
    return Q


def window(key, iv0, win, E, Q, front, tile_chunks=1024):
    """-> (plain bytes, gathered IVs [n, 16], cover counts per stored byte, block encryptions)"""
    k = np.frombuffer(bytes(key), np.uint8).copy()
    v = np.frombuffer(bytes(iv0), np.uint8).copy()
    w = np.ascontiguousarray(win, dtype=np.uint8)
    e, q = np.asarray(E, np.int64), np.asarray(Q, np.int64)
    n = len(E) - 1
    assert w.size == E[-1]
    out = np.zeros(max(int(Q[-1]), 1), np.uint8)
    ivs = np.zeros(16 * n, np.uint8)
    cover = np.zeros(max(w.size, 1), np.uint8)
    blocks = load().acw_window(k.ctypes.data, k.size, v.ctypes.data, w.ctypes.data if w.size else None, e.ctypes.data, q.ctypes.data, n,
                               int(front), int(tile_chunks), out.ctypes.data, ivs.ctypes.data, cover.ctypes.data)
    assert blocks >= 0
    return out[: int(Q[-1])], ivs.reshape(n, 16), cover[: w.size], int(blocks)


def run_asan(cases, workdir):
    """cases = [(key, iv0, win, E, Q, front, tile_chunks)] through the sanitised program -> [(plain, ivs, cover)]"""
    path_in, path_out = os.path.join(workdir, "windows.bin"), os.path.join(workdir, "plain.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for key, iv0, win, E, Q, front, tile_chunks in cases:
            n = len(E) - 1
            f.write(struct.pack("<I", len(key)) + bytes(key) + bytes(iv0) + struct.pack("<iqq", n, front, tile_chunks))
            f.write(np.asarray(E, np.int64).tobytes() + np.asarray(Q, np.int64).tobytes() + np.asarray(win, np.uint8).tobytes())
    r = subprocess.run([asan_program(), path_in, path_out], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = []
    with open(path_out, "rb") as f:
        for key, iv0, win, E, Q, front, _ in cases:
            n = len(E) - 1
            out.append((np.frombuffer(f.read(Q[-1]), np.uint8), np.frombuffer(f.read(16 * n), np.uint8).reshape(n, 16),
                        np.frombuffer(f.read(E[-1]), np.uint8)))
    return out
