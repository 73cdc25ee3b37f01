"""The host build of the product's Zstandard decoder core (tests/model/zstd_decode_model.cpp, one "lane") for the tests that
compare it with libzstd: built on demand next to its source, decoded into a destination with guard bytes behind it."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load(flag=""):
    src = os.path.join(HERE, "model", "zstd_decode_model.cpp")
    so = os.path.join(HERE, "model", "zstd_decode_model%s.so" % ("_" + flag[3:].lower() if flag else ""))
    core = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", "zstd_decode_core.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(core)) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", *([flag] if flag else []),
                        src, "-o", so], check=True)
    m = ctypes.CDLL(so)
    i64p = ctypes.POINTER(ctypes.c_int64)
    m.zs_decoded_size.argtypes = [ctypes.c_void_p, ctypes.c_int64, i64p]
    m.zs_decode.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, i64p]
    return m


def decode(model, comp, cap):
    """(0, decoded bytes) or (negative status, None); asserts that nothing was written behind `cap` and that the size pass
    and the decode pass agree."""
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    total = ctypes.c_int64(-1)
    rc = model.zs_decoded_size(comp.ctypes.data, comp.size, ctypes.byref(total))
    if rc != 0:
        return rc, None
    size = total.value
    guard = 64
    out = np.full(max(cap, 0) + guard, 0xA5, dtype=np.uint8)
    rc = model.zs_decode(comp.ctypes.data, comp.size, out.ctypes.data, cap, ctypes.byref(total))
    assert np.all(out[cap:] == 0xA5), "decoder wrote past its destination"
    if rc != 0:
        return rc, None
    assert total.value == size, "size pass and decode pass disagree"
    return 0, out[:size].copy()


def corpora():
    """(name, data) of the sources tests/test_zstd_model.py has libzstd compress."""
    import corpus
    from s3shuffle import datagen

    rng = np.random.default_rng(7)
    yield "terasort", datagen.terasort_map_output(700_000, 1, seed=2)[0]
    yield "wide", datagen.tpcds_wide_map_output(500_000, 1, seed=3)[0]
    yield "kvint", datagen.kv_int_map_output(120_000, 1, seed=1)[0]
    yield "zeros", np.zeros(300_000, np.uint8)
    yield "random", rng.integers(0, 256, 200_000, dtype=np.uint8)
    for k in range(corpus.N_KINDS):
        yield "corpus%d" % k, corpus.chunk_corpus(k, 6000 if k == 6 else 90_000, rng)
    for n in (0, 1, 2, 3, 7, 63, 64, 255, 256, 257, 1000, 4095):
        yield "tiny%d" % n, rng.integers(0, 4, n, dtype=np.uint8)
