"""The lock-step CPU model of the byU32 batch (tests/model/lz4_wave_model_u32.cpp — what lz4_compress_u32_kernel runs on one
wavefront: u32 table, 5-byte hash, distance test) must be byte-identical with liblz4 under every same-address LDS store order
the hardware might choose.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lz4_u32_ref as R
from test_lz4_u32_ref import inputs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "model", "lz4_wave_model_u32.cpp")
SO = os.path.join(HERE, "model", "liblz4_wave_model_u32.so")


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(SRC):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", SO, SRC], check=True)
    L = ctypes.CDLL(SO)
    L.lz4_wave_model_u32_compress.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64,
                                              ctypes.c_void_p]
    return L


def _run(model, d, mode, seed, stats=None):
    out = np.empty(d.size + 64, np.uint8)
    n = model.lz4_wave_model_u32_compress(d.ctypes.data, d.size, out.ctypes.data, mode, seed, stats.ctypes.data if stats is not None else None)
    return None if n < 0 else out[:n].tobytes()


def test_u32_model_matches_liblz4_under_every_store_order(model):
    b0, b1 = R.boundary_pair()
    cases = inputs() + [("boundary_65535", b0), ("boundary_65536", b1)]
    raw = compressed = with_refusals = 0
    for name, d in cases:
        want = R.liblz4_block(d)
        _, refused = R.compress_u32(d.tobytes())
        for mode, seeds in ((0, (1,)), (1, (1,)), (2, (d.size, 77))):
            for seed in seeds:
                stats = np.zeros(8, np.int64)
                got = _run(model, d, mode, seed, stats)
                if got is None:  # would not fit in len bytes: the frame layer stores RAW
                    assert len(want) >= d.size, (name, d.size, mode)
                    continue
                assert got == want, (name, d.size, mode, seed)
                assert stats[3] == refused, (name, d.size, mode)  # the batch refuses exactly what the sequential parse refuses
        raw += len(want) >= d.size
        compressed += len(want) < d.size
        with_refusals += refused > 0
    assert raw >= 1 and compressed >= 1 and with_refusals >= 4
