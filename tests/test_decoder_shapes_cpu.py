"""CPU: what makes the spec-level corpus of tests/decoder_shapes.py trustworthy before tests/test_gpu_decoder_shapes.py holds
it against the hardware.  Every case is valid by the word of independent decoders (the plain Python decoders of
tests/framing.py, liblz4, pyarrow's Snappy when it imports, the oracle's reduce side on the framed streams), every class label
has a case, the kernel's two window constants are bracketed by the distances, the lock-step model decodes every LZ4 / Snappy
block of up to 32 KiB at three output alignments, and the COMPILED kernels decode the smallest case of every label in the ISA
interpreter."""
import os
import re
import shutil
import sys
import time

import numpy as np
import pytest

import decoder_shapes as ds
import framing
from test_batch_decode_model import model, run  # noqa: F401  (the model library's fixture and its guarded call)

HERE = os.path.dirname(os.path.abspath(__file__))
KERNEL = os.path.join(os.path.dirname(HERE), "spark-s3-shuffle_amd", "csrc", "lz4_decode_batch.hip")
LZ4, SNAPPY, LZF = ds.LZ4, ds.SNAPPY, ds.LZF
NAMES = {LZ4: "lz4", SNAPPY: "snappy", LZF: "lzf"}
CODECS = pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
DECODE_PY = {LZ4: framing.lz4_decode_py, SNAPPY: framing.snappy_decode_py, LZF: framing.lzf_decode_py}


@CODECS
def test_every_case_is_valid_by_the_independent_decoders(oracle, codec):
    cases = ds.cases(codec)
    assert len({c.name for c in cases}) == len(cases)
    assert sum(len(c.expected) for c in cases) < 8 << 20
    L = framing.liblz4() if codec == LZ4 else None
    sn = None
    if codec == SNAPPY:
        try:
            import pyarrow as pa

            sn = pa.Codec("snappy")
        except ImportError:  # the oracle alone arbitrates
            sn = None
    for c in cases:
        assert c.codec == codec and c.expected == b"".join(u[2] for u in c.units), c.name
        for stored, payload, expected in c.units:
            if stored:
                assert payload == expected, c.name
                continue
            assert DECODE_PY[codec](payload) == expected, c.name
            if codec == LZ4:
                src = np.frombuffer(payload, np.uint8)
                out = np.empty(len(expected) + 1, np.uint8)
                n = L.LZ4_decompress_safe(src.ctypes.data, out.ctypes.data, src.size, len(expected))
                assert n == len(expected) and out[:n].tobytes() == expected, (c.name, n)
            if sn is not None:
                got = sn.decompress(payload, decompressed_size=len(expected)).to_pybytes() if expected else b""
                assert got == expected, c.name
    # the framed streams through the oracle's reduce side (LZF: pinned against liblzf 3.6), the whole corpus as one range
    img, index, offs = ds.pack_range(cases)
    rc, out, bad = oracle.decompress_range(codec, 0, img, index, None, int(offs[-1]) + 64)
    assert rc == 0, (rc, cases[bad].name if 0 <= bad < len(cases) else bad)
    assert out.size == offs[-1]
    assert ds.first_difference(cases, offs, out.tobytes(), "oracle") is None, ds.first_difference(cases, offs, out.tobytes(), "oracle")


def test_lzf_writer_and_decoder_against_the_format():
    """the three element shapes byte by byte, as the kernel's comment states the format"""
    assert framing.lzf_block([("lit", b"abc")]) == b"\x02abc"
    assert framing.lzf_block([("ref", 1, 3)]) == bytes([1 << 5, 0])                    # (ctrl >> 5) + 2 = 3, distance 0 + 1
    assert framing.lzf_block([("ref", 8192, 8)]) == bytes([(6 << 5) | 31, 255])        # the longest short form, the farthest
    assert framing.lzf_block([("ref", 257, 9)]) == bytes([(7 << 5) | 1, 0, 0])         # 7 + 0 + 2
    assert framing.lzf_block([("ref", 300, 264)]) == bytes([(7 << 5) | 1, 255, 43])    # 7 + 255 + 2
    assert framing.lzf_decode_py(b"\x02abc" + bytes([1 << 5, 2])) == b"abcabc"
    assert framing.lzf_decode_py(b"\x00a" + bytes([7 << 5, 0, 0])) == b"a" * 10
    for bad in (b"\x02ab", bytes([1 << 5, 0]), b"\x00a" + bytes([1 << 5, 1]), b"\x00a" + bytes([7 << 5, 0]), b"\x00a" + bytes([1 << 5])):
        assert framing.lzf_decode_py(bad) is None, bad
    assert framing.lzf_chunk(b"xy", 9) == b"ZV\x01\x00\x02\x00\x09xy"
    assert framing.lzf_chunk(b"xy", 2, stored=True) == b"ZV\x00\x00\x02xy"


@CODECS
def test_every_class_label_has_a_case(codec):
    labels = ds.LABELS[codec]
    assert len(set(labels)) == len(labels)
    covered = set()
    for c in ds.cases(codec):
        assert c.classes and c.classes <= set(labels), (c.name, sorted(c.classes - set(labels)))
        covered |= c.classes
    assert not set(labels) - covered, sorted(set(labels) - covered)
    # every case of the subset covers what it was chosen for, and the subset covers every label
    assert set().union(*(c.classes for c in ds.smallest_per_label(codec))) == set(labels)


def test_a_wrong_byte_is_reported_with_its_case_and_position():
    cases = ds.cases(LZF)
    img, index, offs = ds.pack_range(cases)
    good = b"".join(c.expected for c in cases)
    assert ds.first_difference(cases, offs, good) is None
    k = len(cases) // 2
    at = int(offs[k]) + 5
    bad = bytearray(good)
    bad[at] ^= 1
    msg = ds.first_difference(cases, offs, bytes(bad), "leg")
    assert msg.startswith("leg: case %s (partition %d" % (cases[k].name, k)) and "first at byte 5:" in msg
    assert cases[0].name in ds.first_difference(cases, offs, good[1:] + b"x")


def test_the_sweeps_bracket_the_kernels_window_constants():
    """S3S_BWIN / S3S_BHIST read from the kernel's TEXT (not imported): a retune of the window fails here"""
    text = open(KERNEL).read()
    win = [int(v) for v in re.findall(r"^#define\s+S3S_BWIN\s+(\d+)", text, re.M)]
    hist = [int(v) for v in re.findall(r"^#define\s+S3S_BHIST\s+(\d+)", text, re.M)]
    assert win == [ds.WINDOW] and hist == [ds.HISTORY], (win, hist)
    for codec in (LZ4, SNAPPY, LZF):
        ds.cases(codec)
        for v in (win[0], hist[0]):
            for d in (v - 1, v, v + 1):
                assert d in ds.DISTANCES[codec], (NAMES[codec], d)
        assert max(ds.DISTANCES[codec]) == {LZ4: 65535, SNAPPY: 70000, LZF: 8192}[codec]
    # the far-source runs follow one another without a gap a flush could hide in
    for c in ds.cases(LZ4):
        if c.name.endswith((".run", ".run255")):
            assert len(c.expected) - int(c.name.split(".")[2][1:]) >= 300 * 4


@pytest.mark.parametrize("codec", [LZ4, SNAPPY], ids=["lz4", "snappy"])
def test_lock_step_model_decodes_every_block_up_to_32k(model, codec):  # noqa: F811
    n = 0
    for c in ds.cases(codec):
        for stored, payload, expected in c.units:
            if stored or len(expected) > 32768:
                continue
            for mis in (0, 7, 15):
                rc, got = run(model, 0 if codec == LZ4 else 1, payload, len(expected), mis)
                assert rc == 0, (c.name, mis, rc)
                if got.tobytes() != expected:
                    at = int(np.argmax(got != np.frombuffer(expected, np.uint8)))
                    pytest.fail("%s at alignment %d: first difference at byte %d" % (c.name, mis, at))
            n += 1
    assert n >= 90  # (most of the corpus: only the far distances and the large-block shapes are above 32 KiB)


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="hipcc not available")
@CODECS
def test_compiled_kernels_decode_the_smallest_case_of_every_label(codec):
    """the batch decoder's three front ends in the ISA interpreter: payload and destination of exactly their sizes"""
    sys.path.insert(0, os.path.join(HERE, "isa"))
    import decode_kernel as dk

    subset = ds.smallest_per_label(codec)
    fmt = {LZ4: 0, SNAPPY: 1, LZF: 2}[codec]
    comp = {LZ4: 0x20, SNAPPY: 1, LZF: 2}[codec]
    blocks, methods, owners = [], [], []
    for c in subset:
        for stored, payload, expected in c.units:
            blocks.append((payload, len(expected)))
            methods.append(0x10 if stored else comp)
            owners.append((c.name, expected))
    t0 = time.time()
    res, st, _ = dk.decode_blocks(blocks, fmt=fmt, methods=methods)
    print("interpreter subset %s: %d cases, %d blocks, %d decoded bytes, %.1f s" % (
        NAMES[codec], len(subset), len(blocks), sum(b[1] for b in blocks), time.time() - t0))
    assert st == 0
    for got, (name, expected) in zip(res, owners):
        if got != expected:
            at = next(i for i, (a, b) in enumerate(zip(got, expected)) if a != b)
            pytest.fail("%s: first difference at byte %d" % (name, at))
