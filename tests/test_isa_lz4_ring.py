"""The COMPILED input-ring kernel (lz4_compress_ring_kernel, S3S_OPT_LZ4_VARIANT 11: hipcc -S output of lz4_compress_ring.hip)
executed on the CPU by tests/isa/gfx950_emu.py with its 20 KiB of LDS, byte for byte against oracle.compress_map_output, on
inputs that put matches on the ring's edges (tests/lz4_ring_cases.py); plus the wait-state check of its asm block.
Needs hipcc (cross-compiles without a GPU) but no device."""
import hashlib
import os
import shutil
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))
sys.path.insert(0, HERE)
import lz4_ring_cases as cases  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None,
                                reason="hipcc not available")

LDS_BYTES = 16384 + 4096
K_SLOT_HEADER, K_FRAME_HEADER, RAW_FLAG = 32, 21, 0x80000000
LZ4, CRC = 1, 2
_PROG = []


def _program():
    """(Program, entry, assembly text) of the ring kernel; lz4_compress.hip is what lz4_compress_ring.hip includes, so its
    hash goes into the cache key of the assembly (as a macro nothing reads)"""
    if not _PROG:
        import gfx950_emu as emu
        import lz4_kernel as lk

        stamp = hashlib.sha1(open(os.path.join(lk.CSRC, "lz4_compress.hip"), "rb").read()).hexdigest()[:12]
        text = lk.compile_asm(src="lz4_compress_ring.hip", flags=("-DS3S_RING_SOURCE_STAMP=0x" + stamp,))
        entry = lk.find_kernel(text, "lz4_compress_ring_kernelILb1E")
        _PROG.append((emu.Program(text, entry), entry, text))
    return _PROG[0]


def compress_chunks(chunks, profile=None, tail_guard=0, block=32768):
    """lz4_kernel.compress_chunks for the ring kernel: one one-item launch per chunk with LDS_BYTES of LDS.  The source
    buffer ends exactly at the last chunk's last byte (+ tail_guard): a read past it faults in the interpreter, and so does
    an LDS access past LDS_BYTES.  Returns (payload or None when stored RAW, the 21 header bytes, wave) per chunk."""
    import gfx950_emu as emu

    prog, entry, _ = _program()
    mem = emu.Memory(None)
    src = np.concatenate([np.asarray(c, dtype=np.uint8) for c in chunks] + [np.zeros(tail_guard, np.uint8)])
    n = len(chunks)
    stride = K_SLOT_HEADER + ((block + 15) & ~15)
    items, off = bytearray(), 0
    for k, c in enumerate(chunks):
        items += struct.pack("<qiiii", off, len(c), 0 | ((5 if block == 32768 else 6) << 8), k, 0)  # (kind | the token's level nibble << 8)
        off += len(c)
    slots = np.zeros(n * stride, dtype=np.uint8)
    sizes = np.zeros(n, dtype=np.uint32)
    checks = np.arange(n, dtype=np.uint32) * np.uint32(0x01010101)
    work = np.zeros(16, dtype=np.uint32)
    a_src = mem.map(src, "src", writable=False)
    a_items = mem.map(np.frombuffer(items, dtype=np.uint8), "items", writable=False)
    a_check = mem.map(checks, "item_check", writable=False)
    a_slots = mem.map(slots, "slots")
    a_sizes = mem.map(sizes, "item_size")
    a_work = mem.map(work, "work")
    waves = []
    for k in range(n):
        work[:] = 0
        kernarg = struct.pack("<QQiiQQQQ", a_src, a_items + 24 * k, 1, stride, a_check + 4 * k, a_slots, a_sizes + 4 * k, a_work)
        waves += emu.launch(prog, entry, mem, kernarg, 1, LDS_BYTES, profile=profile)
        assert work[0] == 2
    out = []
    for k in range(n):
        sz = int(sizes[k])
        slot = slots[k * stride:(k + 1) * stride]
        plen = (sz & 0x7FFFFFFF) - K_FRAME_HEADER
        out.append((None if sz & RAW_FLAG else slot[K_SLOT_HEADER:K_SLOT_HEADER + plen].copy(),
                    bytes(slot[K_SLOT_HEADER - K_FRAME_HEADER:K_SLOT_HEADER]), waves[k]))
    return out


def _check(chunks, oracle, **kw):
    """every chunk as a one-partition map output: the kernel's block (header without the xxHash32 the kernel is handed, and
    payload) against the first frame of oracle.compress_map_output's stream"""
    block = 65536 if max(len(c) for c in chunks) > 32768 else 32768
    res = compress_chunks(chunks, block=block, **kw)
    for c, (payload, hdr, w) in zip(chunks, res):
        img, index, _ = oracle.compress_map_output(LZ4, CRC, c, np.array([0, len(c)], dtype=np.int64), block)
        img = bytes(np.asarray(img, dtype=np.uint8))
        assert img[:8] == b"LZ4Block" and hdr[:8] == b"LZ4Block"
        clen, olen = struct.unpack("<ii", img[9:17])
        assert olen == len(c) and len(img) == 21 + clen + 21
        assert hdr[8:17] == img[8:17], "token / lengths differ (len %d)" % len(c)
        if payload is None:
            assert clen == len(c), "kernel stored RAW a chunk the reference compresses"
        else:
            assert bytes(payload) == img[21:21 + clen], "ring kernel differs from the oracle (len %d)" % len(c)
    return res


def _visits(profile, label):
    """instructions executed behind the labels of the three window bodies that start with `label`"""
    return sum(v[0] for k, v in profile.items() if k.startswith(".Lw_" + label))


def test_span_edge(oracle):
    chunks = cases.span_edge()
    for c, inside in zip(chunks, (True, False, False)):
        prof = {}
        _check([c], oracle, profile=prof)
        assert _visits(prof, "fwonlyr") + _visits(prof, "extbr") > 0, "near sources are served from the ring"
        if not inside:  # offsets SPAN and SPAN + 1 take the global loads
            assert _visits(prof, "extg") > 0


def test_wrap(oracle):
    prof = {}
    _check(cases.wrap(), oracle, profile=prof)
    assert _visits(prof, "fwonlyr") > 0


def test_coverage_edge(oracle):
    _check(cases.coverage_edge(), oracle)


def test_hand_back_and_re_entry(oracle):
    prof = {}
    _check(cases.hand_back(), oracle, profile=prof)
    assert _visits(prof, "dispf") > 3 * 15, "the block was left and entered again (each entry refills the ring)"


def test_short_history(oracle):
    _check(cases.short_history(), oracle)


def test_lengths(oracle):
    res = _check(cases.lengths(), oracle)
    assert res[0][2].n_lds < res[1][2].n_lds


def test_end_of_allocation(oracle):
    _check(cases.end_of_allocation(), oracle, tail_guard=0)


def test_generated_data(oracle):
    prof = {}
    _check(cases.generated(), oracle, profile=prof)
    assert _visits(prof, "fwonlyr") > 0 and _visits(prof, "exth") > 0


def test_ring_block_keeps_its_wait_states():
    import hazards

    _, entry, text = _program()
    asm_viol, cc_viol, _, _ = hazards.check_kernel(text, entry)
    assert not asm_viol, asm_viol[:5]
    assert not cc_viol, ("rule set stricter than the compiler", cc_viol[:3])
