"""The compiled LZ4 compress kernels with extra build flags on the CPU interpreter (TEST INFRASTRUCTURE ONLY, no GPU):
the input-ring kernel (lz4_compress_ring_kernel, variant 11, 20 KiB of LDS) and the variant-10 kernel
(lz4_compress_l2_kernel, 16 KiB), both built from lz4_window_engine.inc.  tests/test_isa_lz4_chain.py and
tests/tools/chain_profile.py share it; the launch is the one of tests/test_isa_lz4_ring.py with `flags`, `lds_order` and
`hooks` passed on."""
import hashlib
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402

RING_LDS_BYTES = 16384 + 4096
K_SLOT_HEADER, K_FRAME_HEADER, RAW_FLAG = 32, 21, 0x80000000
_PROGS = {}


def ring_program(flags=()):
    """(Program, entry, assembly text) of the ring kernel built with `flags`"""
    key = tuple(flags)
    if key not in _PROGS:
        stamp = hashlib.sha1(open(os.path.join(lk.CSRC, "lz4_compress.hip"), "rb").read()).hexdigest()[:12]
        text = lk.compile_asm(src="lz4_compress_ring.hip", flags=("-DS3S_RING_SOURCE_STAMP=0x" + stamp,) + key)
        entry = lk.find_kernel(text, "lz4_compress_ring_kernelILb1E")
        _PROGS[key] = (emu.Program(text, entry), entry, text)
    return _PROGS[key]


def compress_chunks(chunks, ring=True, flags=(), profile=None, lds_order=None, hooks=None, tail_guard=0, block=32768):
    """(payload or None when stored RAW, the 21 header bytes, wave) per chunk.  The source buffer ends at the last chunk's
    last byte (+ tail_guard): a read past it, or an LDS access past the kernel's allocation, faults in the interpreter."""
    if not ring:
        return lk.compress_chunks(chunks, flags=tuple(flags), profile=profile, lds_order=lds_order, hooks=hooks,
                                  tail_guard=tail_guard, block=block)
    prog, entry, _ = ring_program(flags)
    mem = emu.Memory(None)
    src = np.concatenate([np.asarray(c, dtype=np.uint8) for c in chunks] + [np.zeros(tail_guard, np.uint8)])
    n = len(chunks)
    stride = K_SLOT_HEADER + ((block + 15) & ~15)
    items, off = bytearray(), 0
    for k, c in enumerate(chunks):
        items += struct.pack("<qiiii", off, len(c), 0 | ((5 if block == 32768 else 6) << 8), k, 0)
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
        waves += emu.launch(prog, entry, mem, kernarg, 1, RING_LDS_BYTES, profile=profile, lds_order=lds_order, hooks=hooks)
        assert work[0] == 2
    out = []
    for k in range(n):
        sz = int(sizes[k])
        slot = slots[k * stride:(k + 1) * stride]
        plen = (sz & 0x7FFFFFFF) - K_FRAME_HEADER
        out.append((None if sz & RAW_FLAG else slot[K_SLOT_HEADER:K_SLOT_HEADER + plen].copy(),
                    bytes(slot[K_SLOT_HEADER - K_FRAME_HEADER:K_SLOT_HEADER]), waves[k]))
    return out
