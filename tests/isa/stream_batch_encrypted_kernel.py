"""Runs the compiled decrypt pass of the batched feed under IO encryption - aes_ctr_window_batch_kernel<NR>
(csrc/aes_ctr_stream_batch.hip; the tile body is csrc/aes_ctr_window_tile.inc) - on the CPU through tests/isa/gfx950_emu.py
(TEST INFRASTRUCTURE), several windows per launch, from the descriptors and the tile -> window map the host code builds
(batch_layout, csrc/decode_stream.hip).

Every stored window lives in a buffer of exactly its L bytes, every plain destination has exactly PL bytes, every IV area
16 x m, and the offset tables m + 1 entries: a load or a store outside them - also one that would land in a neighbour's buffer
of a packed allocation - is a fault of the interpreter's memory.  The destinations are prefilled, so a byte that was not written
shows, and the interpreter's memory counts the stores per byte."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402

SRC = "aes_ctr_stream_batch.hip"
TILE_CHUNKS = 1024  # kWinTileChunks: 256 threads x 4 chunks of 16 stored bytes
DESC_FMT = "<QQQQQiiqq4I"  # AesWindow (csrc/s3s_internal.h)
DESC_BYTES = struct.calcsize(DESC_FMT)
assert DESC_BYTES == 80
PREFILL = 0xA5
_PROG = {}


class CountingMemory(emu.Memory):
    """the interpreter's memory, counting the stores per byte of every writable region"""

    def __init__(self):
        super().__init__(None)
        self.writes = {}

    def map(self, data, name, writable=True, **kw):
        base = super().map(data, name, writable, **kw)
        if writable:
            self.writes[name] = np.zeros(self.regions[-1][1].size, np.int32)
        return base

    def store(self, addrs, active, data):
        n = data.shape[1]
        for lane in np.flatnonzero(active):
            base, arr, name, _ = self.find(int(addrs[lane]))
            o = int(addrs[lane]) - base
            if name in self.writes and o + n <= arr.size:  # (a store outside a region: super().store raises the fault)
                self.writes[name][o:o + n] += 1
        super().store(addrs, active, data)


def tiles_of(m: int, front: int, L: int) -> int:
    """aes_ctr_window_tiles: a window without a plain piece or a stored byte owns no tile"""
    if m <= 0 or L <= 0:
        return 0
    chunks = (L + (front & 15) + 15) >> 4
    return (chunks + TILE_CHUNKS - 1) // TILE_CHUNKS


def _program(rounds):
    if "text" not in _PROG:
        text = lk.compile_asm(SRC)
        _PROG["text"] = (text, emu.parse_objects(text))
    text, objs = _PROG["text"]
    if rounds not in _PROG:
        entry = lk.find_kernel(text, "aes_ctr_window_batch_kernelILi%dE" % rounds)
        _PROG[rounds] = (emu.Program(text, entry), entry)
    return _PROG[rounds] + (objs,)


def decrypt_batch(round_keys, rounds, wins, extra_tiles=0):
    """round_keys: 4 x (rounds + 1) uint32 (aes_ctr_core.h's expand_key); wins: one dict per window - stored (the window's L bytes),
    E, Q (m + 1 offsets), front, iv0 (16 bytes, the carried IV; read when front > 0).  extra_tiles: workgroups launched beyond
    the map's end (total_tiles stays what it is: they must leave at once).
    -> (one dict per window: plain (PL bytes), ivs ([m, 16]), plain_writes / iv_writes (stores per byte), tiles, tile0; the
    tile -> window map)"""
    mem = CountingMemory()
    desc = np.zeros(DESC_BYTES * len(wins), np.uint8)
    out, tile_win, tile0 = [], [], 0
    for i, w in enumerate(wins):
        E, Q = np.asarray(w["E"], np.int64), np.asarray(w["Q"], np.int64)
        m = E.size - 1
        assert Q.size == E.size and E[0] == 0 and Q[0] == 0
        stored = np.ascontiguousarray(w["stored"], dtype=np.uint8)
        L, PL = int(E[m]), int(Q[m])
        assert stored.size == L
        plain = np.full(max(PL, 1), PREFILL, np.uint8)[:PL]
        ivs = np.full(max(16 * m, 1), PREFILL, np.uint8)[:16 * m]
        a_in = mem.map(stored.copy(), "stored%d" % i, writable=False) if L else 0
        a_out = mem.map(plain, "plain%d" % i) if PL else 0
        a_iv = mem.map(ivs, "ivs%d" % i) if m else 0
        a_E, a_Q = mem.map(E, "E%d" % i, writable=False), mem.map(Q, "Q%d" % i, writable=False)
        t = tiles_of(m, int(w["front"]), L)
        iv0 = bytes(w.get("iv0") or bytes(16))
        struct.pack_into(DESC_FMT, desc, DESC_BYTES * i, a_in, a_out, a_E, a_Q, a_iv, m, tile0, int(w["front"]), L, *struct.unpack(">4I", iv0))
        tile_win += [i] * t
        out.append(dict(plain=plain, ivs=ivs.reshape(m, 16), tiles=t, tile0=tile0, plain_writes=mem.writes.get("plain%d" % i, np.zeros(0, np.int32)),
                        iv_writes=mem.writes.get("ivs%d" % i, np.zeros(0, np.int32)).reshape(m, 16)))
        tile0 += t
    total = len(tile_win)
    if total == 0:
        return out, tile_win
    a_desc = mem.map(desc, "windows", writable=False)
    a_map = mem.map(np.asarray(tile_win, np.int32), "tile_win", writable=False)
    rk = np.zeros(60, np.uint32)
    rk[:4 * (rounds + 1)] = np.asarray(round_keys, np.uint32)[:4 * (rounds + 1)]
    prog, entry, objs = _program(rounds)
    emu.launch(prog, entry, mem, rk.tobytes() + struct.pack("<QQi", a_desc, a_map, total), total + extra_tiles, 0, block_x=256, objects=objs)
    return out, tile_win
