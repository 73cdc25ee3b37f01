"""Runs the compiled kernels of a resumable Zstandard stream (zstd_decode_stream.hip + zstd_stream_core.h: `zstd_walk_kernel`,
the unit walk, and `zstd_stream_kernel`, the resumable frame decoder in its size and execute modes) on the CPU through
tests/isa/gfx950_emu.py (TEST INFRASTRUCTURE), feed by feed the way s3s_dstream_feed_device drives them.  The window buffer of
a feed ends exactly at comp_len, dst has exactly out_len bytes, the staging area exactly history + the resumed frame's output,
the state record and the history exactly their sizes: an access outside any of them faults in the interpreter."""
import os
import re
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402

STATE_BYTES = 9864  # sizeof(s3s_zstd::ZStreamState)
UNIT = struct.Struct("<qiiii")  # ZUnit: off, kind, payload, frame_unit, pad
FRAME, SKIP, RAW, LAST = 0, 1, 2, 0x10
_PROGS = None


def programs():
    global _PROGS
    if _PROGS is None:
        text = lk.compile_asm("zstd_decode_stream.hip")
        walk, run = lk.find_kernel(text, "zstd_walk_kernel"), lk.find_kernel(text, "zstd_stream_kernel")
        lds = max(int(line.split()[-1]) for line in text.splitlines() if ".amdhsa_group_segment_fixed_size" in line)
        callees = [m.group(1) for m in re.finditer(r'^\s*\.type\s+(_ZN8s3s_zstd\w+),@function', text, re.M)]
        _PROGS = (emu.Program(text, walk), walk, emu.Program(text, run, callees=callees), run, text, lds)
    return _PROGS


class Stream:
    """The host side of s3s_dstream_feed_device for one partition, with the two kernels in the interpreter."""

    def __init__(self, part, wlog):
        self.part, self.wlog = bytes(part), wlog
        self.pos, self.open, self.state, self.hist, self.window, self.produced = 0, False, None, b"", 0, 0

    def feed(self, wend):
        """The window part[pos, wend) -> (status, consumed, need_comp, decoded bytes)"""
        p_walk, e_walk, p_run, e_run, text, lds = programs()
        objs = dict(emu.parse_objects(text))
        mem = emu.Memory()
        win = np.frombuffer(self.part[self.pos:wend], np.uint8).copy()
        a_win = mem.map(win if win.size else np.zeros(1, np.uint8), "window", writable=False)
        poff = np.array([0, win.size], np.int64)
        a_poff = mem.map(poff.view(np.uint8), "piece_off", writable=False)
        status, result = np.zeros(4, np.int32), np.zeros(9, np.int64)
        a_status, a_result = mem.map(status.view(np.uint8), "status"), mem.map(result.view(np.uint8), "result")
        cnt = np.zeros(1, np.uint32)
        a_cnt = mem.map(cnt.view(np.uint8), "piece_units")
        pend = len(self.part) - self.pos

        def walk(emit, a_base, a_units, a_dsize):
            karg = struct.pack("<QQiiqqi4xQQQQQQ", a_win, a_poff, 1, 1 if self.open else 0, pend, 1 << self.wlog, emit, a_base, a_cnt, a_units,
                               a_dsize, a_status, a_result)
            emu.launch(p_walk, e_walk, mem, karg, 1, 0, objects=objs)

        walk(0, 0, 0, 0)
        if status[0]:
            return int(status[0]), 0, 0, b""
        n, stop, need = int(cnt[0]), int(result[0]), int(result[1])
        if n == 0:
            return 0, 0, need, b""
        units, dsize = np.zeros(n * UNIT.size, np.uint8), np.zeros(n, np.uint32)
        base = np.array([0, n], np.int64)
        a_units, a_dsize, a_base = mem.map(units, "units"), mem.map(dsize.view(np.uint8), "dsize"), mem.map(base.view(np.uint8), "unit_base", writable=False)
        walk(1, a_base, a_units, a_dsize)
        ulist = [UNIT.unpack_from(units, k * UNIT.size) for k in range(n)]
        a_st_in = mem.map(np.frombuffer(self.state, np.uint8).copy(), "state_in", writable=False) if self.open else 0

        def run(execute, a_out, a_st_out, a_dst, a_staging, a_lit):
            karg = struct.pack("<QQQQQqiiQQQQqQqQQ", a_win, a_units, a_dsize, a_out, a_base, n, execute, 1 if self.open else 0, a_st_in, a_st_out,
                               a_dst, a_staging, len(self.hist), a_lit, 0, a_status, a_result + 64)
            emu.launch(p_run, e_run, mem, karg, 1, lds, objects=objs)

        run(0, 0, 0, 0, 0, 0)  # the size pass
        if status[0]:
            return int(status[0]), 0, 0, b""
        unit_out = np.concatenate([[0], np.cumsum(dsize.astype(np.int64))])
        out_len = int(unit_out[n])
        last = ulist[-1]
        open_after = (last[1] & 15) == FRAME or ((last[1] & 15) >= RAW and not last[1] & LAST)
        fu = last[3] if open_after else -1
        resumed_n = 0
        while self.open and resumed_n < n and (ulist[resumed_n][1] & 15) >= RAW and ulist[resumed_n][3] == -1:
            resumed_n += 1
        resumed_out = int(unit_out[resumed_n])
        dst = np.zeros(max(out_len, 1), np.uint8)[:out_len]
        staging = np.concatenate([np.frombuffer(self.hist, np.uint8), np.zeros(resumed_out, np.uint8)]) if self.open else np.zeros(0, np.uint8)
        state_out, lit = np.zeros(STATE_BYTES, np.uint8), np.zeros((128 << 10) + 64, np.uint8)
        a_dst = mem.map(dst, "dst") if out_len else 0
        a_staging = mem.map(staging, "staging") if staging.size else 0
        a_out = mem.map(unit_out.view(np.uint8), "unit_out", writable=False)
        run(1, a_out, mem.map(state_out, "state_out") if open_after else 0, a_dst, a_staging, mem.map(lit, "lit"))
        if status[0]:
            return int(status[0]), 0, 0, b""
        assert int(result[8]) == resumed_out
        if resumed_out:
            dst[:resumed_out] = staging[len(self.hist):]
        if open_after and fu < 0:
            self.produced += out_len
            self.hist = bytes(staging[staging.size - min(self.window, self.produced):])
        elif open_after:
            hdr = self.part[self.pos + ulist[fu][0]:][:ulist[fu][2]]
            wd = hdr[5]
            self.window = (1 << (10 + (wd >> 3))) + ((1 << (10 + (wd >> 3))) >> 3) * (wd & 7)  # (frames with a window descriptor)
            self.produced = out_len - int(unit_out[fu])
            self.hist = bytes(dst[out_len - min(self.window, self.produced):])
        else:
            self.hist, self.window, self.produced = b"", 0, 0
        self.open, self.state = open_after, bytes(state_out) if open_after else None
        self.pos += stop
        return 0, stop, 0, bytes(dst)
