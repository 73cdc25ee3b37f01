"""Runs the compiled stream-mode kernels of the reduce side (s3s_dstream_feed*, csrc/decode_stream.hip) on the CPU through
tests/isa/gfx950_emu.py (TEST INFRASTRUCTURE), in the order a feed launches them:

  LZ4     tile_speculate_kernel -> tile_resolve_stream_kernel -> scan_u32_kernel | host: n_frames, stop -> tile_emit_kernel
          (comp_len = stop) -> scan_u32_kernel -> frames_cut_kernel
  Snappy  snappy_count_stream_kernel -> scan_u32_kernel | host -> snappy_emit_stream_kernel -> scan_u32_kernel ->
  / LZF   frames_cut_kernel
  seeds   checksum_seed_kernel<ALGO>

The stream kernels are csrc/decode_stream_kernels.hip; speculation, emit and scan are the one-shot kernels of
csrc/lz4_decompress.hip.

The window's buffer ends with the window's last byte and every array has exactly the size the host code gives it, so a
header parse that looks at or beyond comp_len is a fault of the interpreter's memory."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402
import checksum_kernel as ck  # noqa: E402

TILE = 65536
STREAM, ONE_SHOT = "decode_stream_kernels.hip", "lz4_decompress.hip"
LZ4, SNAPPY, LZF = 1, 2, 4
_PROG = {}


def _text(src):
    if src not in _PROG:
        text = lk.compile_asm(src)
        _PROG[src] = (text, {k: v for k, v in emu.parse_objects(text).items() if k.startswith("_ZN3s3s")})
    return _PROG[src]


def _launch(src, needle, mem, kernarg, grid, block_x=64, implicit=False):
    text, objs = _text(src)
    if implicit:  # kernels that read blockDim.x: the implicit arguments follow the explicit ones (code object v5)
        kernarg += b"\0" * (-len(kernarg) % 8) + struct.pack("<IIIHHHHHH", grid, 1, 1, block_x, 1, 1, 0, 0, 0) + bytes(200)
    key = (src, needle)
    if key not in _PROG:
        entry = lk.find_kernel(text, needle)
        _PROG[key] = (emu.Program(text, entry), entry)
    prog, entry = _PROG[key]
    emu.launch(prog, entry, mem, kernarg, grid, 0, block_x=block_x, objects=objs)


def _cut(mem, codec, a_fr, a_or, a_fo, n_frames, dst_capacity, stop):
    result = np.full(4, -7, np.int64)
    a_res = mem.map(result, "cut_result")
    _launch(STREAM, "frames_cut_kernel", mem,
            struct.pack("<QQQqqqiiQ", a_fr, a_or, a_fo, n_frames, dst_capacity, stop, codec, 0, a_res), (n_frames + 256) // 256, block_x=256)
    return [int(x) for x in result]


def _frames(n_frames):
    frames = np.zeros(max(n_frames, 1) * 24, np.uint8)[: n_frames * 24]
    orig = np.zeros(max(n_frames, 1), np.uint32)[:n_frames]
    fout = np.full(n_frames + 1, -7, np.int64)
    return frames, orig, fout


def feed_lz4(window: bytes, range_left: int, dst_capacity: int):
    """-> dict(status, stop, need, n_frames, frames, k, consumed, out_len, need_dst) for one window of an LZ4Block range"""
    n = len(window)
    n_tiles = (n + TILE - 1) // TILE
    assert n_tiles > 0
    mem = emu.Memory(None)
    a_comp = mem.map(np.frombuffer(bytearray(window), dtype=np.uint8), "comp", writable=False)
    spec_entry, spec_exit = np.full(n_tiles, -7, np.int64), np.full(n_tiles, -7, np.int64)
    spec_count, true_entry = np.full(n_tiles, -7, np.int32), np.full(n_tiles, -7, np.int64)
    frame_base, status, result = np.full(n_tiles + 1, -7, np.int64), np.zeros(1, np.int32), np.full(2, -7, np.int64)
    a_se, a_sx, a_sc = mem.map(spec_entry, "spec_entry"), mem.map(spec_exit, "spec_exit"), mem.map(spec_count, "spec_count")
    a_te, a_fb, a_st, a_res = mem.map(true_entry, "true_entry"), mem.map(frame_base, "frame_base"), mem.map(status, "status"), mem.map(result, "result")
    src = ONE_SHOT
    _launch(src, "tile_speculate_kernel", mem, struct.pack("<QqiiQQQ", a_comp, n, n_tiles, 0, a_se, a_sx, a_sc), n_tiles)
    _launch(STREAM, "tile_resolve_stream_kernel", mem,
            struct.pack("<QqqiiQQQQQQ", a_comp, n, range_left, n_tiles, 0, a_se, a_sx, a_sc, a_te, a_st, a_res), 1)
    if int(status[0]) == 0:
        _launch(src, "scan_u32_kernel", mem, struct.pack("<QqQ", a_sc, n_tiles, a_fb), 1)
    out = dict(status=int(status[0]), stop=int(result[0]), need=int(result[1]), n_frames=0, frames=[], k=0, consumed=0, out_len=0, need_dst=0)
    if out["status"] != 0:
        return out
    n_frames = out["n_frames"] = int(frame_base[n_tiles])
    stop = out["consumed"] = out["stop"]
    if n_frames == 0:
        return out
    frames, orig, fout = _frames(n_frames)
    a_fr, a_or, a_fo = mem.map(frames, "frames"), mem.map(orig, "frame_orig"), mem.map(fout, "frame_out")
    nt = (stop + TILE - 1) // TILE
    _launch(src, "tile_emit_kernel", mem, struct.pack("<QqiiQQQQQ", a_comp, stop, nt, 0, a_te, a_fb, a_fr, a_or, a_st), (nt + 63) // 64)
    _launch(src, "scan_u32_kernel", mem, struct.pack("<QqQ", a_or, n_frames, a_fo), 1)
    out["status"] = int(status[0])
    out["frames"] = [struct.unpack_from("<qiiIi", frames, 24 * k) for k in range(n_frames)]
    out["k"], out["consumed"], out["out_len"], out["need_dst"] = _cut(mem, LZ4, a_fr, a_or, a_fo, n_frames, dst_capacity, stop)
    return out


def feed_chunks(codec: int, window: bytes, piece_off, first_mid: bool, last_pend: int, dst_capacity: int):
    """the same for a window of a Snappy / LZF range: piece_off = the pieces of partitions inside the window (window-relative)"""
    fmt = 1 if codec == LZF else 0
    offs = np.asarray(piece_off, np.int64)
    n = len(offs) - 1
    mem = emu.Memory(None)
    a_comp = mem.map(np.frombuffer(bytearray(window) or bytearray(1), dtype=np.uint8)[: len(window)] if window else np.zeros(1, np.uint8), "comp", writable=False)
    a_off = mem.map(offs, "piece_off", writable=False)
    cnt, base = np.full(n, 0xFFFFFFFF, np.uint32), np.full(n + 1, -7, np.int64)
    status, result = np.zeros(1, np.int32), np.full(2, -7, np.int64)
    a_cnt, a_base, a_st, a_res = mem.map(cnt, "piece_nframes"), mem.map(base, "frame_base"), mem.map(status, "status"), mem.map(result, "result")
    src = STREAM
    _launch(src, "snappy_count_stream_kernel", mem, struct.pack("<QQiiqQQQi", a_comp, a_off, n, int(first_mid), last_pend, a_cnt, a_st, a_res, fmt),
            (n + 63) // 64, implicit=True)
    out = dict(status=int(status[0]), stop=int(result[0]), need=int(result[1]), n_frames=0, frames=[], k=0, consumed=0, out_len=0, need_dst=0)
    if out["status"] != 0:
        return out
    _launch(ONE_SHOT, "scan_u32_kernel", mem, struct.pack("<QqQ", a_cnt, n, a_base), 1)
    n_frames = out["n_frames"] = int(base[n])
    stop = out["consumed"] = out["stop"]
    if n_frames == 0:
        return out
    frames, orig, fout = _frames(n_frames)
    a_fr, a_or, a_fo = mem.map(frames, "frames"), mem.map(orig, "frame_orig"), mem.map(fout, "frame_out")
    _launch(src, "snappy_emit_stream_kernel", mem,
            struct.pack("<QQiiqQQQQi", a_comp, a_off, n, int(first_mid), last_pend, a_base, a_fr, a_or, a_st, fmt), (n + 63) // 64, implicit=True)
    _launch(ONE_SHOT, "scan_u32_kernel", mem, struct.pack("<QqQ", a_or, n_frames, a_fo), 1)
    out["status"] = int(status[0])
    out["frames"] = [struct.unpack_from("<qiiIi", frames, 24 * k) for k in range(n_frames)]
    out["k"], out["consumed"], out["out_len"], out["need_dst"] = _cut(mem, codec, a_fr, a_or, a_fo, n_frames, dst_capacity, stop)
    return out


def checksum_seed(algo: int, lengths, seeds, own):
    """checksum_seed_kernel<ALGO>: own[i] = the checksum of a range of lengths[i] bytes alone -> its state behind seeds[i]"""
    n = len(lengths)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    mem = emu.Memory(None)
    a_off = mem.map(offs, "offsets", writable=False)
    a_tab = mem.map(ck.tables(0x82F63B78 if algo == 3 else 0xEDB88320), "tables", writable=False)
    a_seed = mem.map(np.asarray(seeds, np.int64), "seeds", writable=False)
    out = np.asarray(own, np.int64).copy()
    a_out = mem.map(out, "out")
    _launch(STREAM, "checksum_seed_kernelILi%dE" % (1 if algo == 1 else 2), mem, struct.pack("<QiiQQQ", a_off, n, 0, a_tab, a_seed, a_out),
            (n + 63) // 64)
    return [int(x) for x in out]
