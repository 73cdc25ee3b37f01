"""Runs the compiled kernels of the batched feed (s3s_dstream_feed_batch*, csrc/decode_stream_batch.hip) on the CPU through
tests/isa/gfx950_emu.py (TEST INFRASTRUCTURE), several windows per launch, in the order a batched feed launches them:

  LZ4     tile_speculate_batch_kernel -> tile_resolve_stream_batch_kernel | host: n_frames, stop -> tile_emit_batch_kernel
          (comp_len = stop) -> frames_cut_batch_kernel | host -> frames_rebase_cut_kernel
  Snappy  snappy_walk_stream_batch_kernel<false> -> piece_scan_batch_kernel | host -> snappy_walk_stream_batch_kernel<true> ->
  / LZF   frames_cut_batch_kernel | host -> frames_rebase_cut_kernel
  seeds   checksum_seed_batch_kernel<ALGO>

Speculation and emit are the batched one-shot kernels of csrc/lz4_decompress.hip.  Every window lives in a buffer of its own
that ends with the window's last byte, and every array has exactly the size the host code gives it, so a read at or beyond a
window's comp_len - also one that would land in the next window of a packed allocation - is a fault of the interpreter's
memory."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import checksum_kernel as ck  # noqa: E402
import stream_kernel as sk  # noqa: E402

TILE = 65536
BATCH, ONE_SHOT = "decode_stream_batch.hip", "lz4_decompress.hip"
LZ4, SNAPPY, LZF = 1, 2, 4
RANGE_FMT, WIN_FMT = "<QqiiQQQQQQQQQQQqqqii", "<qqiiiiqq"  # LzRange, StreamWin (csrc/s3s_internal.h)
RANGE_BYTES, WIN_BYTES, WORDS = struct.calcsize(RANGE_FMT), struct.calcsize(WIN_FMT), 8
assert (RANGE_BYTES, WIN_BYTES) == (144, 48)
DST_BASE = 0x7000_0000_0000  # the destinations are never touched by these kernels: any address will do


def feed_batch(codec: int, wins):
    """wins: one dict per window - window (bytes), dst_capacity, and range_left (LZ4) or piece_off, first_mid, last_pend (Snappy,
    LZF); skip_after_cut (optional): the window leaves the batch behind the cut, as a wrong checksum makes it.
    -> one dict per window: status, stop, need, n_frames, k, consumed, out_len, need_dst, frames (the rebased records: (absolute
    payload address - the window's address, comp_len, orig_len, check, method)), out_abs (relative to the window's dst)"""
    m = len(wins)
    fmt = 1 if codec == LZF else 0
    mem = emu.Memory(None)
    a_comp, n_unit, first_piece = [], [], []
    for i, w in enumerate(wins):
        b = w["window"]
        assert len(b) > 0
        a_comp.append(mem.map(np.frombuffer(bytearray(b), dtype=np.uint8), "comp%d" % i, writable=False))
        n_unit.append((len(b) + TILE - 1) // TILE if codec == LZ4 else len(w["piece_off"]) - 1)
        first_piece.append(sum(n_unit[:i]) if codec != LZ4 else 0)
    total_units = sum(n_unit)
    status = np.zeros(m + 1, np.int32)
    result = np.zeros(WORDS * m, np.int64)
    a_st, a_res = mem.map(status, "status"), mem.map(result, "result")
    ws = []
    for i in range(m):
        c1 = n_unit[i] + 1 if codec == LZ4 else n_unit[i] + 2
        arrs = dict(spec_entry=np.full(c1, -7, np.int64), spec_exit=np.full(c1, -7, np.int64), true_entry=np.full(c1, -7, np.int64),
                    frame_base=np.full(c1, -7, np.int64), spec_count=np.full(c1, -7, np.int32))
        ws.append({k: (v, mem.map(v, "%s%d" % (k, i))) for k, v in arrs.items()})
    ranges, swins = np.zeros(RANGE_BYTES * m, np.uint8), np.zeros(WIN_BYTES * m, np.uint8)
    a_rng, a_win = mem.map(ranges, "ranges"), mem.map(swins, "wins")
    state = [dict(comp_len=len(w["window"]), n_frames=0, skip=0, frames=0, orig=0, fout=0, oabs=0, stop=0, first_frame=0) for w in wins]

    def pack():
        tile0 = 0
        for i, w in enumerate(wins):
            s, a = state[i], ws[i]
            struct.pack_into(RANGE_FMT, ranges, RANGE_BYTES * i, a_comp[i], s["comp_len"], n_unit[i] if codec == LZ4 else 0, tile0,
                             a["spec_entry"][1], a["spec_exit"][1], a["true_entry"][1], a["frame_base"][1], a["spec_count"][1],
                             a_st + 4 * i, a_res + 8 * WORDS * i, s["frames"], s["orig"], s["fout"], s["oabs"], s["n_frames"],
                             DST_BASE + (i << 32), w["dst_capacity"], s["skip"], 0)
            struct.pack_into(WIN_FMT, swins, WIN_BYTES * i, w.get("range_left", 0), w.get("last_pend", 0), first_piece[i],
                             n_unit[i] if codec != LZ4 else 0, int(w.get("first_mid", 0)), 0, s["stop"], s["first_frame"])
            tile0 += n_unit[i] if codec == LZ4 else 0

    unit_win = np.concatenate([np.full(n_unit[i], i, np.int32) for i in range(m)])
    a_map = mem.map(unit_win, "unit_win", writable=False)
    a_off = 0
    if codec != LZ4:
        a_off = mem.map(np.concatenate([np.asarray(w["piece_off"], np.int64) for w in wins]), "piece_off", writable=False)
    pack()
    # ---- phase 1
    if codec == LZ4:
        sk._launch(ONE_SHOT, "tile_speculate_batch_kernel", mem, struct.pack("<QQi", a_rng, a_map, total_units), total_units)
        sk._launch(BATCH, "tile_resolve_stream_batch_kernel", mem, struct.pack("<QQi", a_rng, a_win, m), m)
    else:
        sk._launch(BATCH, "snappy_walk_stream_batch_kernelILb0E", mem, struct.pack("<QQQQii", a_rng, a_win, a_off, a_map, total_units, fmt),
                   (total_units + 63) // 64)
        sk._launch(BATCH, "piece_scan_batch_kernel", mem, struct.pack("<QQi", a_rng, a_win, m), m)
    out = []
    total_frames = 0
    for i in range(m):
        r = dict(status=int(status[i]), stop=int(result[WORDS * i]), need=int(result[WORDS * i + 1]), n_frames=0, k=0, consumed=0, out_len=0,
                 need_dst=0, frames=[], out_abs=[])
        if r["status"] == 0:
            r["n_frames"] = int(result[WORDS * i + 2])
            r["consumed"] = r["stop"]
        out.append(r)
        state[i].update(n_frames=r["n_frames"], skip=int(r["status"] != 0), stop=r["stop"], first_frame=total_frames)
        if codec == LZ4 and r["status"] == 0:
            state[i]["comp_len"] = r["stop"]
        total_frames += r["n_frames"]
    if total_frames == 0:
        return out
    # ---- phase 2: the batch-wide frame table, the per-window scans of decoded sizes (one more entry per window)
    frames = np.zeros(24 * total_frames, np.uint8)
    orig = np.zeros(total_frames + m, np.uint32)
    fout, oabs = np.full(total_frames + m, -7, np.int64), np.full(total_frames, -7, np.int64)
    a_fr, a_or, a_fo, a_oa = mem.map(frames, "frames"), mem.map(orig, "frame_orig"), mem.map(fout, "frame_out"), mem.map(oabs, "out_abs")
    for i in range(m):
        f0 = state[i]["first_frame"]
        state[i].update(frames=a_fr + 24 * f0, orig=a_or + 4 * (f0 + i), fout=a_fo + 8 * (f0 + i), oabs=a_oa + 8 * f0)
    pack()
    if codec == LZ4:
        sk._launch(ONE_SHOT, "tile_emit_batch_kernel", mem, struct.pack("<QQi", a_rng, a_map, total_units), (total_units + 63) // 64)
    else:
        sk._launch(BATCH, "snappy_walk_stream_batch_kernelILb1E", mem, struct.pack("<QQQQii", a_rng, a_win, a_off, a_map, total_units, fmt),
                   (total_units + 63) // 64)
    sk._launch(BATCH, "frames_cut_batch_kernel", mem, struct.pack("<QQii", a_rng, a_win, m, codec), (m + 3) // 4, block_x=256)
    for i, r in enumerate(out):
        r["status"] = int(status[i])
        if r["status"] == 0 and r["n_frames"] > 0:
            r["k"], r["consumed"], r["out_len"], r["need_dst"] = (int(x) for x in result[WORDS * i + 4:WORDS * i + 8])
        if r["status"] != 0 or wins[i].get("skip_after_cut"):
            state[i]["skip"] = 1
    # ---- phase 3: the rebase with the cut
    pack()
    sk._launch(BATCH, "frames_rebase_cut_kernel", mem, struct.pack("<QQiiq", a_rng, a_win, m, 0, total_frames), (total_frames + 255) // 256, block_x=256)
    for i, r in enumerate(out):
        f0 = state[i]["first_frame"]
        for j in range(r["n_frames"]):
            off, clen, olen, check, method = struct.unpack_from("<qiiIi", frames, 24 * (f0 + j))
            live = not state[i]["skip"] and j < r["k"]
            r["frames"].append((off - a_comp[i] if live else off, clen, olen, check, method))
            r["out_abs"].append(int(oabs[f0 + j]) - (DST_BASE + (i << 32)))
    return out


def checksum_seed_batch(algo: int, lengths_per_window, seeds, own):
    """checksum_seed_batch_kernel<ALGO> over the flattened piece table: lengths_per_window[w] = the lengths of window w's pieces;
    seeds / own: one per piece -> the continued states"""
    offs, piece_win = [], []
    for w, lens in enumerate(lengths_per_window):
        offs += [0] + [int(x) for x in np.cumsum(lens)]
        piece_win += [w] * len(lens)
    n = len(piece_win)
    mem = emu.Memory(None)
    a_off = mem.map(np.asarray(offs, np.int64), "offsets", writable=False)
    a_pw = mem.map(np.asarray(piece_win, np.int32), "piece_win", writable=False)
    a_tab = mem.map(ck.tables(0x82F63B78 if algo == 3 else 0xEDB88320), "tables", writable=False)
    a_seed = mem.map(np.asarray(seeds, np.int64), "seeds", writable=False)
    out = np.asarray(own, np.int64).copy()
    a_out = mem.map(out, "out")
    sk._launch(BATCH, "checksum_seed_batch_kernelILi%dE" % (1 if algo == 1 else 2), mem, struct.pack("<QQiiQQQ", a_off, a_pw, n, 0, a_tab, a_seed, a_out),
               (n + 63) // 64)
    return [int(x) for x in out]
