"""Runs the device side of one BATCHED feed of the streaming map side under IO encryption (s3s_cstream_feed_batch_device over
streams of s3s_cstream_open_encrypted, csrc/compress_stream.hip) on the CPU through tests/isa/gfx950_emu.py
(TEST INFRASTRUCTURE), in the order the call launches it, for LZ4 windows on plans WITH IV records:

  xxh32_items_quad_kernel -> lz4_compress_l2_kernel (csrc/lz4_compress.hip), ONE launch over the items of all windows
  -> [item_size of the kItemIv records] -> scan_items_batch_kernel (csrc/assemble.hip)
  -> cstream_cut_batch_kernel -> gather_items_cut_batch_kernel (csrc/compress_stream_batch_kernels.hip)
  -> aes_ctr_cstream_batch_kernel<10> (csrc/aes_ctr_cstream_batch.hip), ONE launch over the outputs of all windows

and, on a copy of every window's output as the gather left it, aes_ctr_cstream_kernel<10, in place> (csrc/aes_ctr_cstream.hip)
with that window's piece offsets, IVs and cut words, so that the two passes can be compared byte for byte.  The plan records,
the marks and the TaskTail, CutEntry and PassWindow descriptors are built here the way csrc/compress_stream_batch_core.h lays
them out; the 16 bytes of a kItemIv record are what seed_iv_items_kernel (csrc/aes_ctr.hip) writes - one compare and one store,
done here on the host.  Every window's dst has exactly its dst_capacity bytes, so a store at or beyond the capacity is a fault
of the interpreter's memory, and the stores of the pass are counted per byte."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
from cstream_kernel import SEED, _P, _prog  # noqa: E402
from stream_batch_encrypted_kernel import CountingMemory  # noqa: E402

CUT_WORDS = 8
ITEM_IV = 10
PASS_TILE = 16384                 # s3s_cs::kPassTile
WIN_FMT = "<QQQQiiq"              # s3s_cs::PassWindow: out, E, ivs, cut, n_pieces, tile0, front
WIN_BYTES = struct.calcsize(WIN_FMT)
assert WIN_BYTES == 48


def feed_bound_encrypted(block, src_len, n_ends):
    blocks = src_len // block + n_ends + 1
    return src_len + 21 * (blocks + n_ends) + 16 * (n_ends + 1)


def pass_tiles(cap, bound, front):
    """s3s_cs::pass_tiles"""
    n = min(cap, bound)
    return 0 if n <= 0 else (n + (front & 15) + PASS_TILE - 1) // PASS_TILE


def plan_window(parts, tail, block, delta, slot0, continues):
    """parts: the partitions that end in the window; tail: whole blocks of the partition it leaves open; continues: piece 0 goes
    on with a partition that earlier feeds opened (no IV record).  One kItemIv record (no slot; mark with last = 0) in front of
    the first block of every other non-empty piece, part_first pointing at it."""
    level = max(0, (block - 1).bit_length() - 10)
    assert len(tail) % block == 0
    n_ends = len(parts)
    items, units, part_first = bytearray(), [], []  # units: (first item, last item, source offset behind it, piece)
    off, slot = 0, slot0
    for p, b in enumerate(list(parts) + [tail]):
        part_first.append(len(items) // 24)
        for pos in range(0, len(b), block):
            n = min(block, len(b) - pos)
            first = len(items) // 24
            if pos == 0 and not (p == 0 and continues):
                items += struct.pack("<qiiii", 0, 0, ITEM_IV, -1, p)
            items += struct.pack("<qiiii", delta + off + pos, n, 0 | (level << 8), slot, p)
            units.append((first, len(items) // 24 - 1, off + pos + n, p))
            slot += 1
        if (b or (p == 0 and continues)) and p < n_ends:
            items += struct.pack("<qiiii", 0, 0, 1 | (level << 8), -1, p)  # kItemLz4End
            units.append((len(items) // 24 - 1, len(items) // 24 - 1, off + len(b), p))
        off += len(b)
    n_items = len(items) // 24
    part_first.append(n_items)
    marks = []
    for u, (i0, i1, src_end, _) in enumerate(units):
        after = units[u + 1][3] if u + 1 < len(units) else n_ends
        marks += [struct.pack("<qii", src_end, 1 if i == i1 else 0, after) for i in range(i0, i1 + 1)]
    assert len(marks) == n_items
    ends = list(np.cumsum([len(b) for b in parts]).astype(int)) if parts else []
    return dict(items=bytes(items), marks=b"".join(marks), part_first=part_first, first_last=units[0][1] if units else -1,
                ends0=units[0][3] if units else 0, n_slots=slot - slot0, n_items=n_items, src_len=off, ends=ends)


def feed_batch_lz4_encrypted(entries, block, round_keys, extra_tiles=0):
    """entries: [dict(parts=[bytes, ...], tail=bytes, cap=int, open_img=int (> 0: piece 0 continues an open partition),
    ivs=uint8[n_ends + 1, 16] (entry 0: the carried IV when open_img > 0))]; round_keys: 44 uint32 of an AES-128 key.
    -> per entry dict(k, consumed, out_len, need_dst, parts_closed, piece_off, lengths, status, holed (dst as the gather left
    it), dst (behind the batched pass), pass_writes (stores of the pass per byte of dst), single (dst behind the single kernel
    on the same plan), tiles, tile0, n_items, src_len, ends)"""
    m = len(entries)
    stride = 32 + ((block + 15) & ~15)
    blobs = [b"".join(e["parts"]) + e.get("tail", b"") for e in entries]
    place = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(int)
    src = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    plans, first_item, first_piece, slot = [], [], [], 0
    for i, e in enumerate(entries):
        first_item.append(sum(p["n_items"] for p in plans))
        first_piece.append(sum(len(p["part_first"]) - 1 for p in plans))
        plans.append(plan_window(e["parts"], e.get("tail", b""), block, int(place[i]), slot, e.get("open_img", 0) > 0))
        slot += plans[-1]["n_slots"]
    N, P = sum(p["n_items"] for p in plans), sum(len(p["part_first"]) - 1 for p in plans)
    PP, L = P + m, P - m
    all_items = b"".join(p["items"] for p in plans)
    kinds = [struct.unpack_from("<i", all_items, 24 * i + 12)[0] & 0xFF for i in range(N)]
    mem = CountingMemory()
    a_src = mem.map(src.copy(), "src", writable=False)
    a_items = mem.map(np.frombuffer(all_items, dtype=np.uint8), "items", writable=False)
    a_marks = mem.map(np.frombuffer(b"".join(p["marks"] for p in plans), dtype=np.uint8), "marks", writable=False)
    a_pf = mem.map(np.array([x for p in plans for x in p["part_first"]], np.int32), "part_first", writable=False)
    check, size = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    item_off, index = np.full(N + m, -7, np.int64), np.full(PP, -7, np.int64)
    slots, work, status = np.zeros(max(slot, 1) * stride, np.uint8), np.zeros(1, np.uint32), np.zeros(m, np.int32)
    result, piece_off = np.full(CUT_WORDS * m, -7, np.int64), np.full(PP, -7, np.int64)
    lengths = np.full(max(L, 1), -7, np.int64)[:L]
    dsts = [np.full(max(e["cap"], 1), 0xA5, np.uint8)[:e["cap"]] for e in entries]
    a_dsts = [mem.map(d if d.size else np.zeros(1, np.uint8), "dst%d" % i) for i, d in enumerate(dsts)]
    a_check, a_size, a_off, a_index = mem.map(check, "item_check"), mem.map(size, "item_size"), mem.map(item_off, "item_off"), mem.map(index, "index")
    a_slots, a_work, a_status = mem.map(slots, "slots"), mem.map(work, "work"), mem.map(status, "status")
    a_res, a_piece = mem.map(result, "cut_result"), mem.map(piece_off, "piece_off")
    a_len = mem.map(lengths if L else np.zeros(1, np.int64), "lengths")
    ivs = np.concatenate([np.ascontiguousarray(e["ivs"], dtype=np.uint8).reshape(-1) for e in entries])
    assert ivs.size == 16 * P
    a_ivs = mem.map(ivs, "ivs", writable=False)
    tails, cuts, wins, tile_win, tile0s = bytearray(), bytearray(), bytearray(), [], []
    for i, (e, p) in enumerate(zip(entries, plans)):
        n_pieces = len(p["part_first"]) - 1
        front = e.get("open_img", 0)
        tails += struct.pack("<iiiiiiiiQqQq", first_item[i], p["n_items"], first_piece[i] + i, n_pieces, first_piece[i], 0, 0, 0,
                             a_dsts[i], e["cap"], a_dsts[i], e["cap"])
        cuts += struct.pack("<qqiiiiiiiiiiii", e["cap"], front, first_item[i], p["n_items"], first_piece[i] + i, n_pieces,
                            first_piece[i], first_piece[i] - i, 0, 0, 0, p["n_slots"], p["first_last"], p["ends0"])
        t = pass_tiles(e["cap"], feed_bound_encrypted(block, p["src_len"], n_pieces - 1), front)
        tile0s.append(len(tile_win))
        wins += struct.pack(WIN_FMT, a_dsts[i], a_piece + 8 * (first_piece[i] + i), a_ivs + 16 * first_piece[i], a_res + 8 * CUT_WORDS * i,
                            n_pieces, len(tile_win), front)
        tile_win += [i] * t
    a_tails = mem.map(np.frombuffer(tails, dtype=np.uint8), "tails", writable=False)
    a_cuts = mem.map(np.frombuffer(cuts, dtype=np.uint8), "cuts", writable=False)
    a_wins = mem.map(np.frombuffer(wins, dtype=np.uint8), "pass_windows", writable=False)
    a_map = mem.map(np.asarray(tile_win if tile_win else [0], np.int32), "tile_win", writable=False)
    prog, entry, objs = _prog("lz4_compress.hip", "xxh32_items_quad_kernelILb0E")
    emu.launch(prog, entry, mem, struct.pack("<QQiIQ", a_src, a_items, N, SEED, a_check), (N + 15) // 16, 0, objects=objs)
    prog, entry, objs = _prog("lz4_compress.hip", "lz4_compress_l2_kernelILb1E")
    emu.launch(prog, entry, mem, struct.pack("<QQiiQQQQ", a_src, a_items, N, stride, a_check, a_slots, a_size, a_work), 1, 16384, objects=objs)
    for i, kind in enumerate(kinds):  # seed_iv_items_kernel, once over the items of the whole call
        if kind == ITEM_IV:
            size[i] = 16
    prog, entry, objs = _prog("assemble.hip", "scan_items_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQ", a_tails, m, 0, a_size, a_off, a_pf, a_index), m, 0, objects=objs)
    prog, entry, objs = _prog("compress_stream_batch_kernels.hip", "cstream_cut_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQQQ", a_cuts, m, 0, a_marks, a_off, a_pf, a_res, a_piece, a_len), m, 0, objects=objs)
    prog, entry, objs = _prog("compress_stream_batch_kernels.hip", "gather_items_cut_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQqQQQ", a_tails, m, N, a_src, a_items, a_res, a_slots, stride, a_size, a_off, a_status),
               N, 0, block_x=256, objects=objs)
    holed = [d.copy() for d in dsts]
    before = [mem.writes["dst%d" % i].copy() for i in range(m)]
    rk = np.zeros(60, np.uint32)
    rk[:44] = round_keys
    total = len(tile_win)
    if total:
        prog, entry, _ = _prog("aes_ctr_cstream_batch.hip", "aes_ctr_cstream_batch_kernelILi10E")
        emu.launch(prog, entry, mem, rk.tobytes() + struct.pack("<QQi", a_wins, a_map, total), total + extra_tiles, 0, block_x=256,
                   objects=emu.parse_objects(_P["aes_ctr_cstream_batch.hip"][0]))
    out = []
    for i, (e, p) in enumerate(zip(entries, plans)):
        n_pieces = len(p["part_first"]) - 1
        n_ends = n_pieces - 1
        pp, ln = first_piece[i] + i, first_piece[i] - i
        r = result[CUT_WORDS * i:CUT_WORDS * (i + 1)]
        front = e.get("open_img", 0)
        # the single kernel on a copy of what the gather left, with this window's offsets, IVs and cut words in arrays of their own
        single = holed[i].copy()
        tiles = pass_tiles(e["cap"], feed_bound_encrypted(block, p["src_len"], n_ends), front)
        if tiles:
            m1 = emu.Memory(None)
            b_dst = m1.map(single, "dst")
            b_piece = m1.map(piece_off[pp:pp + n_pieces + 1].copy(), "piece_off", writable=False)
            b_ivs = m1.map(ivs[16 * first_piece[i]:16 * (first_piece[i] + n_pieces)].copy(), "ivs", writable=False)
            b_res = m1.map(r.copy(), "cut_result", writable=False)
            prog, entry, _ = _prog("aes_ctr_cstream.hip", "aes_ctr_cstream_kernelILi10ELi0E")
            emu.launch(prog, entry, m1, rk.tobytes() + struct.pack("<QQQQQQiiqq", 0, b_dst, b_piece, 0, b_ivs, b_res, n_pieces, 0, front, 0),
                       tiles, 0, block_x=256, objects=emu.parse_objects(_P["aes_ctr_cstream.hip"][0]))
        out.append(dict(k=int(r[0]), consumed=int(r[1]), out_len=int(r[2]), need_dst=int(r[3]), parts_closed=int(r[4]),
                        piece_off=[int(x) for x in piece_off[pp:pp + n_pieces + 1]], lengths=[int(x) for x in lengths[ln:ln + n_ends]],
                        status=int(status[i]), holed=holed[i].tobytes(), dst=dsts[i].tobytes(),
                        pass_writes=mem.writes["dst%d" % i] - before[i], single=single.tobytes(), tiles=tiles, tile0=tile0s[i],
                        n_items=p["n_items"], src_len=p["src_len"], ends=p["ends"]))
    return out
