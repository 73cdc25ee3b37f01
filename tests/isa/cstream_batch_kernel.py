"""Runs the device side of one BATCHED feed of the streaming map side (s3s_cstream_feed_batch_device, csrc/compress_stream.hip)
on the CPU through tests/isa/gfx950_emu.py (TEST INFRASTRUCTURE), in the order the call launches it, for LZ4 windows of fresh
streams:

  xxh32_items_quad_kernel -> lz4_compress_l2_kernel (csrc/lz4_compress.hip), ONE launch over the items of all windows
  -> scan_items_batch_kernel (csrc/assemble.hip)
  -> cstream_cut_batch_kernel -> gather_items_cut_batch_kernel (csrc/compress_stream_batch_kernels.hip)

and, on the same plan and the same scan, cstream_cut_kernel (csrc/compress_stream_kernels.hip) once per window, so that the two
cuts can be compared word for word.  The plan records, the marks, the TaskTail and CutEntry descriptors are built here the way
csrc/compress_stream_batch_core.h lays them out.  Every array has exactly the size the host code gives it and every window's
dst has exactly its dst_capacity bytes, so a store at or beyond the capacity is a fault of the interpreter's memory.  The
windows' sources lie in ONE region in the order `src_order` gives; the kernels get the FIRST entry's address as their base, so
an entry placed in front of it has a negative delta."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402
from cstream_kernel import SEED, _prog  # noqa: E402

CUT_WORDS = 8


def plan_window(parts, tail, block, delta, slot0):
    """parts: the partitions that end in the window; tail: whole blocks of the partition it leaves open.  -> items (bytes),
    marks (bytes), part_first (entry-relative), first_last, ends0, slots used, window length, ends"""
    level = max(0, (block - 1).bit_length() - 10)
    assert len(tail) % block == 0
    n_ends = len(parts)
    items, units, part_first = bytearray(), [], []
    off, slot = 0, slot0
    for p, b in enumerate(list(parts) + [tail]):
        part_first.append(len(items) // 24)
        for pos in range(0, len(b), block):
            n = min(block, len(b) - pos)
            items += struct.pack("<qiiii", delta + off + pos, n, 0 | (level << 8), slot, p)
            units.append((len(items) // 24 - 1, off + pos + n, p))
            slot += 1
        if b and p < n_ends:
            items += struct.pack("<qiiii", 0, 0, 1 | (level << 8), -1, p)  # kItemLz4End
            units.append((len(items) // 24 - 1, off + len(b), p))
        off += len(b)
    n_items = len(items) // 24
    part_first.append(n_items)
    marks = b"".join(struct.pack("<qii", src_end, 1, units[u + 1][2] if u + 1 < len(units) else n_ends) for u, (_, src_end, _) in enumerate(units))
    ends = list(np.cumsum([len(b) for b in parts]).astype(int)) if parts else []
    return dict(items=bytes(items), marks=marks, part_first=part_first, first_last=units[0][0] if units else -1,
                ends0=units[0][2] if units else 0, n_slots=slot - slot0, n_items=n_items, src_len=off, ends=ends)


def feed_batch_lz4(entries, block, src_order=None):
    """entries: [dict(parts=[bytes, ...], tail=bytes, cap=int, open_img=int)], fresh streams.  -> per entry dict(k, consumed,
    out_len, need_dst, parts_closed, piece_off, lengths, status, dst, single=dict(the single cut kernel's words, piece_off,
    lengths), n_items)"""
    m = len(entries)
    stride = 32 + ((block + 15) & ~15)
    src_order = list(src_order or range(m))
    blobs = [b"".join(e["parts"]) + e.get("tail", b"") for e in entries]
    place, at = {}, 0
    for i in src_order:
        place[i] = at
        at += len(blobs[i])
    src = np.frombuffer(b"".join(blobs[i] for i in src_order), dtype=np.uint8)
    base = place[0]
    plans, first_item, first_piece, slot = [], [], [], 0
    for i, e in enumerate(entries):
        first_item.append(sum(p["n_items"] for p in plans))
        first_piece.append(sum(len(p["part_first"]) - 1 for p in plans))
        plans.append(plan_window(e["parts"], e.get("tail", b""), block, place[i] - base, slot))
        slot += plans[-1]["n_slots"]
    N, P = sum(p["n_items"] for p in plans), sum(len(p["part_first"]) - 1 for p in plans)
    PP, L = P + m, P - m
    mem = emu.Memory(None)
    a_src = mem.map(src.copy(), "src", writable=False) + base
    a_items = mem.map(np.frombuffer(b"".join(p["items"] for p in plans), dtype=np.uint8), "items", writable=False)
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
    tails, cuts = bytearray(), bytearray()
    for i, (e, p) in enumerate(zip(entries, plans)):
        n_pieces = len(p["part_first"]) - 1
        tails += struct.pack("<iiiiiiiiQqQq", first_item[i], p["n_items"], first_piece[i] + i, n_pieces, first_piece[i], 0, 0, 0,
                             a_dsts[i], e["cap"], a_dsts[i], e["cap"])
        cuts += struct.pack("<qqiiiiiiiiiiii", e["cap"], e.get("open_img", 0), first_item[i], p["n_items"], first_piece[i] + i, n_pieces,
                            first_piece[i], first_piece[i] - i, 0, 0, 0, p["n_slots"], p["first_last"], p["ends0"])
    a_tails = mem.map(np.frombuffer(tails, dtype=np.uint8), "tails", writable=False)
    a_cuts = mem.map(np.frombuffer(cuts, dtype=np.uint8), "cuts", writable=False)
    prog, entry, objs = _prog("lz4_compress.hip", "xxh32_items_quad_kernelILb0E")
    emu.launch(prog, entry, mem, struct.pack("<QQiIQ", a_src, a_items, N, SEED, a_check), (N + 15) // 16, 0, objects=objs)
    prog, entry, objs = _prog("lz4_compress.hip", "lz4_compress_l2_kernelILb1E")
    emu.launch(prog, entry, mem, struct.pack("<QQiiQQQQ", a_src, a_items, N, stride, a_check, a_slots, a_size, a_work), 1, 16384, objects=objs)
    prog, entry, objs = _prog("assemble.hip", "scan_items_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQ", a_tails, m, 0, a_size, a_off, a_pf, a_index), m, 0, objects=objs)
    prog, entry, objs = _prog("compress_stream_batch_kernels.hip", "cstream_cut_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQQQ", a_cuts, m, 0, a_marks, a_off, a_pf, a_res, a_piece, a_len), m, 0, objects=objs)
    prog, entry, objs = _prog("compress_stream_batch_kernels.hip", "gather_items_cut_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQqQQQ", a_tails, m, N, a_src, a_items, a_res, a_slots, stride, a_size, a_off, a_status),
               N, 0, block_x=256, objects=objs)
    out = []
    for i, (e, p) in enumerate(zip(entries, plans)):
        n_pieces = len(p["part_first"]) - 1
        n_ends = n_pieces - 1
        pp, ln = first_piece[i] + i, first_piece[i] - i
        r = result[CUT_WORDS * i:CUT_WORDS * (i + 1)]
        # the single cut kernel on this window's slice of the plan and of the scan, in arrays of their own
        m1 = emu.Memory(None)
        s_res, s_piece = np.full(CUT_WORDS, -7, np.int64), np.full(n_pieces + 1, -7, np.int64)
        s_len = np.full(max(n_ends, 1), -7, np.int64)[:n_ends]
        b_marks = m1.map(np.frombuffer(p["marks"], dtype=np.uint8), "marks", writable=False)
        b_off = m1.map(item_off[first_item[i] + i:first_item[i] + i + p["n_items"] + 1].copy(), "item_off", writable=False)
        b_pf = m1.map(np.array(p["part_first"], np.int32), "part_first", writable=False)
        b_res, b_piece = m1.map(s_res, "cut_result"), m1.map(s_piece, "piece_off")
        b_len = m1.map(s_len if n_ends else np.zeros(1, np.int64), "lengths")
        prog, entry, objs = _prog("compress_stream_kernels.hip", "cstream_cut_kernel")
        emu.launch(prog, entry, m1, struct.pack("<QQiiQiiqiiqQQQ", b_marks, b_off, p["n_items"], 0, b_pf, n_pieces, 0, e["cap"], p["first_last"],
                                                p["ends0"], e.get("open_img", 0), b_res, b_piece, b_len), 1, 0, objects=objs)
        out.append(dict(k=int(r[0]), consumed=int(r[1]), out_len=int(r[2]), need_dst=int(r[3]), parts_closed=int(r[4]),
                        words=[int(x) for x in r], piece_off=[int(x) for x in piece_off[pp:pp + n_pieces + 1]],
                        lengths=[int(x) for x in lengths[ln:ln + n_ends]], status=int(status[i]), dst=dsts[i].tobytes(),
                        n_items=p["n_items"], src_len=p["src_len"], ends=p["ends"],
                        item_end=[int(x) for x in item_off[first_item[i] + i + 1:first_item[i] + i + p["n_items"] + 1]],
                        single=dict(words=[int(x) for x in s_res], piece_off=[int(x) for x in s_piece], lengths=[int(x) for x in s_len])))
    return out
