"""Runs the device side of one feed of the streaming map side under IO encryption (s3s_cstream_open_encrypted,
csrc/compress_stream.hip) on the CPU through tests/isa/gfx950_emu.py (TEST INFRASTRUCTURE), up to the cut gather and, with a key,
the encrypt pass, for an LZ4 window whose partitions all end inside it, on a plan WITH IV records:

  xxh32_items_quad_kernel -> lz4_compress_l2_kernel (csrc/lz4_compress.hip) -> [item_size of the kItemIv records]
  -> scan_items_kernel (csrc/assemble.hip) -> cstream_cut_kernel -> gather_items_cut_kernel (csrc/compress_stream_kernels.hip)

The plan records and the marks are built here the way the host code builds them: one kItemIv record (kind 10, no slot, mark with
last = 0 and the unit's src_end) in front of the first block of every non-empty partition, part_first pointing at it.  The
16 bytes of a kItemIv record are what seed_iv_items_kernel (csrc/aes_ctr.hip) writes; it is one compare and one store and is
done here on the host.  With a key, aes_ctr_cstream_kernel<10, in place> (csrc/aes_ctr_cstream.hip) runs behind the gather, on a
grid sized from dst_capacity alone, and reads out_len from the cut's result words.  Every array has
exactly the size the host code gives it and dst has exactly dst_capacity bytes, so a store at or beyond the capacity is a fault
of the interpreter's memory."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
from cstream_kernel import SEED, _P, _prog  # noqa: E402

ITEM_IV = 10
PREFILL = 0xA5


def feed_lz4_encrypted(parts, block, dst_capacity, open_img=0, round_keys=None, ivs=None):
    """parts: the bytes of the partitions that end in the window, in order (a fresh stream).  round_keys (44 uint32 of an
    AES-128 key) and ivs (16 bytes a piece, n_ends + 1 pieces): also run the encrypt pass in place.
    -> dict(k, consumed, out_len, need_dst, parts_closed, piece_off, lengths, status, dst)"""
    level = max(0, (block - 1).bit_length() - 10)
    stride = 32 + ((block + 15) & ~15)
    src = np.frombuffer(b"".join(parts), dtype=np.uint8)
    n_ends = len(parts)
    items, marks, part_first = bytearray(), [], []
    off = ch = 0
    units = []  # (first item, last item, source offset behind it, piece)
    for p, b in enumerate(parts):
        part_first.append(len(items) // 24)
        for pos in range(0, len(b), block):
            n = min(block, len(b) - pos)
            first = len(items) // 24
            if pos == 0:
                items += struct.pack("<qiiii", 0, 0, ITEM_IV, -1, p)
            items += struct.pack("<qiiii", off + pos, n, 0 | (level << 8), ch, p)
            units.append((first, len(items) // 24 - 1, off + pos + n, p))
            ch += 1
        if b:
            items += struct.pack("<qiiii", 0, 0, 1 | (level << 8), -1, p)  # kItemLz4End
            units.append((len(items) // 24 - 1, len(items) // 24 - 1, off + len(b), p))
        off += len(b)
    n_items = len(items) // 24
    assert n_items > 0
    part_first += [n_items, n_items]
    n_pieces = n_ends + 1
    for u, (i0, i1, src_end, piece) in enumerate(units):  # s3s_cs::Mark { src_end, last, ends_after }
        after = units[u + 1][3] if u + 1 < len(units) else n_ends
        for i in range(i0, i1 + 1):
            marks.append(struct.pack("<qii", src_end, 1 if i == i1 else 0, after))
    assert len(marks) == n_items
    kinds = [struct.unpack_from("<i", items, 24 * i + 12)[0] & 0xFF for i in range(n_items)]
    mem = emu.Memory(None)
    a_src = mem.map(src.copy(), "src", writable=False)
    a_items = mem.map(np.frombuffer(items, dtype=np.uint8), "items", writable=False)
    a_marks = mem.map(np.frombuffer(b"".join(marks), dtype=np.uint8), "marks", writable=False)
    check, size = np.zeros(n_items, np.uint32), np.zeros(n_items, np.uint32)
    item_off, index = np.full(n_items + 1, -7, np.int64), np.full(n_pieces + 1, -7, np.int64)
    slots, work, status = np.zeros(max(ch, 1) * stride, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    result, piece_off, lengths = np.full(8, -7, np.int64), np.full(n_pieces + 1, -7, np.int64), np.full(max(n_ends, 1), -7, np.int64)[:n_ends]
    dst = np.full(max(dst_capacity, 1), PREFILL, np.uint8)[:dst_capacity]
    a_check, a_size, a_off, a_index = mem.map(check, "item_check"), mem.map(size, "item_size"), mem.map(item_off, "item_off"), mem.map(index, "index")
    a_slots, a_work, a_status = mem.map(slots, "slots"), mem.map(work, "work"), mem.map(status, "status")
    a_pf = mem.map(np.array(part_first, np.int32), "part_first", writable=False)
    a_res, a_piece = mem.map(result, "cut_result"), mem.map(piece_off, "piece_off")
    a_len = mem.map(lengths if n_ends else np.zeros(1, np.int64), "lengths")
    a_dst = mem.map(dst if dst_capacity else np.zeros(1, np.uint8), "dst")
    prog, entry, objs = _prog("lz4_compress.hip", "xxh32_items_quad_kernelILb0E")
    emu.launch(prog, entry, mem, struct.pack("<QQiIQ", a_src, a_items, n_items, SEED, a_check), (n_items + 15) // 16, 0, objects=objs)
    prog, entry, objs = _prog("lz4_compress.hip", "lz4_compress_l2_kernelILb1E")
    emu.launch(prog, entry, mem, struct.pack("<QQiiQQQQ", a_src, a_items, n_items, stride, a_check, a_slots, a_size, a_work), 1, 16384, objects=objs)
    for i, kind in enumerate(kinds):  # seed_iv_items_kernel
        if kind == ITEM_IV:
            size[i] = 16
    prog, entry, objs = _prog("assemble.hip", "scan_items_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQiiQ", a_size, n_items, 0, a_off, a_pf, n_pieces, 0, a_index), 1, 0, objects=objs)
    prog, entry, objs = _prog("compress_stream_kernels.hip", "cstream_cut_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QQiiQiiqiiqQQQ", a_marks, a_off, n_items, 0, a_pf, n_pieces, 0, dst_capacity, units[0][1],
                                             units[0][3], open_img, a_res, a_piece, a_len), 1, 0, objects=objs)
    prog, entry, objs = _prog("compress_stream_kernels.hip", "gather_items_cut_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QQQQqQQQqQ", a_src, a_items, a_res, a_slots, stride, a_size, a_off, a_dst, dst_capacity, a_status),
               n_items, 0, block_x=256, objects=objs)
    if round_keys is not None and dst_capacity > 0:
        rk = np.zeros(60, np.uint32)
        rk[:44] = round_keys
        iv = np.ascontiguousarray(ivs, dtype=np.uint8).reshape(-1)
        assert iv.size == 16 * n_pieces
        a_ivs = mem.map(iv, "ivs", writable=False)
        text = _prog("aes_ctr_cstream.hip", "aes_ctr_cstream_kernelILi10ELi0E")
        tiles = (dst_capacity + (open_img & 15) + 16383) // 16384
        emu.launch(text[0], text[1], mem, rk.tobytes() + struct.pack("<QQQQQQiiqq", 0, a_dst, a_piece, 0, a_ivs, a_res, n_pieces, 0, open_img, 0),
                   tiles, 0, block_x=256, objects=emu.parse_objects(_P["aes_ctr_cstream.hip"][0]))
    return dict(k=int(result[0]), consumed=int(result[1]), out_len=int(result[2]), need_dst=int(result[3]), parts_closed=int(result[4]),
                piece_off=[int(x) for x in piece_off], lengths=[int(x) for x in lengths], status=int(status[0]), dst=dst.tobytes())
