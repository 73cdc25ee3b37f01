"""Snappy chunks above 32 KiB through the compiled map-side kernels on the CPU (TEST INFRASTRUCTURE).

The item plan is built the way csrc/s3s_ctx.h (snappy_plan_chunk) builds it: a chunk of at most one 64 KiB fragment is one
kItemSnappyChunk item; a larger chunk is a kItemSnappyChunkHead item followed by one kItemSnappyFrag item per fragment.
Then the launches of compress_core in their order: snappy_compress_kernel, scan_items_kernel, gather_items_kernel (or the
batched tails: scan_items_batch_kernel / gather_items_batch_kernel).  Every buffer has exactly its size."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402

FRAGMENT = 65536
K_HEADER, K_CHUNK, K_HEAD, K_FRAG = 2, 3, 4, 5
_P = {}


def _prog(src, needle):
    if src not in _P:
        text = lk.compile_asm(src)
        _P[src] = (text, {k: v for k, v in emu.parse_objects(text).items() if k.startswith("_ZN3s3s")})
    if (src, needle) not in _P:
        entry = lk.find_kernel(_P[src][0], needle)
        _P[(src, needle)] = (emu.Program(_P[src][0], entry), entry)
    return _P[(src, needle)] + (_P[src][1],)


def slot_stride(block):
    n = min(block, FRAGMENT)
    return 32 + ((32 + n + n // 6 + 15) & ~15)


def plan_chunk(items, slot, src_off, ln, part):
    """appends the items of one chunk (bytes of 24-byte Item records); returns the next free slot"""
    if ln <= FRAGMENT:
        items += struct.pack("<qiiii", src_off, ln, K_CHUNK, slot, part)
        return slot + 1
    items += struct.pack("<qiiii", src_off, ln, K_HEAD, -1, part)
    for f in range(0, ln, FRAGMENT):
        items += struct.pack("<qiiii", src_off + f, min(FRAGMENT, ln - f), K_FRAG, slot, part)
        slot += 1
    return slot


def _plan(parts, block, off0=0, slot0=0):
    items = bytearray()
    part_first = []
    off, slot = off0, slot0
    for p, b in enumerate(parts):
        part_first.append(len(items) // 24)
        if b:
            items += struct.pack("<qiiii", 0, 0, K_HEADER, -1, p)
        for pos in range(0, len(b), block):
            slot = plan_chunk(items, slot, off + pos, min(block, len(b) - pos), p)
        off += len(b)
    part_first.append(len(items) // 24)
    return items, part_first, off, slot


def _compress(mem, a_src, items, n_items, a_slots, stride, a_size, windows):
    prog, entry, _ = _prog("snappy_compress.hip", "snappy_compress_kernelILb%dE" % (1 if windows else 0))
    objs = {k: v for k, v in emu.parse_objects(_P["snappy_compress.hip"][0]).items() if "g_sn_sched" in k or k.startswith("_ZN3s3s")}
    a_items = mem.map(np.frombuffer(items, dtype=np.uint8), "items", writable=False)
    emu.launch(prog, entry, mem, struct.pack("<QQiiQqQ", a_src, a_items, n_items, 0, a_slots, stride, a_size), n_items, 32768,
               objects=objs)
    return a_items


def _far(far, stride):
    far = far or {}
    k = far.get("slots", 0)
    return far.get("src", 0), k // stride + 1 if k else 0, far.get("dst", 0)


def compress_map_output(parts, block, dst_bytes, windows=True, far=None, cross=None):
    """parts: list of bytes (one per partition).  -> (status, .data image, index list [n + 1])
    far = {"src": K, "slots": K, "dst": K}: the kernels get `pointer - K` and every 64-bit offset they add to it is `+ K`
    (Item.src_off; Item.chunk from the first slot whose byte offset lies above K; item_off patched between scan and gather,
    dst_capacity + K); cross = {region name: byte}: gfx950_emu.Memory(cross)."""
    n = len(parts)
    stride = slot_stride(block)
    k_src, ch0, k_dst = _far(far, stride)
    items, part_first, total, n_slots = _plan(parts, block, k_src, ch0)
    n_slots -= ch0
    n_items = len(items) // 24
    mem = emu.Memory(cross)
    src = np.frombuffer(b"".join(parts), dtype=np.uint8)
    a_src = mem.map(src.copy() if src.size else np.zeros(1, np.uint8), "src", writable=False) - k_src
    size = np.zeros(max(n_items, 1), np.uint32)
    item_off = np.full(n_items + 1, -7, np.int64)
    index = np.full(n + 1, -7, np.int64)
    slots = np.zeros(max(n_slots, 1) * stride, np.uint8)
    status = np.zeros(1, np.int32)
    dst = np.full(max(dst_bytes, 1), 0xA5, np.uint8)[:dst_bytes]
    a_size, a_off, a_index = mem.map(size, "item_size"), mem.map(item_off, "item_off"), mem.map(index, "index")
    a_slots, a_status = mem.map(slots, "slots") - ch0 * stride, mem.map(status, "status")
    a_pf = mem.map(np.array(part_first, np.int32), "part_first", writable=False)
    a_dst = mem.map(dst if dst_bytes else np.zeros(1, np.uint8), "dst") - k_dst
    a_items = _compress(mem, a_src, items, n_items, a_slots, stride, a_size, windows) if n_items else 0
    prog, entry, objs = _prog("assemble.hip", "scan_items_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQiiQ", a_size, n_items, 0, a_off, a_pf, n, 0, a_index), 1, 0, objects=objs)
    item_off += k_dst
    if n_items:
        prog, entry, objs = _prog("assemble.hip", "gather_items_kernel")
        emu.launch(prog, entry, mem, struct.pack("<QQiiQqQQQqQ", a_src, a_items, n_items, 0, a_slots, stride, a_size, a_off,
                                                 a_dst, dst_bytes + k_dst, a_status), n_items, 0, block_x=256, objects=objs)
    return int(status[0]), dst.tobytes(), [int(x) for x in index]


def compress_map_outputs_batch(tasks, block, dst_bytes_per_task, windows=True, far=None, cross=None):
    """A batched Snappy map-side call: ONE compress launch over the items of every task, then the tail kernels once per
    call through TaskTail descriptors.  -> list of (status, image, index) per task."""
    T = len(tasks)
    stride = slot_stride(block)
    items = bytearray()
    pf_all, first_item, first_part, n_parts = [], [], [], []
    k_src, ch0, k_dst = _far(far, stride)  # (as compress_map_output; "dst" shifts every task's TaskTail.dst: regions dst0, dst1, ...)
    off, slot = k_src, ch0
    for parts in tasks:
        first_item.append(len(items) // 24)
        first_part.append(sum(n_parts))
        n_parts.append(len(parts))
        it, pf, off, slot = _plan(parts, block, off, slot)
        items += it
        pf_all += pf
    n_items = len(items) // 24
    first_item.append(n_items)
    total_parts = sum(n_parts)
    mem = emu.Memory(cross)
    slot -= ch0
    src = np.frombuffer(b"".join(b"".join(p) for p in tasks), dtype=np.uint8)
    a_src = mem.map(src.copy() if src.size else np.zeros(1, np.uint8), "src", writable=False) - k_src
    size = np.zeros(max(n_items, 1), np.uint32)
    item_off = np.full(n_items + T + 1, -7, np.int64)
    index = np.full(total_parts + T, -7, np.int64)
    slots = np.zeros(max(slot, 1) * stride, np.uint8)
    status = np.zeros(T + 1, np.int32)
    dsts = [np.full(max(n, 1), 0xA5, np.uint8)[:n] for n in dst_bytes_per_task]
    a_dsts = [mem.map(d if d.size else np.zeros(1, np.uint8), "dst%d" % t) for t, d in enumerate(dsts)]
    a_size, a_off, a_index = mem.map(size, "item_size"), mem.map(item_off, "item_off"), mem.map(index, "index")
    a_slots, a_status = mem.map(slots, "slots") - ch0 * stride, mem.map(status, "status")
    a_pf = mem.map(np.array(pf_all, np.int32), "part_first", writable=False)
    tails = bytearray()
    for t in range(T):
        tails += struct.pack("<iiiiiiiiQqQq", first_item[t], first_item[t + 1] - first_item[t], first_part[t] + t, n_parts[t],
                             first_part[t], 0, 0, 0, a_dsts[t], dst_bytes_per_task[t], a_dsts[t] - k_dst, dst_bytes_per_task[t] + k_dst)
    a_tails = mem.map(np.frombuffer(tails, dtype=np.uint8), "tails", writable=False)
    a_items = _compress(mem, a_src, items, n_items, a_slots, stride, a_size, windows) if n_items else 0
    prog, entry, objs = _prog("assemble.hip", "scan_items_batch_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQ", a_tails, T, 0, a_size, a_off, a_pf, a_index), T, 0, objects=objs)
    item_off += k_dst
    if n_items:
        prog, entry, objs = _prog("assemble.hip", "gather_items_batch_kernel")
        emu.launch(prog, entry, mem, struct.pack("<QiiQQQqQQQ", a_tails, T, n_items, a_src, a_items, a_slots, stride, a_size, a_off,
                                                 a_status), n_items, 0, block_x=256, objects=objs)
    res = []
    for t in range(T):
        pp = first_part[t] + t
        res.append((int(status[t]), dsts[t].tobytes(), [int(x) for x in index[pp:pp + n_parts[t] + 1]]))
    return res


def compress_fragments(frags, windows=True, far=None, cross=None):
    """single fragments (<= 64 KiB each) as kItemSnappyChunk items in 64 KiB slots: -> list of raw snappy blocks
    (far = {"src": K, "slots": K} / cross: as compress_map_output)"""
    stride = slot_stride(FRAGMENT)
    k_src, ch0, _ = _far(far, stride)
    items = bytearray()
    off = k_src
    for k, c in enumerate(frags):
        items += struct.pack("<qiiii", off, len(c), K_CHUNK, ch0 + k, 0)
        off += len(c)
    mem = emu.Memory(cross)
    a_src = mem.map(np.concatenate([np.asarray(c, np.uint8) for c in frags]), "src", writable=False) - k_src
    slots = np.zeros(len(frags) * stride, np.uint8)
    size = np.zeros(len(frags), np.uint32)
    a_slots, a_size = mem.map(slots, "slots") - ch0 * stride, mem.map(size, "item_size")
    _compress(mem, a_src, items, len(frags), a_slots, stride, a_size, windows)
    out = []
    for k in range(len(frags)):
        s = slots[k * stride:(k + 1) * stride]
        clen = int.from_bytes(bytes(s[28:32]), "big")
        assert clen + 4 == int(size[k])
        out.append(bytes(s[32:32 + clen]))
    return out
