"""LZ4 blocks above 64 KiB through the compiled map-side kernels on the CPU (TEST INFRASTRUCTURE).

`compress_chunks_u32` runs `lz4_compress_u32_kernel` (the byU32 parse: 4096 x u32 table, 5-byte hash, distance test) on
single chunks of 65 547 bytes and more; `compress_map_output` is one whole map-side call at a block size above 64 KiB with
the item plan built the way csrc/s3s_ctx.h (lz4_chunk_kind) builds it - a chunk's kind follows its LENGTH - and the
launches of launch_lz4_compress in their order:

    xxh32_items_quad_kernel<false>      frame checks of the chunks below 65 547 bytes
    xxh32_items_wave_kernel<6>          frame checks of the byU32 chunks, one wavefront each
    lz4_compress_l2_kernel<true>        chunks below 65 547 bytes + end frames (persistent grid); passes kind 6 by
    lz4_compress_u32_kernel             the byU32 chunks, one workgroup per item; passes every other kind by
    scan_items_kernel, gather_items_kernel, checksums

Every buffer has exactly its size: a read past the last chunk's last byte faults."""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import checksum_kernel as ck  # noqa: E402
import gfx950_emu as emu  # noqa: E402
import lz4_kernel as lk  # noqa: E402

U32_FROM = 65536 + 11
K_CHUNK, K_END, K_CHUNK_U32 = 0, 1, 6
SEED = 0x9747B28C
_P = {}


_WORK = {}


def _call_work(k):
    return _WORK["fn"](k)


def _prog(src, needle):
    if src not in _P:
        text = lk.compile_asm(src)
        _P[src] = (text, {k: v for k, v in emu.parse_objects(text).items() if k.startswith("_ZN3s3s")})
    if (src, needle) not in _P:
        entry = lk.find_kernel(_P[src][0], needle)
        _P[(src, needle)] = (emu.Program(_P[src][0], entry), entry)
    return _P[(src, needle)] + (_P[src][1],)


def level(block):
    return max(0, (block - 1).bit_length() - 10)


def chunk_kind(ln):
    return K_CHUNK_U32 if ln >= U32_FROM else K_CHUNK


def compress_chunks_u32(chunks, block=None, lds_order=None, far=None, cross=None):
    """chunks: uint8 arrays of >= 65 547 bytes.  -> [(payload or None when stored RAW, 21-byte frame header, wave)]
    far = {"src": K, "slots": K}: the kernel gets `src - K` with Item.src_off + K, and `slots - chunk0 * stride` with
    Item.chunk from chunk0 on (the first slot whose byte offset lies above K); cross = {region name: byte}: gfx950_emu.Memory(cross)"""
    prog, entry, objs = _prog("lz4_compress.hip", "lz4_compress_u32_kernel")
    block = block or max(len(c) for c in chunks)
    stride = 32 + ((block + 15) & ~15)
    n = len(chunks)
    mem = emu.Memory(cross)
    far = far or {}
    k_src = far.get("src", 0)
    ch0 = far.get("slots", 0) // stride + 1 if far.get("slots", 0) else 0
    src = np.concatenate([np.asarray(c, dtype=np.uint8) for c in chunks])
    items = bytearray()
    off = k_src
    for k, c in enumerate(chunks):
        assert len(c) >= U32_FROM
        items += struct.pack("<qiiii", off, len(c), K_CHUNK_U32 | (level(block) << 8), ch0 + k, 0)
        off += len(c)
    slots = np.zeros(n * stride, np.uint8)
    sizes = np.zeros(n, np.uint32)
    checks = (np.arange(n, dtype=np.uint32) + np.uint32(3)) * np.uint32(0x01010101)
    a_src = mem.map(src, "src", writable=False) - k_src
    a_items = mem.map(np.frombuffer(items, dtype=np.uint8), "items", writable=False)
    a_check = mem.map(checks, "item_check", writable=False)
    a_slots, a_sizes = mem.map(slots, "slots") - ch0 * stride, mem.map(sizes, "item_size")
    waves = emu.launch(prog, entry, mem, struct.pack("<QQiiQQQ", a_src, a_items, n, stride, a_check, a_slots, a_sizes), n, 16384,
                       lds_order=lds_order, objects=objs)
    out = []
    for k in range(n):
        sz = int(sizes[k])
        slot = slots[k * stride:(k + 1) * stride]
        plen = (sz & 0x7FFFFFFF) - 21
        payload = None if sz & 0x80000000 else bytes(slot[32:32 + plen])
        out.append((payload, bytes(slot[11:32]), waves[k]))
    return out


def expected_header(chunk, payload, block, check):
    """the frame header the kernel must write for a chunk whose liblz4 payload is `payload`, frame check `check`"""
    raw = len(payload) >= len(chunk)
    return b"LZ4Block" + bytes([(0x10 if raw else 0x20) | level(block)]) + struct.pack(
        "<iiI", len(chunk) if raw else len(payload), len(chunk), check & 0x0FFFFFFF)


def compress_map_output(parts, algo, dst_bytes, block, far=None, cross=None):
    """parts: list of bytes (one per partition, may be empty) -> (status, image bytes, index [n + 1], checksums [n] or None)
    far = {"src": K, "slots": K, "dst": K} / cross: as tests/isa/map_side.py::compress_map_output"""
    n = len(parts)
    lv = level(block)
    stride = 32 + ((block + 15) & ~15)
    far = far or {}
    k_src, k_dst = far.get("src", 0), far.get("dst", 0)
    ch0 = far.get("slots", 0) // stride + 1 if far.get("slots", 0) else 0
    src = np.frombuffer(b"".join(parts), dtype=np.uint8)
    items = bytearray()
    part_first = []
    off, ch = k_src, ch0
    for p, b in enumerate(parts):
        part_first.append(len(items) // 24)
        for pos in range(0, len(b), block):
            ln = min(block, len(b) - pos)
            items += struct.pack("<qiiii", off + pos, ln, chunk_kind(ln) | (lv << 8), ch, p)
            ch += 1
        if b:
            items += struct.pack("<qiiii", 0, 0, K_END | (lv << 8), -1, p)
        off += len(b)
    n_items = len(items) // 24
    part_first.append(n_items)
    mem = emu.Memory(cross)
    a_src = mem.map(src.copy() if src.size else np.zeros(1, np.uint8), "src", writable=False) - k_src
    a_items = mem.map(np.frombuffer(items or bytearray(24), dtype=np.uint8), "items", writable=False)
    check = np.zeros(max(n_items, 1), np.uint32)
    size = np.zeros(max(n_items, 1), np.uint32)
    item_off = np.full(n_items + 1, -7, np.int64)
    index = np.full(n + 1, -7, np.int64)
    slots = np.zeros(max(ch - ch0, 1) * stride, np.uint8)
    work = np.zeros(1, np.uint32)
    status = np.zeros(1, np.int32)
    dst = np.full(max(dst_bytes, 1), 0xA5, np.uint8)[:dst_bytes]
    a_check, a_size, a_off, a_index = (mem.map(check, "item_check"), mem.map(size, "item_size"), mem.map(item_off, "item_off"),
                                       mem.map(index, "index"))
    a_slots, a_work, a_status = mem.map(slots, "slots") - ch0 * stride, mem.map(work, "work"), mem.map(status, "status")
    a_pf = mem.map(np.array(part_first, np.int32), "part_first", writable=False)
    a_dst = mem.map(dst if dst_bytes else np.zeros(1, np.uint8), "dst") - k_dst
    if n_items:
        prog, entry, objs = _prog("lz4_compress.hip", "xxh32_items_quad_kernelILb0E")
        emu.launch(prog, entry, mem, struct.pack("<QQiIQ", a_src, a_items, n_items, SEED, a_check), (n_items + 15) // 16, 0, objects=objs)
        prog, entry, objs = _prog("lz4_compress.hip", "xxh32_items_wave_kernelILi6E")
        emu.launch(prog, entry, mem, struct.pack("<QQiIQ", a_src, a_items, n_items, SEED, a_check), n_items, 0, objects=objs)
        prog, entry, objs = _prog("lz4_compress.hip", "lz4_compress_l2_kernelILb1E")
        emu.launch(prog, entry, mem, struct.pack("<QQiiQQQQ", a_src, a_items, n_items, stride, a_check, a_slots, a_size, a_work), 1, 16384,
                   objects=objs)
        assert int(work[0]) == n_items + 1
        prog, entry, objs = _prog("lz4_compress.hip", "lz4_compress_u32_kernel")
        kernarg = struct.pack("<QQiiQQQ", a_src, a_items, n_items, stride, a_check, a_slots, a_size)
        u32_items = [k for k in range(n_items) if items[24 * k + 12] == K_CHUNK_U32]
        emu.launch(prog, entry, mem, kernarg, [k for k in range(n_items) if k not in u32_items], 16384, objects=objs)  # pass by
        # The workgroups of this launch are independent (one item, one slot, one item_size word each) and the interpreter takes
        # 10 - 50 s for each: they are dealt out to a few forked workers, which hand back what their workgroup wrote.
        def one(k):
            emu.launch(prog, entry, mem, kernarg, [k], 16384, objects=objs)
            c = struct.unpack_from("<i", items, 24 * k + 16)[0] - ch0
            return k, c, slots[c * stride:(c + 1) * stride].copy(), int(size[k])

        _WORK["fn"] = one
        import multiprocessing
        with multiprocessing.get_context("fork").Pool(max(1, min(4, os.cpu_count() or 1, len(u32_items) or 1))) as pool:
            for k, c, slot, sz in pool.map(_call_work, u32_items, chunksize=1):
                slots[c * stride:(c + 1) * stride] = slot
                size[k] = sz
    prog, entry, objs = _prog("assemble.hip", "scan_items_kernel")
    emu.launch(prog, entry, mem, struct.pack("<QiiQQiiQ", a_size, n_items, 0, a_off, a_pf, n, 0, a_index), 1, 0, objects=objs)
    item_off += k_dst
    if n_items:
        prog, entry, objs = _prog("assemble.hip", "gather_items_kernel")
        emu.launch(prog, entry, mem, struct.pack("<QQiiQqQQQqQ", a_src, a_items, n_items, 0, a_slots, stride, a_size, a_off,
                                                 a_dst, dst_bytes + k_dst, a_status), n_items, 0, block_x=256, objects=objs)
    idx = [int(x) for x in index]
    sums = None
    if algo and int(status[0]) == 0:
        sums = ck.checksum_ranges(algo, dst.tobytes(), idx, data_len=dst_bytes)
    return int(status[0]), dst.tobytes(), idx, sums
