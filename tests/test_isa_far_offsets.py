"""Offsets around 2^31 and 2^32 and 4 GiB address crossings through the COMPILED kernels on the CPU (tests/isa/gfx950_emu.py).

The C-ABI takes int64 offsets, lengths and capacities everywhere.  Every other interpreter test places its regions at
0x7F0000000000 + small and starts its offsets at 0, so no offset in them has a bit above 2^17 or so and no address
computation carries from the low into the high dword.  Two devices close that gap here:

  far = K     a harness hands the kernel `pointer - K` and adds K to every 64-bit offset the kernel adds to that pointer.  The
              bytes touched are the same exactly-sized regions, the offset arithmetic runs on values around K: an offset that
              is truncated to 32 bits or sign-extended from 32 lands in unmapped memory (MemFault), a wrong-but-mapped address
              shows as a byte difference.  K = 2^31 - 100, 2^32 - 100 (the crossing falls 100 bytes into the first chunk /
              frame / checksum segment, not on its edge) and 2^32 + 2^31 + 12 345; K = 0 is what every older test runs.
  cross       gfx950_emu.Memory(cross={region: byte}) maps a region so that this byte of it has a 4 GiB-aligned address.

Expected result everywhere: what the K = 0 tests assert — bytes, index, checksums and status of the oracle (or of zlib /
libzstd / the plain Python restatement), unchanged.

Kernels of spark-s3-shuffle_amd/csrc that take a 64-bit offset, base or length, and where they are covered
(far test | crossing test).  GPU-B = tests/test_gpu_beyond_4gib.py.
"""
import os
import re
import shutil
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))
import corpus  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None,
                                reason="hipcc not available")

# kernel -> (test that shifts its offsets with far, test that puts a 4 GiB crossing into its buffers); a string that is not a
# test name is the reason why there is none
COVERAGE = {
    # csrc/lz4_compress.hip
    "xxh32_items_quad_kernel": ("test_far_whole_map_side_call", "test_crossings_whole_map_side_call"),
    "xxh32_items_wave_kernel": ("test_far_lz4_blocks_above_64k", "test_crossings_lz4_u32_chunk"),
    "lz4_compress_l2_kernel": ("test_far_lz4_chunks", "test_crossings_lz4_and_snappy_chunks"),
    "lz4_compress_u32_kernel": ("test_far_lz4_blocks_above_64k", "test_crossings_lz4_u32_chunk"),
    # csrc/snappy_compress.hip
    "snappy_compress_kernel": ("test_far_snappy_chunks_and_fragments", "test_crossings_lz4_and_snappy_chunks"),
    # csrc/assemble.hip
    "scan_items_kernel": ("test_scan_items_running_sum_passes_2_31_and_2_32",
                          "no data pointer: reads u32 sizes, writes i64 sums (arrays of a few KiB)"),
    "scan_items_batch_kernel": ("test_scan_items_running_sum_passes_2_31_and_2_32", "as scan_items_kernel"),
    "gather_items_kernel": ("test_far_whole_map_side_call", "test_crossings_whole_map_side_call"),
    "gather_items_batch_kernel": ("test_far_batched_map_side_call", "test_crossings_batched_calls"),
    # csrc/checksum.hip
    "checksum_segments_kernel": ("test_far_checksum_ranges", "test_crossings_checksum_and_discovery"),
    "checksum_segments_batch_kernel": ("test_far_batched_map_side_call", "test_crossings_batched_calls"),
    "checksum_fold_kernel": ("test_checksum_fold_and_combine_of_a_range_above_2_32", "no data pointer: folds partials"),
    "checksum_combine_kernel": ("test_checksum_fold_and_combine_of_a_range_above_2_32", "no data pointer: folds partials"),
    "checksum_combine_batch_kernel": ("test_far_batched_map_side_call", "no data pointer: folds partials"),
    # csrc/lz4_decode_batch.hip
    "batch_decode_kernel": ("test_far_batch_decoder", "test_crossings_decoders"),
    "lz4_verify_frames_kernel": ("test_far_reduce_side_ranges", "test_crossings_decoders"),
    # csrc/lz4_decompress.hip
    "lz4_decompress_valu_kernel": ("test_far_ring_decoders", "test_crossings_decoders"),
    "tile_speculate_kernel": ("tiles are k * 65536 from the range start: no 64-bit offset beyond comp_len; GPU-B case 3 runs it "
                              "over a range above 2^32", "test_crossings_checksum_and_discovery"),
    "tile_resolve_kernel": ("as tile_speculate_kernel", "test_crossings_checksum_and_discovery"),
    "tile_emit_kernel": ("as tile_speculate_kernel", "test_crossings_checksum_and_discovery"),
    "scan_u32_kernel": ("test_scan_u32_running_sum_passes_2_31_and_2_32", "no data pointer: u32 counts in, i64 sums out"),
    "tile_speculate_batch_kernel": ("LzRange carries absolute pointers: GPU-B case 4", "test_crossings_batched_calls"),
    "tile_resolve_batch_kernel": ("as tile_speculate_batch_kernel", "test_crossings_batched_calls"),
    "tile_emit_batch_kernel": ("as tile_speculate_batch_kernel", "test_crossings_batched_calls"),
    "frames_finish_batch_kernel": ("rebases to ABSOLUTE addresses (0x7F.. in the interpreter: every older batched test is far "
                                   "already); GPU-B case 4", "test_crossings_batched_calls"),
    # csrc/snappy_decompress.hip
    "snappy_count_kernel": ("test_far_reduce_side_ranges", "test_crossings_checksum_and_discovery"),
    "snappy_emit_kernel": ("test_far_reduce_side_ranges", "test_crossings_checksum_and_discovery"),
    "snappy_decompress_valu_kernel": ("test_far_ring_decoders", "test_crossings_decoders"),
    # csrc/zstd_decompress.hip
    "zstd_partitions_kernel": ("test_far_and_crossings_zstd", "test_far_and_crossings_zstd"),
    "zstd_compact_kernel": ("absolute pointers and an int length per piece (<= 64 KiB): nothing to shift; its launch site is "
                            "covered by tests/test_gpu_zstd.py", "as left"),
    # csrc/decode_api.hip (a host file the interpreter does not build)
    "rebase_frames_kernel": ("not built by the interpreter (host-side file); comp_base / dst_base are int64 sums: GPU-B case 4 "
                             "runs the batched decode over ranges whose sum passes 2^32", "as left"),
}
INTERPRETED = ["lz4_compress.hip", "snappy_compress.hip", "assemble.hip", "checksum.hip", "lz4_decode_batch.hip",
               "lz4_decompress.hip", "snappy_decompress.hip", "zstd_decompress.hip"]

KS = [(1 << 31) - 100, (1 << 32) - 100, (1 << 32) + (1 << 31) + 12345]
FAR = pytest.mark.parametrize("k", [0] + KS, ids=["K0", "K2e31-100", "K2e32-100", "K2e32+2e31+12345"])


def test_coverage_table_names_every_kernel():
    """every __global__ kernel in the compiled assembly of the files the interpreter builds has a row above, and every test a
    row names exists (a kernel added later cannot be forgotten)"""
    import lz4_kernel as lk

    found = set()
    for src in INTERPRETED:
        for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", lk.compile_asm(src), re.M):
            sym, names, at = m.group(1), [], 0
            while at < len(sym):  # the <length><identifier> pieces of the mangled name
                d = re.match(r"\d+", sym[at:])
                if d:
                    at += len(d.group(0))
                    names.append(sym[at:at + int(d.group(0))])
                    at += int(d.group(0))
                else:
                    at += 1
            names = [n for n in names if n.endswith("_kernel")]
            assert len(names) == 1, sym
            found.add(names[0])
    assert len(found) >= 29
    assert found <= set(COVERAGE), "kernels without a row in COVERAGE: %s" % sorted(found - set(COVERAGE))
    assert set(COVERAGE) - found == {"rebase_frames_kernel"}
    for kern, cells in COVERAGE.items():
        for cell in cells:
            if cell.startswith("test_"):
                assert callable(globals().get(cell)), (kern, cell)
    doc = __doc__  # (the table is the module's documentation as well)
    assert "far test | crossing test" in doc


# ---- the interpreter's memory ------------------------------------------------------------------------------------------------
def test_memory_map_takes_an_explicit_base():
    import gfx950_emu as emu

    mem = emu.Memory()
    a = mem.map(np.arange(16, dtype=np.uint8), "a")
    b = mem.map(np.arange(100, dtype=np.uint8), "b", base=(5 << 32) - 40)  # byte 40 sits on a 4 GiB-aligned address
    c = mem.map(np.zeros(8, np.uint8), "c")
    assert a == 0x7F0000000000 and b == (5 << 32) - 40 and c > a and c < 0x7F0000000000 + (1 << 26)  # (the default sequence is untouched)
    assert mem.load_scalar(b + 38, 4) == bytes([38, 39, 40, 41])  # across the boundary
    addrs = np.full(64, b + 39, np.uint64)
    got = mem.load(addrs, np.arange(64) < 2, 2)
    assert got[0].tolist() == [39, 40]
    with pytest.raises(emu.MemFault):
        mem.load_scalar(b + 98, 4)
    with pytest.raises(emu.MemFault):
        mem.find(b - 1)
    for base in (b + 99, b - 7, a, a + 15):
        with pytest.raises(emu.EmuError):
            mem.map(np.zeros(8, np.uint8), "overlap", base=base)
    mem.map(np.zeros(8, np.uint8), "touching", base=b + 100)
    m2 = emu.Memory(cross={"x": 30, "y": 0})
    x, y = m2.map(np.zeros(64, np.uint8), "x"), m2.map(np.zeros(64, np.uint8), "y")
    z = m2.map(np.zeros(64, np.uint8), "z")
    assert (x + 30) % (1 << 32) == 0 and y % (1 << 32) == 0 and x != y and z == 0x7F0000000000
    with pytest.raises(emu.EmuError):
        emu.Memory(cross={"x": 65}).map(np.zeros(64, np.uint8), "x")


def test_interpreter_models_fmamk_and_fmaak():
    """hipcc divides 64-bit integers whose high dwords are not zero (`plen / unit` of a range above 2^32 in the checksum combine
    kernel) through a float estimate with v_fmamk_f32 (D = S0 * K + S1, K the literal in third place) and v_fmaak_f32
    (D = S0 * S1 + K); no older test reached that path, so the interpreter did not know them"""
    import gfx950_emu as emu

    prog = emu.Program("k:\n\tv_fmamk_f32 v3, v1, 0x4f800000, v2\n\tv_fmaak_f32 v4, v1, v2, 0xc0400000\n\ts_endpgm\n", "k")
    w = emu.new_wave(emu.Memory(), 0)
    x = np.resize(np.array([1.5, 3.0, 2.0 ** -10, 123456.0, -7.25], np.float32), 64)
    y = np.resize(np.array([0.5, -2.0, 4096.0, 1.0], np.float32), 64)
    w.v[1][:], w.v[2][:] = x.view(np.uint32), y.view(np.uint32)
    emu.run_wave(prog, w, "k")
    assert np.array_equal(w.v[3].view(np.float32), (x.astype(np.float64) * 2.0 ** 32 + y).astype(np.float32))
    assert np.array_equal(w.v[4].view(np.float32), (x.astype(np.float64) * y - 3.0).astype(np.float32))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _chunks(seed, sizes=((7, 3000), (0, 2000), (6, 2500), (1, 2000))):
    """kinds 0, 1, 6, 7: a stored (RAW) chunk, one long match, dense sequences, TeraSort-like records"""
    rng = np.random.default_rng(seed)
    return [corpus.chunk_corpus(k, n, rng) for k, n in sizes]


def _parts(seed):
    c = _chunks(seed, ((7, 5000), (0, 3000), (6, 2500), (1, 2000), (7, 13)))
    return [c[0].tobytes(), b"", c[1].tobytes(), c[2].tobytes(), b"", c[3].tobytes(), c[4].tobytes()]


def _offs(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _far(k, *names):
    return {n: k for n in names}


# ---- A.2: far offsets, map side ----------------------------------------------------------------------------------------------------
@FAR
def test_far_lz4_chunks(oracle, k):
    """Item.src_off with d_src and item.chunk * slot_stride (an int32 argument of this kernel) with d_slots, with and without
    the window engine"""
    import lz4_kernel as lk

    chunks = _chunks(71)
    for windows in (True, False):
        res = lk.compress_chunks(chunks, windows=windows, far=_far(k, "src", "slots"))
        for c, (payload, hdr, _) in zip(chunks, res):
            ref = oracle.lz4_compress_block(c)
            assert hdr[:8] == b"LZ4Block"
            if payload is None:
                assert len(ref) >= len(c)
            else:
                assert np.array_equal(payload, ref), (windows, len(c))
        assert res[1][0] is None and res[0][0] is not None  # a stored chunk and a compressed one


@FAR
def test_far_snappy_chunks_and_fragments(oracle, k):
    """the same for snappy_compress_kernel (slot stride int64), single chunks and a 64 KiB-slot fragment"""
    import snappy_big_blocks as sbb
    import snappy_kernel as sk

    chunks = _chunks(72)
    for windows in (True, False):
        for c, (slot, sz, _) in zip(chunks, sk.compress_chunks(chunks, windows=windows, far=_far(k, "src", "slots"))):
            assert bytes(slot[32:32 + sz - 4]) == bytes(oracle.snappy_compress_block(c)), (windows, len(c))
    frags = _chunks(73, ((7, 9000), (0, 1500)))
    got = sbb.compress_fragments(frags, far=_far(k, "src", "slots"))
    assert got == [bytes(oracle.snappy_compress_block(f)) for f in frags]


@FAR
def test_far_whole_map_side_call(oracle, k):
    """every launch of compress_core in its order (frame-check pre-pass, codec kernel, scan, gather incl. the RAW copy from the
    source, checksums) with source, slots, destination (item_off[] patched by + K between scan and gather, dst_capacity + K)
    and the checksum data all shifted; and the capacity test `off + n > dst_capacity` one byte short"""
    import map_side as ms

    parts = _parts(74)
    data, offs = np.frombuffer(b"".join(parts), np.uint8), _offs(parts)
    far = _far(k, "src", "slots", "dst", "data")
    for codec, algo in ((1, 1), (2, 2)):
        img, idx, sums = oracle.compress_map_output(codec, algo, data, offs)
        st, got, gi, gs = ms.compress_map_output(parts, algo, img.size, codec=codec, far=far)
        assert st == 0 and got == img.tobytes() and gi == list(idx) and gs == [int(x) for x in sums], (codec, algo)
    st, got, gi, _ = ms.compress_map_output(parts, 0, img.size - 1, codec=2, far=far)
    assert st == -2 and gi == list(idx)


@pytest.mark.parametrize("k", KS[1:2] + KS[2:], ids=["K2e32-100", "K2e32+2e31+12345"])
def test_far_snappy_multi_fragment_chunk(oracle, k):
    """a Snappy chunk above one 64 KiB fragment (head item + fragment items: the gather reads item_off[] of the fragments
    behind the head) with every pointer shifted; K = 0 is tests/test_isa_snappy_big_blocks.py"""
    import snappy_big_blocks as sbb

    rng = np.random.default_rng(75)
    parts = [corpus.chunk_corpus(7, 70_000, rng).tobytes(), b"", corpus.chunk_corpus(0, 900, rng).tobytes()]
    img, idx, _ = oracle.compress_map_output(2, 0, np.frombuffer(b"".join(parts), np.uint8), _offs(parts), 100_000)
    st, got, gi = sbb.compress_map_output(parts, 100_000, img.size, far=_far(k, "src", "slots", "dst"))
    assert st == 0 and got == img.tobytes() and gi == list(idx)
    st, _, _ = sbb.compress_map_output(parts, 100_000, img.size - 1, far=_far(k, "src", "slots", "dst"))
    assert st == -2


@FAR
def test_far_batched_map_side_call(oracle, k):
    """the TaskTail form: TaskTail.dst / dst_capacity (gather) and TaskTail.data / data_len (checksum segments) shifted, the
    scanned item_off[] and index[] patched by + K between the launches; LZ4 with checksums, Snappy without"""
    import map_side as ms
    import snappy_big_blocks as sbb

    p = _parts(76)
    tasks = [p[:3], [p[6]], [b"", b""], p[3:6]]
    far = _far(k, "src", "slots", "dst", "data")
    want = []
    for parts in tasks:
        want.append(oracle.compress_map_output(1, 2, np.frombuffer(b"".join(parts), np.uint8), _offs(parts)))
    res = ms.compress_map_outputs_batch(tasks, 2, [w[0].size for w in want], far=far)
    for (st, img, idx, sums), (wimg, widx, wsums) in zip(res, want):
        assert st == 0 and img == wimg.tobytes() and idx == [int(x) for x in widx] and sums == [int(x) for x in wsums]
    caps = [w[0].size for w in want]
    caps[3] -= 1
    res = ms.compress_map_outputs_batch(tasks, 0, caps, far=far)
    assert [r[0] for r in res] == [0, 0, 0, -2] and res[0][1] == want[0][0].tobytes()
    want = [oracle.compress_map_output(2, 0, np.frombuffer(b"".join(parts), np.uint8), _offs(parts)) for parts in tasks[:2]]
    res = sbb.compress_map_outputs_batch(tasks[:2], 32768, [w[0].size for w in want], far=_far(k, "src", "slots", "dst"))
    for (st, img, idx), (wimg, widx, _) in zip(res, want):
        assert st == 0 and img == wimg.tobytes() and idx == [int(x) for x in widx]


@pytest.mark.parametrize("k", KS, ids=["K2e31-100", "K2e32-100", "K2e32+2e31+12345"])
def test_far_lz4_blocks_above_64k(k):
    """lz4_compress_u32_kernel on one chunk of 65 547 bytes against liblz4 (K = 0: tests/test_isa_lz4_big_blocks.py); at one K the
    whole map-side call at a 131 072-byte block size, which adds xxh32_items_wave_kernel and the gather of a byU32 item"""
    import lz4_big_blocks as bb
    import lz4_u32_ref as R

    rng = np.random.default_rng(77)
    chunk = np.concatenate([corpus.chunk_corpus(7, 12_000, rng), np.zeros(bb.U32_FROM - 14_000, np.uint8), corpus.chunk_corpus(0, 2000, rng)])
    assert chunk.size == bb.U32_FROM
    (payload, hdr, _), = bb.compress_chunks_u32([chunk], far=_far(k, "src", "slots"))
    assert payload == R.liblz4_block(chunk)
    if k == KS[1]:
        parts = [chunk.tobytes(), b"", corpus.chunk_corpus(6, 700, rng).tobytes()]
        img, idx, sums = R.expected_map_output([np.frombuffer(p, np.uint8) for p in parts], 131_072, 1)
        st, got, gi, gs = bb.compress_map_output(parts, 1, len(img), 131_072, far=_far(k, "src", "slots", "dst"))
        assert st == 0 and got == img and gi == idx and gs == sums


def _launch(src, needle, mem, kernarg, grid, **kw):
    import gfx950_emu as emu
    import map_side as ms

    prog, entry, objs = ms._prog(src, needle)
    emu.launch(prog, entry, mem, kernarg, grid, 0, objects=objs, **kw)


def test_scan_items_running_sum_passes_2_31_and_2_32():
    """scan_items_kernel and scan_items_batch_kernel on a synthetic item_size[] (up to 32 MiB + 21 per item, the largest frame;
    bit 31 = stored RAW set on a third) whose running sum passes 2^31 and 2^32 inside the first 256-item tile and again
    across the following tiles, against numpy's int64 cumulative sum"""
    import gfx950_emu as emu

    rng = np.random.default_rng(78)
    n = 700  # three tiles of 256 items, the last one ragged
    size = rng.integers(1 << 24, (1 << 25) + 22, n).astype(np.uint32)
    size[rng.random(n) < 0.1] = 21
    want = np.concatenate([[0], np.cumsum(size.astype(np.int64))])
    assert want[40] < (1 << 31) < want[128] < (1 << 32) < want[255] and want[-1] > 3 * (1 << 32)
    stored = size | np.where(rng.random(n) < 0.33, 0x80000000, 0).astype(np.uint32)
    pf = np.array([0, 0, 120, 121, 256, 300, 300, 699, 700, 700], np.int32)
    mem = emu.Memory()
    off, index = np.full(n + 1, -7, np.int64), np.full(pf.size, -7, np.int64)
    a_size, a_off = mem.map(stored, "item_size", writable=False), mem.map(off, "item_off")
    a_pf, a_index = mem.map(pf, "part_first", writable=False), mem.map(index, "index")
    _launch("assemble.hip", "scan_items_kernel", mem, struct.pack("<QiiQQiiQ", a_size, n, 0, a_off, a_pf, pf.size - 1, 0, a_index), 1)
    assert np.array_equal(off, want) and np.array_equal(index, want[pf])
    # two tasks of 300 and 400 items through their TaskTail records (item_off holds one extra entry per task)
    mem = emu.Memory()
    off, index = np.full(n + 2, -7, np.int64), np.full(7, -7, np.int64)
    pf2 = np.array([0, 128, 300, 0, 1, 256, 400], np.int32)  # task 0: 2 partitions, task 1: 3 (packed, n + 1 each)
    tails = struct.pack("<iiiiiiiiQqQq", 0, 300, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0) + struct.pack("<iiiiiiiiQqQq", 300, 400, 3, 3, 2, 0, 0, 0, 0, 0, 0, 0)
    a_size, a_off = mem.map(stored, "item_size", writable=False), mem.map(off, "item_off")
    a_pf, a_index = mem.map(pf2, "part_first", writable=False), mem.map(index, "index")
    a_tails = mem.map(np.frombuffer(tails, np.uint8), "tails", writable=False)
    _launch("assemble.hip", "scan_items_batch_kernel", mem, struct.pack("<QiiQQQQ", a_tails, 2, 0, a_size, a_off, a_pf, a_index), 2)
    w0 = np.concatenate([[0], np.cumsum(size[:300].astype(np.int64))])
    w1 = np.concatenate([[0], np.cumsum(size[300:].astype(np.int64))])
    assert w0[-1] > (1 << 32) and w1[-1] > (1 << 32)
    assert np.array_equal(off[:301], w0) and np.array_equal(off[301:], w1)
    assert index.tolist() == [int(w0[0]), int(w0[128]), int(w0[300]), int(w1[0]), int(w1[1]), int(w1[256]), int(w1[400])]


def test_scan_u32_running_sum_passes_2_31_and_2_32():
    """scan_u32_kernel (frame counts -> frame_base, decoded sizes -> frame_out[]) on decoded sizes of up to 32 MiB per frame"""
    import discover_kernel as dsc
    import gfx950_emu as emu

    rng = np.random.default_rng(79)
    n = 600
    v = rng.integers(1 << 23, (1 << 25) + 1, n).astype(np.uint32)
    want = np.concatenate([[0], np.cumsum(v.astype(np.int64))])
    assert want[255] > (1 << 32) > want[100] and want[-1] > 2 * (1 << 32)
    mem = emu.Memory()
    out = np.full(n + 1, -7, np.int64)
    a_in, a_out = mem.map(v, "in", writable=False), mem.map(out, "out")
    dsc._launch("scan_u32_kernel", mem, struct.pack("<QqQ", a_in, n, a_out), 1)
    assert np.array_equal(out, want)


# ---- A.2: far offsets, checksums -----------------------------------------------------------------------------------------------
def _sum(algo, oracle, b):
    if algo == 1:
        return zlib.adler32(b)
    if algo == 2:
        return zlib.crc32(b)
    return oracle.crc32c(np.frombuffer(b, np.uint8)) if len(b) else 0


@FAR
@pytest.mark.parametrize("algo", [1, 2, 3], ids=["adler32", "crc32", "crc32c"])
def test_far_checksum_ranges(oracle, algo, k):
    """offsets[] with data and data_len: segments, fold (groups of 2 segments), combine; ranges that start in front of and end
    behind the crossing, an empty one, several segments; and offsets behind data_len are not followed"""
    import checksum_kernel as ck

    data = np.random.default_rng(80 + algo).integers(0, 256, 60_000, dtype=np.uint8).tobytes()
    offs = [0, 37, 37, 101, 16384 + 100, 16384 * 3 + 99, 60_000]
    want = [_sum(algo, oracle, data[a:b]) for a, b in zip(offs, offs[1:])]
    assert ck.checksum_ranges(algo, data, offs, far=k) == want
    assert ck.checksum_ranges(algo, data, offs, fold_group=2, far=k) == want
    got = ck.checksum_ranges(algo, data[:30_000], [0, 20_000, 30_000, 50_000, 60_000], data_len=30_000, far=k)
    assert got[:2] == [_sum(algo, oracle, data[:20_000]), _sum(algo, oracle, data[20_000:30_000])]


def _x8n(n, poly):
    """x^(8 n) mod P, reflected representation, square and multiply on Python integers"""
    import checksum_kernel as ck

    r, base, e = 0x80000000, 0x40000000, 8 * n
    while e:
        if e & 1:
            r = ck._mul(r, base, poly)
        base = ck._mul(base, base, poly)
        e >>= 1
    return r


def _fold_reference(algo, parts, span, poly):
    """the combine identities of checksum.hip's header on Python integers: parts = [(A | crc, B, bytes)] of consecutive
    pieces, span = the bytes they cover together -> (A | crc, B) of the whole, relative to its end"""
    import checksum_kernel as ck

    end, a, b, c = 0, 0, 0, 0
    for v, vb, ln in parts:
        end += ln
        after = span - end
        a += v % 65521
        b += vb % 65521 + (v % 65521) * after
        c ^= ck._mul(v, _x8n(after, poly), poly)
    return (a % 65521, b % 65521) if algo == 1 else (c, 0)


@pytest.mark.parametrize("algo", [1, 2, 3], ids=["adler32", "crc32", "crc32c"])
def test_checksum_fold_and_combine_of_a_range_above_2_32(algo):
    """`plen` itself above 2^32 for the fold / combine arithmetic alone: hand-built partials of a synthetic range of
    2^32 + 16 385 + 7 bytes (262 146 segments, 1 025 groups of 256 — the product's folded form) that starts at 2^31 - 100.
    checksum_fold_kernel on the first, a middle and the last group, then checksum_combine_kernel over hand-built group
    partials, against the same partials folded with the adler32_combine / crc32_combine identities in Python integers."""
    import checksum_kernel as ck
    import gfx950_emu as emu

    SEG, G = ck.SEG, 256
    plen = (1 << 32) + 16385 + 7
    nseg = (plen + SEG - 1) // SEG
    groups = (nseg + G - 1) // G
    assert (nseg, groups) == (262146, 1025)
    poly = 0x82F63B78 if algo == 3 else 0xEDB88320
    kalgo = 1 if algo == 1 else 2
    rng = np.random.default_rng(90 + algo)
    part = rng.integers(0, 1 << 32, (nseg, 4), dtype=np.uint64).astype(np.uint32)
    if algo == 1:
        part[:, :2] %= 65521
    part[:, 2], part[:, 3] = SEG, 0
    part[-1, 2] = plen - (nseg - 1) * SEG
    part2 = rng.integers(0, 1 << 32, (groups, 4), dtype=np.uint64).astype(np.uint32)
    if algo == 1:
        part2[:, :2] %= 65521
    part2[:, 2], part2[:, 3] = G * SEG, 0
    part2[-1, 2] = plen - (groups - 1) * G * SEG
    offs = np.array([(1 << 31) - 100, (1 << 31) - 100 + plen], np.int64)
    mem = emu.Memory()
    a_off, a_seg = mem.map(offs, "offsets", writable=False), mem.map(np.array([0, nseg], np.int32), "seg_start", writable=False)
    a_tab = mem.map(ck.tables(poly), "tables", writable=False)
    a_par = mem.map(part.reshape(-1), "partial", writable=False)
    folded = np.full((groups, 4), 0xDEADBEEF, np.uint32)
    a_fold = mem.map(folded.reshape(-1), "partial2")
    out = np.full(1, -1, np.int64)
    a_out = mem.map(out, "out")
    prog, entry = ck._program("checksum_fold_kernelILi%dE" % kalgo)
    picked = [0, 517, groups - 1]
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQii", a_off, 1, 0, a_seg, a_tab, a_par, a_fold, G, groups), picked, 0,
               objects=ck._PROG["objs"])
    for g in picked:
        rows = part[g * G:(g + 1) * G]
        span = int(rows[:, 2].astype(np.int64).sum())
        want = _fold_reference(algo, [(int(r[0]), int(r[1]), int(r[2])) for r in rows], span, poly)
        assert (int(folded[g, 0]), int(folded[g, 1]) if algo == 1 else 0) == want and int(folded[g, 2]) == span, g
    assert (folded[1] == 0xDEADBEEF).all()
    a_par2 = mem.map(part2.reshape(-1), "group_partials", writable=False)
    prog, entry = ck._program("checksum_combine_kernelILi%dE" % kalgo)
    emu.launch(prog, entry, mem, struct.pack("<QiiQQQQqii", a_off, 1, 0, a_seg, a_tab, a_par2, a_out, G * SEG, groups, 0), 1, 0,
               objects=ck._PROG["objs"])
    v, vb = _fold_reference(algo, [(int(r[0]), int(r[1]), int(r[2])) for r in part2], plen, poly)
    want = (((plen + vb) % 65521) << 16 | (1 + v) % 65521) if algo == 1 else v
    assert int(out[0]) == want


# ---- A.2: far offsets, reduce side ---------------------------------------------------------------------------------------------
def _lz4_blocks(oracle, chunks):
    out, methods = [], []
    for c in chunks:
        pay = bytes(oracle.lz4_compress_block(c))
        raw = len(pay) >= len(c)
        out.append((c.tobytes() if raw else pay, len(c)))
        methods.append(0x10 if raw else 0x20)
    return out, methods


@FAR
def test_far_batch_decoder(oracle, k):
    """Frame.comp_off with d_comp and frame_out[] with d_dst: batch_decode_kernel for LZ4 (a stored frame among them),
    Snappy and LZF"""
    import decode_kernel as dk

    chunks = _chunks(81)
    far = _far(k, "comp", "dst")
    blocks, methods = _lz4_blocks(oracle, chunks)
    assert 0x10 in methods and 0x20 in methods
    res, st, _ = dk.decode_blocks(blocks, fmt=0, methods=methods, far=far)
    assert st == 0 and res == [c.tobytes() for c in chunks]
    res, st, _ = dk.decode_blocks([(bytes(oracle.snappy_compress_block(c)), len(c)) for c in chunks], fmt=1, far=far)
    assert st == 0 and res == [c.tobytes() for c in chunks]
    lzf = [(bytes(oracle.lzf_compress_block(c)), len(c)) for c in (chunks[0], chunks[2], chunks[3])]
    res, st, _ = dk.decode_blocks(lzf, fmt=2, methods=[2] * 3, far=far)
    assert st == 0 and res == [chunks[0].tobytes(), chunks[2].tobytes(), chunks[3].tobytes()]


@FAR
def test_far_ring_decoders(oracle, k):
    """the ring decoders (decode variant 3; LZ4 verifies the frame check itself)"""
    import decode_kernel as dk

    chunks = _chunks(82)
    far = _far(k, "comp", "dst")
    blocks, methods = _lz4_blocks(oracle, chunks)
    checks = [oracle.xxh32(c) & 0x0FFFFFFF for c in chunks]
    res, st, _ = dk.decode_blocks(blocks, fmt=0, methods=methods, kernel="ring", checks=checks, far=far)
    assert st == 0 and res == [c.tobytes() for c in chunks]
    res, st, _ = dk.decode_blocks([(bytes(oracle.snappy_compress_block(c)), len(c)) for c in chunks], fmt=1, kernel="ring", far=far)
    assert st == 0 and res == [c.tobytes() for c in chunks]


@FAR
def test_far_reduce_side_ranges(oracle, k):
    """whole fetched ranges: the frame records of the compiled discovery, decoded with shifted pointers and checked by
    lz4_verify_frames_kernel (frame_out[] with d_dst); the Snappy / LZF chunk walk with part_offsets[] + K and d_comp - K
    (snappy_count_kernel / snappy_emit_kernel write Frame.comp_off + K)"""
    import decode_kernel as dk
    import discover_kernel as dsc

    parts = _parts(83)
    data, offs = np.frombuffer(b"".join(parts), np.uint8), _offs(parts)
    far = _far(k, "comp", "dst")
    img, idx, _ = oracle.compress_map_output(1, 0, data, offs)
    st, recs, outs = dsc.discover(img.tobytes())
    assert st == 0 and outs[-1] == data.size
    st, back = dk.decode_range(img.tobytes(), recs, outs, far=far)
    assert st == 0 and back == data.tobytes()
    bad = bytearray(img.tobytes())
    victim = next(r for r in recs if r[4] == 0x20 and r[1] > 100)
    bad[victim[0] + 40] ^= 0x04
    st, _ = dk.decode_range(bytes(bad), recs, outs, far=far)
    assert st == -3  # (the frame check, at the shifted offsets)
    for codec, cf, fmt in ((2, 0, 1), (4, 1, 2)):
        img, idx, _ = oracle.compress_map_output(codec, 0, data, offs)
        plain = dsc.discover_snappy(img.tobytes(), idx, chunk_format=cf)
        st, recs, outs = dsc.discover_snappy(img.tobytes(), idx, chunk_format=cf, far=k)
        assert st == 0 and (st, recs, outs) == plain and outs[-1] == data.size
        st, back = dk.decode_range(img.tobytes(), recs, outs, fmt=fmt, far=far)
        assert st == 0 and back == data.tobytes()
        assert dsc.discover_snappy(img.tobytes()[:-1], list(idx[:-1]) + [int(idx[-1]) - 1], chunk_format=cf, far=k)[0] == -3


def _zstd_parts():
    from oracle import zstd_ref
    from s3shuffle import datagen

    tera, _ = datagen.terasort_map_output(1 << 20, 10, seed=3)
    rng = np.random.default_rng(84)
    pieces = [tera[:5000], rng.integers(0, 256, 1500).astype(np.uint8), np.zeros(3000, np.uint8)]
    return [(bytes(zstd_ref.compress_stream(p, level=1)), p.size) for p in pieces], [p.tobytes() for p in pieces]


@pytest.mark.parametrize("how", ["K2e31-100", "K2e32-100", "K2e32+2e31+12345", "cross-first-window", "cross-interior", "cross-tail"])
def test_far_and_crossings_zstd(how):
    """zstd_partitions_kernel: the partitions carry absolute pointers; the 64-bit offset it adds is ZPart.lit_off to the literal
    scratch (far), and its source, destination and scratch each get a 4 GiB crossing"""
    import zstd_kernel as zk

    parts, want = _zstd_parts()
    comp_len, dst_len = sum(len(p) for p, _ in parts), sum(n for _, n in parts)
    if how.startswith("K"):
        kw = dict(far=KS[["K2e31-100", "K2e32-100", "K2e32+2e31+12345"].index(how)])
    else:
        at = {"cross-first-window": (30, 30, 30), "cross-interior": (comp_len // 2, dst_len // 2, 1000),
              "cross-tail": (comp_len - 7, dst_len - 7, 64)}[how]
        kw = dict(cross={"comp": at[0], "dst": at[1], "lit": at[2]})
    out, rcs, _ = zk.decode_partitions(parts, **kw)
    assert rcs == [0] * len(parts) and out == want


# ---- A.4: 4 GiB address crossings ----------------------------------------------------------------------------------------------
WHERE = pytest.mark.parametrize("where", ["first-window", "interior", "tail"])


def _at(where, start, length, size):
    """a byte (a) inside the first 64-byte window of the chunk at `start`, (b) in its interior, (c) within the region's last 16"""
    return {"first-window": start + 30, "interior": start + length // 2, "tail": size - 7}[where]


@WHERE
def test_crossings_lz4_and_snappy_chunks(oracle, where):
    import lz4_kernel as lk
    import snappy_kernel as sk

    chunks = _chunks(85)
    total = sum(c.size for c in chunks)
    second = chunks[0].size
    stride = lk.K_SLOT_BYTES
    cross = {"src": _at(where, second, chunks[1].size, total), "slots": _at(where, stride + 32, 1500, 4 * stride - 20000)}
    for windows in (True, False):
        for c, (payload, hdr, _) in zip(chunks, lk.compress_chunks(chunks, windows=windows, cross=cross)):
            ref = oracle.lz4_compress_block(c)
            assert hdr[:8] == b"LZ4Block" and ((payload is None and len(ref) >= len(c)) or np.array_equal(payload, ref))
    cross["src"] = _at(where, 0, chunks[0].size, total)
    sstride = (32 + 32768 + 32768 // 6 + 64 + 15) & ~15
    cross["slots"] = _at(where, 32, 1000, 4 * sstride - 30000)
    for c, (slot, sz, _) in zip(chunks, sk.compress_chunks(chunks, cross=cross)):
        assert bytes(slot[32:32 + sz - 4]) == bytes(oracle.snappy_compress_block(c))


@WHERE
def test_crossings_whole_map_side_call(oracle, where):
    """source, slots and destination each mapped so that a 4 GiB-aligned address lies inside them (and the checksum kernels
    read the image across the same crossing)"""
    import map_side as ms

    parts = _parts(86)
    data, offs = np.frombuffer(b"".join(parts), np.uint8), _offs(parts)
    for codec, algo in ((1, 2), (2, 1)):
        img, idx, sums = oracle.compress_map_output(codec, algo, data, offs)
        # the stored (incompressible) partition: its chunk is read by the codec kernel AND copied by the gather
        cross = {"src": _at(where, int(offs[2]), len(parts[2]), data.size), "dst": _at(where, int(idx[2]), int(idx[3] - idx[2]), img.size),
                 "slots": _at(where, 32, 1200, 1500)}
        st, got, gi, gs = ms.compress_map_output(parts, algo, img.size, codec=codec, cross=cross)
        assert st == 0 and got == img.tobytes() and gi == list(idx) and gs == [int(x) for x in sums], (codec, algo)


def test_crossings_lz4_u32_chunk():
    """the byU32 path: source crossing in the chunk's interior, slot crossing in the frame header; the whole map-side call adds
    xxh32_items_wave_kernel and the gather"""
    import lz4_big_blocks as bb
    import lz4_u32_ref as R

    rng = np.random.default_rng(87)
    chunk = np.concatenate([corpus.chunk_corpus(7, 9_000, rng), np.zeros(bb.U32_FROM - 10_000, np.uint8), corpus.chunk_corpus(0, 1000, rng)])
    parts = [corpus.chunk_corpus(6, 500, rng).tobytes(), chunk.tobytes()]
    img, idx, sums = R.expected_map_output([np.frombuffer(p, np.uint8) for p in parts], 131_072, 2)
    cross = {"src": 500 + 4000, "slots": 32 + 131_072 + 20, "dst": idx[1] + 10}
    st, got, gi, gs = bb.compress_map_output(parts, 2, len(img), 131_072, cross=cross)
    assert st == 0 and got == img and gi == idx and gs == sums


@WHERE
def test_crossings_decoders(oracle, where):
    """compressed input and destination of the batch decoder (LZ4, Snappy), the frame-check kernel and the ring decoders"""
    import decode_kernel as dk
    import discover_kernel as dsc

    chunks = _chunks(88)
    want = [c.tobytes() for c in chunks]
    blocks, methods = _lz4_blocks(oracle, chunks)
    checks = [oracle.xxh32(c) & 0x0FFFFFFF for c in chunks]
    comp_total, first = sum(len(p) for p, _ in blocks), len(blocks[0][0])
    cross = {"comp": _at(where, first, len(blocks[1][0]), comp_total), "dst": _at(where, chunks[0].size, chunks[1].size, sum(c.size for c in chunks))}
    res, st, _ = dk.decode_blocks(blocks, fmt=0, methods=methods, cross=cross)
    assert st == 0 and res == want
    res, st, _ = dk.decode_blocks(blocks, fmt=0, methods=methods, kernel="ring", checks=checks, cross=dict(cross, comp=cross["comp"] & ~3))
    assert st == 0 and res == want
    sblocks = [(bytes(oracle.snappy_compress_block(c)), len(c)) for c in chunks]
    scross = dict(cross, comp=_at(where, 0, len(sblocks[0][0]), sum(len(p) for p, _ in sblocks)))
    res, st, _ = dk.decode_blocks(sblocks, fmt=1, cross=scross)
    assert st == 0 and res == want
    res, st, _ = dk.decode_blocks(sblocks, fmt=1, kernel="ring", cross=dict(scross, comp=scross["comp"] & ~3))
    assert st == 0 and res == want
    parts = _parts(89)
    data, offs = np.frombuffer(b"".join(parts), np.uint8), _offs(parts)
    img, idx, _ = oracle.compress_map_output(1, 0, data, offs)
    st, recs, outs = dsc.discover(img.tobytes())
    st, back = dk.decode_range(img.tobytes(), recs, outs, cross={"comp": _at(where, recs[0][0], recs[0][1], img.size),
                                                                 "dst": _at(where, 0, recs[0][2], data.size)})
    assert st == 0 and back == data.tobytes()


@WHERE
def test_crossings_checksum_and_discovery(oracle, where):
    """the checksum segments, the LZ4Block tile discovery and the Snappy / LZF chunk walk with the range mapped across a 4 GiB
    boundary (the tiles are k * 65536 from the range start, so it is the range that moves)"""
    import checksum_kernel as ck
    import discover_kernel as dsc

    data = np.random.default_rng(91).integers(0, 256, 50_000, dtype=np.uint8).tobytes()
    offs = [0, 37, 16384 + 100, 50_000]
    at = _at(where, 37, 16384, 50_000)
    for algo in (1, 2, 3):
        assert ck.checksum_ranges(algo, data, offs, cross={"data": at}) == [_sum(algo, oracle, data[a:b]) for a, b in zip(offs, offs[1:])]
    rng = np.random.default_rng(92)
    src = np.concatenate([corpus.chunk_corpus(7, 40_000, rng), corpus.chunk_corpus(0, 70_000, rng), corpus.chunk_corpus(6, 3000, rng)])
    stream = oracle.compress_stream(1, src).tobytes()  # two 64 KiB tiles, the second one starts inside a stored frame
    assert 65536 < len(stream) < 2 * 65536
    want = dsc.reference_frames(stream)
    for at in {_at(where, 0, 21, len(stream)), _at(where, 65536, 2000, len(stream))}:
        st, recs, outs = dsc.discover(stream, cross={"comp": at})
        assert st == 0 and recs == want and outs[-1] == src.size
    st, _, _ = dsc.discover(stream[:-30], cross={"comp": len(stream) - 40})
    assert st == -3
    parts = _parts(93)
    pdata, poffs = np.frombuffer(b"".join(parts), np.uint8), _offs(parts)
    for codec, cf in ((2, 0), (4, 1)):
        img, idx, _ = oracle.compress_map_output(codec, 0, pdata, poffs)
        plain = dsc.discover_snappy(img.tobytes(), idx, chunk_format=cf)
        assert plain[0] == 0
        assert dsc.discover_snappy(img.tobytes(), idx, chunk_format=cf, cross={"comp": _at(where, int(idx[2]), 16, img.size)}) == plain


@WHERE
def test_crossings_batched_calls(oracle, where):
    """the batched forms: every task's destination (TaskTail.dst / .data) and the shared source and slots of a batched
    map-side call; a range's compressed bytes and destination in the batched reduce-side call (LzRange.comp / dst_base, the
    absolute addresses frames_finish_batch_kernel writes)"""
    import discover_kernel as dsc
    import map_side as ms

    p = _parts(94)
    tasks = [p[:3], [p[6]], p[3:6]]
    want = [oracle.compress_map_output(1, 1, np.frombuffer(b"".join(t), np.uint8), _offs(t)) for t in tasks]
    total = sum(len(b"".join(t)) for t in tasks)
    cross = {"src": _at(where, len(p[0]), len(p[2]), total), "slots": _at(where, 32, 1200, 1500),
             "dst0": _at(where, 0, 21, want[0][0].size), "dst2": _at(where, 21, 500, want[2][0].size)}
    res = ms.compress_map_outputs_batch(tasks, 1, [w[0].size for w in want], cross=cross)
    for (st, img, idx, sums), (wimg, widx, wsums) in zip(res, want):
        assert st == 0 and img == wimg.tobytes() and idx == [int(x) for x in widx] and sums == [int(x) for x in wsums]
    rng = np.random.default_rng(95)
    srcs = [np.concatenate([corpus.chunk_corpus(7, 40_000, rng), corpus.chunk_corpus(0, 70_000, rng)]).tobytes(),
            corpus.chunk_corpus(6, 3000, rng).tobytes()]
    streams = [oracle.compress_stream(1, np.frombuffer(b, np.uint8)).tobytes() for b in srcs]
    assert len(streams[0]) > 65536 + 4000  # (two tiles)
    cross = {"comp0": _at(where, 65536, 2000, len(streams[0])), "dst0": _at(where, 32768, 7232, len(srcs[0])),
             "comp1": _at(where, 0, 21, len(streams[1])), "dst1": _at(where, 0, 3000, len(srcs[1]))}
    res, dec_status = dsc.decode_ranges_batch(streams, [len(b) for b in srcs], cross=cross)
    assert dec_status == 0 and [st for st, _ in res] == [0, 0] and [out for _, out in res] == srcs
