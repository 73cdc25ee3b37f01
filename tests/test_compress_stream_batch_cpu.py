"""CPU: the batched feed of the streaming map side (s3s_cstream_feed_batch*) as far as it goes without a GPU.

Surface: the header declares the symbols, the entry struct and the read-only key 18 with the ABI still 11, the cross-compiled
library exports them, the binding's structure has the C compiler's size, a null context is answered before any device work.
Host arithmetic: csrc/compress_stream_batch_core.h as a stand-alone program under AddressSanitizer and UBSan
(tests/model/cstream_batch_model.cpp) with the kernels played over a pipe (tests/cstream_batch_lib.py), on random rounds of
2 - 9 streams against tests/cstream_units.Model; one-token mutants of the header must each fail.
Compiled kernels: cstream_cut_batch_kernel and gather_items_cut_batch_kernel in the gfx950 interpreter
(tests/isa/cstream_batch_kernel.py), three windows in one launch, against the model and the single cut kernel."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cstream_batch_lib as cb
import cstream_units as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
SYMBOLS = ["s3s_cstream_feed_batch_device", "s3s_cstream_feed_batch"]


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols(codec_lib):
    header = open(HEADER).read()
    import s3shuffle
    from s3shuffle import codec

    exported = subprocess.run(["nm", "-D", "--defined-only", s3shuffle.library_path()], check=True, capture_output=True, text=True).stdout
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert re.search(r"\bT %s\b" % sym, exported), sym
        assert getattr(codec_lib, sym).argtypes, sym
    assert "typedef struct s3s_cstream_feed_entry" in header
    assert int(re.search(r"S3S_OPT_CSTREAM_BATCH_ENTRIES\s*=\s*\((\d+)\)", header).group(1)) == 18 == codec.OPT_CSTREAM_BATCH_ENTRIES
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()
    # the section stands behind the batched reduce-side feed, not inside the "map side, streaming" section
    assert header.index("typedef struct s3s_dstream_feed_entry") < header.index("the batched feed of s3s_cstream") < header.index("typedef struct s3s_cstream_feed_entry")
    section = header[header.index("the batched feed of s3s_cstream"):header.index("typedef struct s3s_cstream_feed_entry")]
    for needle in ("would have produced for that stream alone", "nothing written at or beyond out_len", "S3S_STATUS_NOT_RUN", "the same stream twice",
                   "do not overlap", "same block size and the same LZ4 / Snappy variant", "ONE host", "S3S_E_HIP", "sliced in", "Key 18",
                   "the sum of the windows", "ONE encrypt pass", "S3S_CODEC_NONE", "Zstandard"):
        assert needle in section, needle


def test_python_binding_shapes(tmp_path):
    import s3shuffle
    from s3shuffle import codec

    assert [f[0] for f in codec.CompressFeedEntry._fields_] == ["stream", "d_src", "src_len", "part_ends", "n_ends", "status", "d_dst",
                                                                 "dst_capacity", "out_lengths", "out_checksums", "result"]
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "s3shuffle_codec.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                    'sizeof(s3s_cstream_feed_entry), offsetof(s3s_cstream_feed_entry, status), offsetof(s3s_cstream_feed_entry, result)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe], check=True)
    size, off_status, off_result = (int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(codec.CompressFeedEntry) == size == 112
    assert (codec.CompressFeedEntry.status.offset, codec.CompressFeedEntry.result.offset) == (off_status, off_result)
    for m in ("compress_stream_feed_batch", "compress_stream_feed_batch_host", "compress_batch_entries"):
        assert hasattr(s3shuffle.Codec, m), m
    assert s3shuffle.CompressFeedEntry is codec.CompressFeedEntry


def test_a_null_context_is_answered_before_any_device_work(codec_lib):
    from s3shuffle import codec

    arr = (codec.CompressFeedEntry * 2)()
    for e in arr:
        e.status = 5
    assert codec_lib.s3s_cstream_feed_batch_device(None, arr, 2) == -1
    assert codec_lib.s3s_cstream_feed_batch(None, arr, 2) == -1
    assert codec_lib.s3s_get_option(None, codec.OPT_CSTREAM_BATCH_ENTRIES) == -1
    assert codec_lib.s3s_set_option(None, codec.OPT_CSTREAM_BATCH_ENTRIES, 1) == -1
    assert [e.status for e in arr] == [5, 5]  # without a context nothing is touched


def test_the_core_header_builds_without_hip_and_allocates_nothing(tmp_path):
    text = open(cb.CORE).read()
    code = "\n".join(line.split("//")[0] for line in text.split("\n"))
    includes = [line.split()[1] for line in code.split("\n") if line.startswith("#include")]
    assert sorted(includes) == ['"compress_stream_core.h"', "<stddef.h>", "<stdint.h>"]
    for word in ("s3s_ctx", "hip", "fail(", "new ", "malloc", "std::vector"):
        assert word not in code, word
    unit = tmp_path / "unit.cpp"
    unit.write_text('#include "compress_stream_batch_core.h"\nint main() { s3s_cs::Totals t; return (int)t.pp(); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cb.CSRC, str(unit), "-o", str(tmp_path / "unit")], check=True)


# ---- host arithmetic against the Python model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    return cb.build(tmp_path_factory.mktemp("cstream_batch"))


CASES = [(cu.LZ4, 64, cb.ADLER, 6), (cu.LZ4, 64, 0, 3), (cu.SNAPPY, 1024, cb.CRC, 6), (cu.LZF, 65535, cb.ADLER, 2)]


@pytest.mark.parametrize("codec,bs,algo,runs", CASES, ids=["lz4-adler", "lz4-nosum", "snappy-crc", "lzf-adler"])
def test_host_arithmetic_against_the_python_model(oracle, model_exe, tmp_path, codec, bs, algo, runs):
    rng = np.random.default_rng(7 * codec + algo)
    batched = refused = hosted = 0
    for run in range(runs):
        n_streams = int(rng.integers(2, 4)) if codec == cu.LZF else [2, 9, 5, 3, 7, 4][run % 6]
        _, b, r, h = cb.run_rounds(oracle, model_exe, tmp_path, codec, bs, algo, seed=1000 * codec + run, n_streams=n_streams)
        batched, refused, hosted = batched + b, refused + r, hosted + h
    # the rounds held healthy windows, refused entries and entries that launch nothing, next to each other
    assert batched >= 5 * runs and refused > 0 and hosted > 0, (batched, refused, hosted)


MUTANTS = [
    ("seeds[c.first_piece + j] = j == 0 ? carry : fresh;", "seeds[c.first_piece + j] = j == 1 ? carry : fresh;"),  # the seed of a non-first piece
    ("return (src_addr - base_addr) + unit_off;", "return (base_addr - src_addr) + unit_off;"),                  # the delta's sign
    ("c.first_pp = (int32_t)t->pp();", "c.first_pp = (int32_t)t->pieces;"),                                      # the entry-relative piece index
    ("c.first_len = (int32_t)t->lens();", "c.first_len = (int32_t)t->pieces;"),
    ("emit(u, c->first_item + it, slot);", "emit(u, it, slot);"),                                                # items of the call, not of the entry
    ("Mark* m = marks + c->first_item;", "Mark* m = marks;"),
    ("*carry = sums[c.parts_closed];", "*carry = sums[0];"),                                                     # the open partition's state
    ("len = arena_al(piece + 8 * PP);", "len = arena_al(piece + 8 * P);"),                                       # n + 1 offsets an entry
    ("piece_entry[c.first_piece + j] = entry;", "piece_entry[c.first_piece + j] = entry + 1;"),
    ("if (it == 0) c->ends0 = u.ends_before;", "if (it == 0) c->ends0 = 0;"),
    # the rules both feeds share: the window that launches nothing, the take step, the first piece's seed
    ("if (n_ends == 0) c.need_src = need_src_unit;", "if (n_ends != 0) c.need_src = need_src_unit;"),
    ("c.parts_closed = n_ends;", "c.parts_closed = 0;"),
    ("if (c.need_dst > 0) {", "if (c.need_dst < 0) {"),                                                           # need_dst, and the stream moves all the same
    ("seeds[c.first_piece + j] = j == 0 ? carry : fresh;", "seeds[c.first_piece + j] = j < 0 ? carry : fresh;"),   # fresh for the first piece too
    ("return n.items == 0 || n.items > kBatchMax", "return n.items != 0 || n.items > kBatchMax"),                   # which entries are windows
]


@pytest.mark.parametrize("old,new", MUTANTS, ids=[str(i) for i in range(len(MUTANTS))])
def test_one_token_mutants_of_the_header_fail(oracle, tmp_path, old, new):
    text = open(cb.CORE).read()
    assert text.count(old) == 1, old
    inc = tmp_path / "inc"
    inc.mkdir()
    (inc / "compress_stream_batch_core.h").write_text(text.replace(old, new))
    (inc / "compress_stream_core.h").write_text(open(os.path.join(cb.CSRC, "compress_stream_core.h")).read())
    exe = cb.build(tmp_path, include_dir=str(inc))
    with pytest.raises(AssertionError):
        for run in range(3):
            cb.run_rounds(oracle, exe, tmp_path, cu.LZ4, 64, cb.ADLER, seed=1000 * cu.LZ4 + run, n_streams=[2, 9, 5][run])


# ---- the compiled kernels through the gfx950 interpreter --------------------------------------------------------------------
def _window(rng, n_blocks_per_part, tail_blocks, block):
    def blob(n):
        b = np.resize(np.frombuffer(b"abcdabcdabcdabce0123", np.uint8), n).copy()
        b[n // 3:2 * n // 3] = rng.integers(0, 256, 2 * n // 3 - n // 3, dtype=np.uint8)
        return b.tobytes()
    return [blob(n * block - (7 if n else 0)) for n in n_blocks_per_part], blob(tail_blocks * block)


def test_cut_batch_and_cut_gather_batch_in_the_interpreter(oracle):
    """Three windows in one launch at block size 64 (the smallest key 1 accepts) with 1, 256 and 257 plan items.  Window 0 (one
    block of an open partition) answers need_dst; window 1 (partitions of 100 blocks, 0 bytes and 154 blocks: 256 items, ONE
    256-item tile) is cut in the middle of that tile, inside its third partition; window 2 (one partition of 256 blocks:
    257 items, the end frame alone in the second tile) takes everything.  Window 2's source lies below window 0's."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "isa"))
    import cstream_batch_kernel as bk

    block = 64
    rng = np.random.default_rng(11)
    shapes = [([], 1), ([100, 0, 154], 0), ([256], 0)]
    wins = [_window(rng, parts, tail, block) for parts, tail in shapes]
    models, images = [], []
    for parts, tail in wins:
        data = np.frombuffer(b"".join(parts) + tail, np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(p) for p in parts] + [len(tail)])]).astype(np.int64)
        img, index, _ = oracle.compress_map_output(cu.LZ4, 0, data, offs, block_size=block)
        img = np.asarray(img).tobytes()
        models.append(cu.Model(cu.LZ4, block, cu.unit_sizes_from_image(cu.LZ4, img, index)))
        images.append((img, [int(x) for x in index]))
    flat1 = [x for p in models[1].sizes for x in p]
    caps = [models[0].sizes[0][0] - 1, sum(flat1[:128]) + 9, len(images[2][0])]
    entries = [dict(parts=parts, tail=tail, cap=cap) for (parts, tail), cap in zip(wins, caps)]
    got = bk.feed_batch_lz4(entries, block, src_order=[2, 0, 1])
    assert [g["n_items"] for g in got] == [1, 256, 257]
    for i, (g, mo, (img, index)) in enumerate(zip(got, models, images)):
        want = mo.feed(g["src_len"], g["ends"], caps[i])
        assert g["status"] == 0
        assert g["words"][:5] == g["single"]["words"][:5] and g["piece_off"] == g["single"]["piece_off"] and g["lengths"] == g["single"]["lengths"], i
        if want.code == cu.E_CAPACITY:
            assert (g["k"], g["consumed"], g["out_len"], g["need_dst"], g["parts_closed"]) == (0, 0, 0, want.need_dst, 0)
            assert g["dst"] == b"\xa5" * caps[i]
            continue
        assert (g["consumed"], g["out_len"], g["need_dst"], g["parts_closed"]) == (want.consumed, want.out_len, 0, want.parts_closed), i
        assert g["lengths"][:want.parts_closed] == want.lengths and not any(g["lengths"][want.parts_closed:])
        # the open piece holds what the image has behind the last partition that ends in the window
        n_ends = len(g["ends"])
        assert g["piece_off"] == [min(int(x), want.out_len) for x in index[:n_ends + 1]] + [want.out_len]
        assert g["dst"] == img[:want.out_len] + b"\xa5" * (caps[i] - want.out_len), i
    assert got[0]["need_dst"] > 0 and got[1]["k"] == 128 and got[1]["parts_closed"] == 2 and got[2]["k"] == 257
