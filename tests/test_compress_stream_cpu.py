"""CPU: the streaming map side (s3s_cstream_*) as far as it goes without a GPU - the header declares the symbols and the
cross-compiled library exports them, the Python binding binds them, the ABI version did not move; the host arithmetic
(compress_stream_core.h) as a stand-alone program under the sanitizers against the Python model of the contract
(cstream_units.py) on random schedules; the compiled cut kernel and cut gather through the gfx950 interpreter."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cstream_units as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
SYMBOLS = ["s3s_cstream_open", "s3s_cstream_feed_device", "s3s_cstream_feed", "s3s_cstream_feed_bound", "s3s_cstream_position",
           "s3s_cstream_written", "s3s_cstream_close"]


# ---- header and binding --------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols(codec_lib):
    header = open(HEADER).read()
    import s3shuffle

    exported = subprocess.run(["nm", "-D", "--defined-only", s3shuffle.library_path()], check=True, capture_output=True, text=True).stdout
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert re.search(r"\bT %s\b" % sym, exported), sym
        assert getattr(codec_lib, sym).argtypes, sym  # bound by s3shuffle.codec.load_library
    assert "typedef struct s3s_cstream_result" in header
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()
    section = header[header.index("map side, streaming"):]
    for needle in ("SAME BYTES", "longest prefix of units", "need_dst is its exact image size", "end frame", "16-byte stream header",
                   "S3S_CODEC_ZSTD", "content size", "IO encryption", "not of the feeds", "host-only", "bounded memory, not speed",
                   "inside a codec stream", "S3S_OPT_LZ4_VARIANT = 9 runs 11"):
        assert needle in section, needle
    assert "streaming map side" in header


def test_the_library_still_links_only_the_hip_runtime(codec_lib):
    import s3shuffle

    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.+?)\]", subprocess.run(["readelf", "-d", s3shuffle.library_path()], check=True,
                                                                                   capture_output=True, text=True).stdout)
    system = ("libstdc++", "libm.", "libgcc_s", "libc.", "libdl", "libpthread", "librt", "ld-linux")
    assert [n for n in needed if not n.startswith(system)] == ["libamdhip64.so.%s" % n.split(".")[-1] for n in needed if n.startswith("libamdhip64")]
    assert any(n.startswith("libamdhip64") for n in needed)


def test_python_binding_shapes(tmp_path):
    import s3shuffle
    from s3shuffle import codec

    assert [f[0] for f in codec.CompressStreamResult._fields_] == ["consumed", "out_len", "need_src", "need_dst", "parts_closed", "reserved"]
    # ... and its size is the C struct's, as the host compiler lays it out
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include "s3shuffle_codec.h"\nint main(void) { printf("%zu\\n", sizeof(s3s_cstream_result)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", exe], check=True)
    assert ctypes.sizeof(codec.CompressStreamResult) == int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout) == 40
    for m in ("feed", "feed_device", "feed_bound", "position", "written", "close", "__enter__", "__exit__"):
        assert hasattr(s3shuffle.CompressStream, m), m
    assert hasattr(s3shuffle.Codec, "compress_stream") and s3shuffle.CompressStreamResult is codec.CompressStreamResult


def test_a_null_context_is_answered_before_any_device_work(codec_lib):
    h = ctypes.c_void_p(None)
    assert codec_lib.s3s_cstream_open(None, 1, 0, ctypes.byref(h)) == -1 and h.value is None
    r = s3shuffle_result()
    assert codec_lib.s3s_cstream_feed_device(None, None, 0, None, 0, None, 0, None, None, ctypes.byref(r)) == -1
    assert codec_lib.s3s_cstream_feed(None, None, 0, None, 0, None, 0, None, None, ctypes.byref(r)) == -1
    assert codec_lib.s3s_cstream_close(None) == -1
    assert codec_lib.s3s_cstream_position(None) == -1 and codec_lib.s3s_cstream_written(None) == -1
    assert codec_lib.s3s_cstream_feed_bound(None, 10, 1) == -1


def s3shuffle_result():
    from s3shuffle import codec

    return codec.CompressStreamResult()


def test_feed_refuses_a_destination_the_library_would_overrun(codec_lib):
    """CompressStream.feed hands dst's address and a capacity to the library: the capacity may not exceed the array, and the
    array must be the bytes the address names (uint8, C-contiguous, writable).  Checked before the stream is touched."""
    import s3shuffle

    s = s3shuffle.CompressStream.__new__(s3shuffle.CompressStream)
    s._s, s._ctx, s._lib, s._checksum = None, None, codec_lib, 0
    src = np.zeros(8, np.uint8)
    read_only = np.zeros(16, np.uint8)
    read_only.flags.writeable = False
    for dst, cap in ((np.zeros(16, np.uint8), 17), (np.zeros(16, np.uint8), -1), (np.zeros(32, np.uint8)[::2], None),
                     (np.zeros(4, np.int32), None), (read_only, None), (bytearray(16), None)):
        with pytest.raises(ValueError, match="dst"):
            s.feed(src, [8], dst, cap)
    with pytest.raises(ValueError, match="closed"):  # a destination that passes reaches the stream
        s.feed(src, [8], np.zeros(16, np.uint8), 16)


# ---- host arithmetic against the Python model -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cstream") / "cstream_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "model", "cstream_model.cpp"), "-o", exe], check=True)
    return exe


def _map_output(rng, bs, nparts):
    sizes = [int(rng.choice([0, 0, 1, bs - 1, bs, bs + 1, 2 * bs, int(rng.integers(1, 4 * bs))])) for _ in range(nparts)]
    total = sum(sizes)
    data = np.resize(np.frombuffer(b"abcdefgh01234567abcdefgh", np.uint8), total).copy()
    data[total // 2:] = rng.integers(0, 256, total - total // 2, dtype=np.uint8)
    return data, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _schedule(rng, model, offs, bs):
    """a random schedule run on the Python model: [(wlen, cap, ends)], [Feed]"""
    total, nparts = int(offs[-1]), len(offs) - 1
    big = max(model_max_unit(model), 1)
    feeds, answers, pos, closed = [], [], 0, 0
    while (pos < total or closed < nparts) and len(feeds) < 400:
        wlen = min(int(rng.choice([0, 1, bs - 1, bs, bs + 1, 3 * bs - 1, int(rng.integers(0, 5 * bs)), total])), total - pos)
        ends = cu.ends_in_window(offs, pos, closed, wlen)
        cap = int(rng.choice([0, 1, 20, 21, big - 1, big, big + 1, 2 * big + 5, int(rng.integers(0, 6 * big)), 1 << 40]))
        f = model.feed(wlen, ends, cap)
        feeds.append((wlen, cap, ends))
        answers.append(f)
        pos += f.consumed
        closed += f.parts_closed
    return feeds, answers


def model_max_unit(model):
    return max((x for p in model.sizes for x in p), default=1)


@pytest.mark.parametrize("codec", [cu.NONE, cu.LZ4, cu.SNAPPY, cu.LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_host_arithmetic_against_the_python_model(oracle, model_exe, codec):
    bs = {cu.NONE: 1, cu.LZ4: 64, cu.SNAPPY: 1024, cu.LZF: 65535}[codec]
    shape_bs = 64 if codec == cu.NONE else bs
    rng = np.random.default_rng(100 + codec)
    n_outputs, n_schedules = (2, 12) if codec == cu.LZF else (6, 50)
    checked = 0
    for _ in range(n_outputs):
        data, offs = _map_output(rng, shape_bs, int(rng.integers(1, 9)))
        img, index, _ = oracle.compress_map_output(codec, 0, data, offs, block_size=bs if codec in (cu.LZ4, cu.SNAPPY) else 32768)
        sizes = cu.unit_sizes_from_image(codec, np.asarray(img).tobytes(), index)
        for p in range(len(offs) - 1):  # the image has the units the contract counts
            u = int(offs[p + 1] - offs[p])
            assert len(sizes[p]) == (u if codec == cu.NONE else -(-u // bs) + (codec == cu.LZ4 and u > 0))
        head = "%d %d %d\n" % (codec, bs, len(sizes)) + "".join("%d %s\n" % (len(s), " ".join(map(str, s))) for s in sizes)
        for _ in range(n_schedules):
            feeds, answers = _schedule(rng, cu.Model(codec, bs, sizes), offs, bs)
            text = head + "".join("%d %d %d %s\n" % (w, c, len(e), " ".join(map(str, e))) for w, c, e in feeds)
            r = subprocess.run([model_exe], input=text, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
            lines = r.stdout.strip().split("\n") if feeds else []
            assert len(lines) == len(feeds)
            for line, f, feed in zip(lines, answers, feeds):
                got = [int(x) for x in line.split()]
                assert (got[0], got[1], got[2], got[3], got[4], got[5], tuple(got[6:])) == f.fields(), (feed, line, f.fields())
            checked += 1
    assert checked == n_outputs * n_schedules


# ---- the compiled cut kernel and cut gather through the gfx950 interpreter ------------------------------------------------
def test_cut_kernel_and_cut_gather_in_the_interpreter(oracle):
    """the smallest window with a capacity cut and a closed partition: LZ4 at block size 64, partitions of 70, 0 and 10 bytes
    (five units); dst has exactly dst_capacity bytes"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "isa"))
    import cstream_kernel as ckn

    rng = np.random.default_rng(5)
    parts = [bytes(np.resize(np.frombuffer(b"abcdabcdabcdabce", np.uint8), 70)), b"", rng.integers(0, 256, 10, dtype=np.uint8).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.array([0, 70, 70, 80], np.int64)
    img, index, _ = oracle.compress_map_output(cu.LZ4, 0, data, offs, block_size=64)
    img = np.asarray(img).tobytes()
    sizes = cu.unit_sizes_from_image(cu.LZ4, img, index)
    flat = [x for p in sizes for x in p]
    assert len(flat) == 5
    for cap in (len(img), sum(flat[:3]) + 5, sum(flat[:3]), sum(flat[:2]) + 20, flat[0], flat[0] - 1, 0):
        want = cu.Model(cu.LZ4, 64, sizes).feed(80, [70, 70, 80], cap)
        got = ckn.feed_lz4(parts, 64, cap)
        assert got["status"] == 0
        if want.code == cu.E_CAPACITY:
            assert (got["k"], got["consumed"], got["out_len"], got["need_dst"], got["parts_closed"]) == (0, 0, 0, want.need_dst, 0)
            assert got["dst"] == b"\xa5" * cap
            continue
        assert (got["consumed"], got["out_len"], got["need_dst"], got["parts_closed"]) == (want.consumed, want.out_len, 0, want.parts_closed), cap
        assert got["lengths"][:want.parts_closed] == want.lengths and not any(got["lengths"][want.parts_closed:])
        assert got["piece_off"] == [min(int(x), want.out_len) for x in index] + [want.out_len]
        assert got["dst"] == img[:want.out_len] + b"\xa5" * (cap - want.out_len), cap
