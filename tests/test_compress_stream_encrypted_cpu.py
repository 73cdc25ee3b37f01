"""CPU: the streaming map side under IO encryption (s3s_cstream_open_encrypted) as far as it goes without a GPU - the symbol,
the binding and the header's paragraph; the host arithmetic (compress_stream_core.h: the plan with IV records, the encrypted NONE
cut, feed_bound) as a stand-alone program under the sanitizers against the Python model of the contract
(cstream_units_encrypted.py); the ownership of aes_ctr_stream_core.h in the map-side geometry against spark_crypto_ref; the
compiled cut kernel and cut gather on a plan with IV records through the gfx950 interpreter."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import aes_ctr_model_lib as acm
import cstream_units as cu
import cstream_units_encrypted as cue
import spark_crypto_ref as scr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")


# ---- symbol, binding, header ------------------------------------------------------------------------------------------------
def test_library_exports_the_symbol_and_the_binding_takes_encrypted(codec_lib):
    import inspect

    import s3shuffle

    header = open(HEADER).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", s3shuffle.library_path()], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bs3s_cstream_open_encrypted\s*\(", header)
    assert re.search(r"\bT s3s_cstream_open_encrypted\b", exported)
    assert codec_lib.s3s_cstream_open_encrypted.argtypes == codec_lib.s3s_cstream_open.argtypes
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()
    assert inspect.signature(s3shuffle.Codec.compress_stream).parameters["encrypted"].default is False
    assert inspect.signature(s3shuffle.CompressStream.__init__).parameters["encrypted"].default is False


def test_header_carries_the_paragraph():
    header = open(HEADER).read()
    section = header[header.index("map side, streaming"):header.index("typedef struct s3s_cstream s3s_cstream;")]
    para = section[section.index("Under Spark IO encryption: s3s_cstream_open_encrypted"):]
    for needle in ("requires the layer to be on (off: S3S_E_INVALID)", "belongs to the unit of the partition's first block",
                   "IV, stream header, chunk", "17", "An empty partition stays 0 bytes", "STORED bytes", "16 * (n_ends + 1)",
                   "s3s_set_stream_ivs(ctx, ivs, n_ends + 1)", "entry 0 is ignored", "consumed either way", "and not of the feeds",
                   "can only be closed", "No key material", "wiped when the partition closes and at", "byte for byte",
                   "same options, key and IVs"):
        assert needle in para, needle
    for line in re.findall(r"\* Not here ([^\n]*(?:\n \*          [^\n]*)*)", section):
        assert "IO encryption" not in line, line
    assert "by\n *          s3s_cstream_open, any context with IO encryption on" in section  # the plain open keeps its refusal


def test_a_null_context_is_answered_before_any_device_work(codec_lib):
    import ctypes

    h = ctypes.c_void_p(None)
    assert codec_lib.s3s_cstream_open_encrypted(None, 1, 0, ctypes.byref(h)) == -1 and h.value is None


# ---- host arithmetic against the Python model -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cstream_enc") / "cstream_encrypted_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "model", "cstream_encrypted_model.cpp"), "-o", exe], check=True)
    return exe


def _map_output(rng, bs, nparts):
    sizes = [int(rng.choice([0, 0, 1, bs - 1, bs, bs + 1, 2 * bs, int(rng.integers(1, 4 * bs))])) for _ in range(nparts)]
    total = sum(sizes)
    data = np.resize(np.frombuffer(b"abcdefgh01234567abcdefgh", np.uint8), total).copy()
    data[total // 2:] = rng.integers(0, 256, total - total // 2, dtype=np.uint8)
    return data, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _schedule(rng, model, codec, offs, bs):
    """a random schedule run on the Python model: [(wlen, cap, ends)], [Feed], [feed_bound]"""
    total, nparts = int(offs[-1]), len(offs) - 1
    big = max((x for p in model.sizes for x in p), default=1)
    feeds, answers, bounds, pos, closed = [], [], [], 0, 0
    while (pos < total or closed < nparts) and len(feeds) < 400:
        wlen = min(int(rng.choice([0, 1, bs - 1, bs, bs + 1, 3 * bs - 1, int(rng.integers(0, 5 * bs)), total])), total - pos)
        ends = cu.ends_in_window(offs, pos, closed, wlen)
        cap = int(rng.choice([0, 1, 16, 17, 20, 21, 36, 37, big - 1, big, big + 1, 2 * big + 5, int(rng.integers(0, 6 * big)), 1 << 40]))
        f = model.feed(wlen, ends, cap)
        feeds.append((wlen, cap, ends))
        answers.append(f)
        bounds.append(cue.feed_bound(codec, model.bs, wlen, len(ends)))
        pos += f.consumed
        closed += f.parts_closed
    return feeds, answers, bounds


SCHEDULES = {cu.NONE: (6, 52), cu.LZ4: (6, 52), cu.SNAPPY: (6, 52), cu.LZF: (2, 12)}  # (map outputs, schedules on each)
assert sum(a * b for a, b in SCHEDULES.values()) >= 900


@pytest.mark.parametrize("codec", [cu.NONE, cu.LZ4, cu.SNAPPY, cu.LZF], ids=["none", "lz4", "snappy", "lzf"])
def test_host_arithmetic_against_the_python_model(oracle, model_exe, codec):
    bs = {cu.NONE: 1, cu.LZ4: 64, cu.SNAPPY: 1024, cu.LZF: 65535}[codec]
    shape_bs = 64 if codec == cu.NONE else bs
    rng = np.random.default_rng(300 + codec)
    n_outputs, n_schedules = SCHEDULES[codec]
    checked = 0
    for _ in range(n_outputs):
        data, offs = _map_output(rng, shape_bs, int(rng.integers(1, 9)))
        img, index, _ = oracle.compress_map_output(codec, 0, data, offs, block_size=bs if codec in (cu.LZ4, cu.SNAPPY) else 32768)
        plain = cu.unit_sizes_from_image(codec, np.asarray(img).tobytes(), index)  # the program adds its IV records itself
        sizes = cue.encrypted_unit_sizes(plain)
        for p in range(len(offs) - 1):  # 16 more on the first unit of each non-empty partition, nothing for an empty one
            assert sum(sizes[p]) == sum(plain[p]) + (16 if offs[p + 1] > offs[p] else 0)
        head = "%d %d %d\n" % (codec, bs, len(plain)) + "".join("%d %s\n" % (len(s), " ".join(map(str, s))) for s in plain)
        for _ in range(n_schedules):
            feeds, answers, bounds = _schedule(rng, cue.Model(codec, bs, sizes), codec, offs, bs)
            text = head + "".join("%d %d %d %s\n" % (w, c, len(e), " ".join(map(str, e))) for w, c, e in feeds)
            r = subprocess.run([model_exe, "plan"], input=text, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
            lines = r.stdout.strip().split("\n") if feeds else []
            assert len(lines) == len(feeds)
            for line, f, b, feed in zip(lines, answers, bounds, feeds):
                got = [int(x) for x in line.split()]
                assert (got[0], got[1], got[2], got[3], got[4], got[5], tuple(got[7:])) == f.fields(), (feed, line, f.fields())
                assert got[6] == b, (feed, got[6], b)
                if f.code == 0:
                    assert f.out_len <= b  # the bound holds every unit of the window
            checked += 1
    assert checked == n_outputs * n_schedules


def test_need_dst_and_first_units_of_none():
    m = cue.Model(cu.NONE, 1, [])
    f = m.feed(5, [5], 16)  # one byte below the first unit
    assert (f.code, f.need_dst) == (cu.E_CAPACITY, 17)
    f = m.feed(5, [5], 17)
    assert (f.code, f.consumed, f.out_len, f.parts_closed) == (0, 1, 17, 0)
    f = m.feed(4, [4], 0)  # inside the partition: a byte
    assert (f.code, f.need_dst) == (cu.E_CAPACITY, 1)
    f = m.feed(9, [4, 4, 9], 4 + 16)  # the partition's rest, an empty one, and the next one's IV does not fit without a byte
    assert (f.consumed, f.out_len, f.parts_closed, f.lengths) == (4, 4, 2, [21, 0])
    assert cue.feed_bound(cu.NONE, 1, 100, 3) == 100 + 64


# ---- ownership in the map-side geometry -------------------------------------------------------------------------------------
def _feed_case(rng, front, tile_chunks):
    """One feed's output as the stream lays it out: piece 0 continues a partition that has `front` stored bytes in front of the
    output (0: it starts here), the others start their partitions; a cut clamps the piece offsets, pieces behind it are empty."""
    key = rng.integers(0, 256, int(rng.choice([16, 24, 32])), dtype=np.uint8).tobytes()
    n = int(rng.integers(1, 7))
    plain_len = [int(rng.choice([0, 0, 1, 15, 16, 17, 31, 33, int(rng.integers(1, 90))])) for _ in range(n)]
    ivs = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    plains = [rng.integers(0, 256, m, dtype=np.uint8) for m in plain_len]
    lead = [16 if (m > 0 and not (j == 0 and front > 0)) else 0 for j, m in enumerate(plain_len)]
    stored = [a + m for a, m in zip(lead, plain_len)]
    full = np.concatenate([[0], np.cumsum(stored)]).astype(np.int64)
    # the cut: behind any stored byte that is not part of an IV or the IV's first byte's unit (the IV goes with a byte)
    allowed = [0]
    for j in range(n):
        allowed += [int(full[j]) + lead[j] + t for t in range(1, plain_len[j] + 1)]
    out_len = int(rng.choice(allowed)) if rng.integers(0, 3) else int(full[-1])
    E = np.minimum(full, out_len)
    Q = np.concatenate([[0], np.cumsum(plain_len)]).astype(np.int64)
    holed = np.concatenate([np.concatenate([np.full(a, 0xA5, np.uint8), p]) for a, p in zip(lead, plains)] + [np.zeros(0, np.uint8)])[:out_len]
    # the reference: spark_crypto_ref over the partitions that start in the output; the carried piece from its key stream offset
    first = 1 if front > 0 else 0
    img = np.concatenate(plains[first:] + [np.zeros(0, np.uint8)])
    idx = np.concatenate([[0], np.cumsum(plain_len[first:])]).astype(np.int64)
    enc, _, _ = scr.encrypt_map_output(img, idx, key, ivs[first:].reshape(-1))
    head = acm.xor_stream(key, ivs[0].tobytes(), plains[0], offset=front - 16) if first else np.zeros(0, np.uint8)
    want = np.concatenate([head, enc])[:out_len]
    return dict(key=key, n=n, front=front, tile=tile_chunks, E=E, Q=Q, ivs=ivs, src=np.concatenate(plains + [np.zeros(0, np.uint8)]),
                holed=holed, want=want)


def test_ownership_in_the_map_side_geometry(model_exe, tmp_path):
    rng = np.random.default_rng(77)
    fronts = [0] * 8 + [16 + r + 16 * int(rng.integers(0, 5)) for r in range(1, 17) for _ in range(3)]
    fronts += [(1 << 36) + 16 + r + int(rng.integers(0, 1 << 20)) * 16 for r in range(16)] + [(1 << 40) + 5, (1 << 36) + 17]
    assert {f % 16 for f in fronts if f} == set(range(16)) and sum(f > 1 << 36 for f in fronts) >= 16
    cases = [_feed_case(rng, f, int(rng.choice([1, 2, 3, 1024]))) for f in fronts for _ in range(4)]
    path_in, path_out = str(tmp_path / "feeds.bin"), str(tmp_path / "out.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            f.write(struct.pack("<I", len(c["key"])) + c["key"] + struct.pack("<iqq", c["n"], c["front"], c["tile"]))
            f.write(c["E"].astype(np.int64).tobytes() + c["Q"].astype(np.int64).tobytes() + c["ivs"].tobytes())
            f.write(struct.pack("<q", c["src"].size) + c["src"].tobytes() + c["holed"].tobytes())
    r = subprocess.run([model_exe, "own", path_in, path_out], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    cut_short = 0
    with open(path_out, "rb") as f:
        for i, c in enumerate(cases):
            L = int(c["E"][-1])
            in_place, from_plain, cover = (np.frombuffer(f.read(L), np.uint8) for _ in range(3))
            assert np.array_equal(in_place, c["want"]), (i, c["front"], list(c["E"]))
            assert np.array_equal(from_plain, c["want"]), (i, c["front"], list(c["E"]))
            assert np.all(cover == 1), (i, c["front"], list(c["E"]), cover.tolist())  # every stored byte owned exactly once
            cut_short += int(np.any(np.diff(c["E"]) == 0) and L > 0)
        assert f.read() == b""
    assert cut_short > 20  # zero-length pieces (empty partitions and pieces behind the cut) were played


# ---- the compiled cut kernel and cut gather on a plan with IV records -------------------------------------------------------
def _interpreter_case(oracle):
    sys.path.insert(0, os.path.join(ROOT, "tests", "isa"))
    import cstream_encrypted_kernel as cek

    rng = np.random.default_rng(5)
    parts = [bytes(np.resize(np.frombuffer(b"abcdabcdabcdabce", np.uint8), 70)), b"", rng.integers(0, 256, 10, dtype=np.uint8).tobytes()]
    data = np.frombuffer(b"".join(parts), np.uint8)
    offs = np.array([0, 70, 70, 80], np.int64)
    img, index, _ = oracle.compress_map_output(cu.LZ4, 0, data, offs, block_size=64)
    img = np.asarray(img).tobytes()
    sizes = cue.unit_sizes_from_plain_image(cu.LZ4, img, index)
    stored = cue.stored_index(index)
    flat = [x for p in sizes for x in p]
    assert len(flat) == 5 and stored[-1] == len(img) + 32
    holed = b"".join((b"\xa5" * 16 + img[int(index[p]):int(index[p + 1])]) if index[p + 1] > index[p] else b"" for p in range(3))
    return cek, parts, img, index, sizes, stored, flat, holed


def test_cut_kernel_and_cut_gather_with_iv_records_in_the_interpreter(oracle):
    """LZ4 at block size 64, partitions of 70, 0 and 10 bytes: five units, two of them with an IV record in front; dst has
    exactly dst_capacity bytes and every taken partition's 16-byte hole keeps the prefill at its stored offset"""
    cek, parts, img, index, sizes, stored, flat, holed = _interpreter_case(oracle)
    for cap in (stored[-1], sum(flat[:3]) + 5, sum(flat[:3]), sum(flat[:3]) + 16, sum(flat[:3]) + 17, sum(flat[:2]) + 20, flat[0], flat[0] - 1, 16, 0):
        want = cue.Model(cu.LZ4, 64, sizes).feed(80, [70, 70, 80], cap)
        got = cek.feed_lz4_encrypted(parts, 64, cap)
        assert got["status"] == 0
        if want.code == cu.E_CAPACITY:
            assert want.need_dst == cue.need_dst_first(cu.LZ4, flat[0] - 16)
            assert (got["k"], got["consumed"], got["out_len"], got["need_dst"], got["parts_closed"]) == (0, 0, 0, want.need_dst, 0)
            assert got["dst"] == b"\xa5" * cap
            continue
        assert (got["consumed"], got["out_len"], got["need_dst"], got["parts_closed"]) == (want.consumed, want.out_len, 0, want.parts_closed), cap
        assert got["lengths"][:want.parts_closed] == want.lengths and not any(got["lengths"][want.parts_closed:])
        assert got["piece_off"] == [min(int(x), want.out_len) for x in stored] + [want.out_len]
        assert got["dst"] == holed[:want.out_len] + b"\xa5" * (cap - want.out_len), cap


def test_the_compiled_encrypt_pass_behind_the_cut_in_the_interpreter(oracle):
    """the same feeds with aes_ctr_cstream_kernel<10, in place> behind the gather: it reads out_len from the cut's result words,
    its grid is sized from the capacity alone, and dst - exactly dst_capacity bytes - holds the one-shot encrypted image up to
    the cut and the prefill behind it"""
    cek, parts, img, index, sizes, stored, flat, holed = _interpreter_case(oracle)
    key = bytes(range(16))
    nr, rk = acm.expand_key(key)
    assert nr == 10
    ivs = np.random.default_rng(8).integers(0, 256, (4, 16), dtype=np.uint8)
    want_img, want_index, _ = scr.encrypt_map_output(np.frombuffer(img, np.uint8), index, key, ivs[:3].reshape(-1))
    assert [int(x) for x in want_index] == stored
    for cap in (stored[-1], stored[-1] + 40, sum(flat[:3]) + 5, sum(flat[:2]) + 20, flat[0], flat[0] - 1):
        want = cue.Model(cu.LZ4, 64, sizes).feed(80, [70, 70, 80], cap)
        got = cek.feed_lz4_encrypted(parts, 64, cap, round_keys=rk, ivs=ivs)
        n = 0 if want.code == cu.E_CAPACITY else want.out_len
        assert got["out_len"] == n and got["dst"] == want_img[:n].tobytes() + b"\xa5" * (cap - n), cap
