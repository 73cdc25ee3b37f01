"""Inputs and the host program for the tests of resumable Zstandard streams (s3s_dstream_open_zstd): TEST INFRASTRUCTURE.
The program is tests/model/zstd_stream_model.cpp - the library's unit walk and resumable decoder compiled for the host with a
main of its own, under ASan / UBSan, run directly (nothing is loaded into Python)."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
SRC = os.path.join(HERE, "model", "zstd_stream_model.cpp")
CORES = [os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", n) for n in ("zstd_stream_core.h", "zstd_decode_core.h")]

import zstd_writer as W  # noqa: E402
import stream_units_zstd as U  # noqa: E402

OK, E_CAPACITY, E_BAD_FRAME, E_UNSUPPORTED = 0, -2, -3, -6


def program():
    exe = os.path.join(HERE, "model", "zstd_stream_model")
    if not os.path.exists(exe) or max(os.path.getmtime(p) for p in [SRC] + CORES) > os.path.getmtime(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], check=True)
    return exe


def plain_program():
    """The same program without the sanitizers, for the report a GPU test compares the device with (sanitizers stay on the CPU side)."""
    exe = os.path.join(HERE, "model", "zstd_stream_model_plain")
    if not os.path.exists(exe) or max(os.path.getmtime(p) for p in [SRC] + CORES) > os.path.getmtime(exe):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", SRC, "-o", exe], check=True)
    return exe


def _run(mode, path, sanitized=True):
    return subprocess.run([program() if sanitized else plain_program(), mode, path], capture_output=True, text=True,
                          env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))


def run_decode(cases, workdir):
    """cases: [(partition bytes, content or None, expected code, wlog, cap, mode, cuts)] -> CompletedProcess (0: all as expected)"""
    path = os.path.join(workdir, "cases.bin")
    with open(path, "wb") as f:
        for comp, content, want, wlog, cap, mode, cuts in cases:
            comp = bytes(comp)
            content = None if content is None else bytes(content)
            f.write(struct.pack("<qqiiqii", len(comp), -1 if content is None else len(content), want, wlog, cap, mode, len(cuts)))
            f.write(struct.pack("<%dq" % len(cuts), *cuts))
            f.write(comp)
            if content:
                f.write(content)
    return _run("decode", path)


def run_report(cases, workdir, sanitized=True):
    """cases: [(partition bytes, wlog, cap, mode, cuts)] -> [(code, bytes handed out, their CRC32)]: what the stream answers,
    nothing expected of it (the same sanitized program; a sanitizer report fails here)"""
    path = os.path.join(workdir, "report.bin")
    with open(path, "wb") as f:
        for comp, wlog, cap, mode, cuts in cases:
            comp = bytes(comp)
            f.write(struct.pack("<qqiiqii", len(comp), -1, 0, wlog, cap, mode, len(cuts)))
            f.write(struct.pack("<%dq" % len(cuts), *cuts))
            f.write(comp)
    r = _run("report", path, sanitized)
    os.remove(path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    out = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def run_units(records, workdir):
    """records: [(window bytes, pend, open, wlog)] -> [(n, stop, need, [(off, kind, payload)])] from the host build of the walk"""
    path = os.path.join(workdir, "units.bin")
    with open(path, "wb") as f:
        for win, pend, open_, wlog in records:
            win = bytes(win)
            f.write(struct.pack("<qqii", len(win), pend, 1 if open_ else 0, wlog) + win)
    r = _run("units", path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = []
    for line in r.stdout.splitlines():
        t = line.split()
        out.append((int(t[0]), int(t[1]), int(t[2]), [tuple(int(x) for x in u.split(":")) for u in t[3:]]))
    assert len(out) == len(records)
    return out


def model_units(win, pend, open_, wlog):
    """The contract model's answer in the program's form."""
    try:
        u, stop, need, _ = U.walk(bytes(win), pend, open_, wlog)
    except U.Bad:
        return (-1, 0, 0, [])
    except U.Refused:
        return (-2, 0, 0, [])
    return (len(u), stop, need, [(o, k, p) for o, k, p, _ in u])


# ---- libzstd's frames ----------------------------------------------------------------------------------------------------------
_cache = {}


def source(kind, n):
    import corpus

    key = ("src", kind, n)
    if key not in _cache:
        _cache[key] = corpus.chunk_corpus(kind, n, np.random.default_rng(100 + kind))
    return _cache[key]


def compress(data, level=1, window_log=0, flush=0, chunk=32768):
    """One libzstd streaming frame (no content size): the bytes arrive `chunk` at a time; flush > 0: ZSTD_e_flush after every
    `flush` bytes (a block ends there).  window_log 0: the level's default for an unknown source size."""
    from oracle import zstd_ref

    if not flush:
        return zstd_ref.compress_stream(data, level=level, chunk=chunk, window_log=window_log)
    z = zstd_ref.lib()
    d = np.ascontiguousarray(data, dtype=np.uint8)
    cctx = z.ZSTD_createCCtx()
    try:
        z.ZSTD_CCtx_setParameter(cctx, zstd_ref.ZSTD_c_compressionLevel, level)
        if window_log:
            z.ZSTD_CCtx_setParameter(cctx, zstd_ref.ZSTD_c_windowLog, window_log)
        cap = int(z.ZSTD_compressBound(d.size)) + 16 * (d.size // flush + 2) + 4096 + d.size // 64
        out = np.empty(cap, dtype=np.uint8)
        ob = zstd_ref._Buf(out.ctypes.data, cap, 0)
        pos = 0
        while pos < d.size:
            n = min(flush, d.size - pos)
            ib = zstd_ref._Buf(d.ctypes.data + pos, n, 0)
            while True:
                r = z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), zstd_ref.ZSTD_e_flush)
                assert not z.ZSTD_isError(r)
                if r == 0 and ib.pos == ib.size:
                    break
            pos += n
        ib = zstd_ref._Buf(d.ctypes.data, 0, 0)
        while True:
            r = z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), zstd_ref.ZSTD_e_end)
            assert not z.ZSTD_isError(r)
            if r == 0:
                break
        return out[:ob.pos].copy()
    finally:
        z.ZSTD_freeCCtx(cctx)


def frame_window_log(frame):
    """log2 of the Window_Size of a frame with a window descriptor, rounded up (what window_log_max must be at least)."""
    w = U.window_size(bytes(frame[:U.header_length(int(frame[4]))]))
    return max(10, (w - 1).bit_length())


def unit_ends(part):
    return [o + n for o, _, _, n in U.partition_units(bytes(part))]


# ---- frames of the spec-level writer: every piece of carried state across a cut --------------------------------------------
def crafted():
    """name -> (frame bytes, content or None, expected code, window_log_max)"""
    import zstd_staged_lib as S

    out = {}
    for name in S.VALID_CASES:  # Repeat_Mode per field and after RLE mode, treeless literals, repeat codes 1..3 with llen == 0, raw / RLE between
        data, content, _ = S.crafted(name)
        out[name] = (data.tobytes(), content.tobytes(), OK, frame_window_log(data))
    for name in S.INVALID_CASES:
        if name == "g_nseq":
            continue
        data, _, _ = S.crafted(name)
        out[name] = (data.tobytes(), None, E_BAD_FRAME, 10)
    h = bytes(np.random.default_rng(9).integers(0, 256, 1024, dtype=np.uint8))
    # a match whose source starts exactly Window_Size (1 KiB) back: two raw blocks fill the window, the match follows two cuts later
    f = W.Frame(window=(0, 0))
    f.raw(h[:512]).raw(h[512:]).compressed(b"", [(0, 8, 1024)]).compressed(b"xyz", [(3, 5, 1024)])
    data, content = f.finish()
    out["window_exact"] = (data, content, OK, 10)
    # one byte further than the window, inside the frame: the one-shot call has the byte, a stream has not - invalid by RFC 8878
    f = W.Frame(window=(0, 0), strict=False)
    f.raw(h[:512]).raw(h[512:]).raw(b"!").compressed(b"", [(0, 8, 1025)])
    data, _ = f.finish()
    out["window_beyond"] = (data, None, E_BAD_FRAME, 10)
    # refusals
    f = W.Frame(checksum=True)
    f.raw(h[:100])
    out["checksum"] = (f.finish()[0], None, E_UNSUPPORTED, 10)
    f = W.Frame(did_bytes=1, did=0)
    f.raw(h[:100])
    out["dictionary_id"] = (f.finish()[0], None, E_UNSUPPORTED, 10)
    f = W.Frame(window=(1, 0))
    f.raw(h[:100])
    out["window_above"] = (f.finish()[0], None, E_UNSUPPORTED, 10)
    out["skippable_big"] = ((0x184D2A50).to_bytes(4, "little") + ((32 << 20) - 7).to_bytes(4, "little") + b"x" * 64, None, E_UNSUPPORTED, 10)
    # skippable frames and two frames in one partition, a single-segment frame, an empty frame
    f1 = W.Frame(single=True, fcs_bytes=1)
    f1.raw(h[:77])
    f2 = W.Frame()
    f2.raw(b"")
    d1, c1 = f1.finish()
    d2, c2 = f2.finish()
    a, ca, _ = S.crafted("b")
    out["several_frames"] = (W.skippable(b"hello") + d1 + W.skippable(b"") + a.tobytes() + d2, c1 + ca.tobytes() + c2, OK, 12)
    return out


# ---- the conformance corpus, classified by the contract model ------------------------------------------------------------------
def conformance_cases():
    """(cases of tests/zstd_conformance.py as tests/test_gpu_zstd_conformance.py takes them, the code a stream must end with):
    0 with the case's content, S3S_E_UNSUPPORTED where the contract model finds a frame outside the feature first, else
    S3S_E_BAD_FRAME."""
    if "conf" not in _cache:
        import zstd_conformance as zc

        cases = zc.fixed_corpus() + [zc.generated_case(seed) for seed in range(400)]
        for c in cases:
            zc.arbiter(c)
        expect = []
        for c in cases:
            try:
                U.partition_units(c.data, 27)
                expect.append(OK if c.rc == 0 else E_BAD_FRAME)
            except U.Refused:
                expect.append(E_UNSUPPORTED)
            except (U.Bad, AssertionError):
                expect.append(E_BAD_FRAME)
        _cache["conf"] = (cases, expect)
    return _cache["conf"]


# ---- field-targeted damage -----------------------------------------------------------------------------------------------------
E_CHECKSUM = -4
DAMAGE_BAD_PARTITION = {"wrong_checksum_of_the_partition_behind": 2}  # (every other case: partition 1)
# Fed unit by unit, the damaged header is met while its partition is still open - the window does not hold the partition's last
# byte - and the contract reports a corrupt frame of an open partition first; in one feed the window holds it: the checksum first
DAMAGE_WANT_UNIT_BY_UNIT = {"wrong_checksum_and_damage": E_BAD_FRAME}
DAMAGE_NAMES = ["magic", "reserved_bit", "checksum_flag", "did_flag", "window_raised", "single_segment_flag", "block_type_3",
                "block_size_past_partition", "block_size_above_128k", "last_flag_cleared", "last_flag_set_early", "sequence_byte",
                "huffman_byte", "truncated_in_block", "truncated_in_header", "truncated_at_block_boundary", "skippable_above_32m",
                "wrong_checksum", "wrong_checksum_and_damage", "wrong_checksum_of_the_partition_behind"]


def _literals_end(block):
    """Bytes of a compressed block's literals section (RFC 8878 3.1.1.3.1.1), and whether it is Huffman-coded."""
    t, sf = block[0] & 3, (block[0] >> 2) & 3
    if t < 2:
        lh = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = block[0] >> 3 if lh == 1 else (int.from_bytes(block[:lh], "little") >> 4)
        return lh + (regen if t == 0 else 1), False
    lh = 3 if sf < 2 else 4 if sf == 2 else 5
    v = int.from_bytes(block[:lh], "little")
    comp = v >> 14 if lh == 3 else v >> 18 if lh == 4 else v >> 22
    return lh + comp, True


def damage_cases():
    """name -> (image, index, checksums or None, checksum algorithm, the code a stream ends with, what the output is a prefix of).
    Three partitions: a good frame, the damaged one (a libzstd window_log 10 frame of 8 KiB of text: a dozen blocks with Huffman
    literals and sequences), a good frame.  window_log_max is 10."""
    if "damage" in _cache:
        return _cache["damage"]
    import zlib

    good, good_content = crafted()["fcs"][:2]
    src = source(6, 8 << 10)
    frame = compress(src, 1, 10).tobytes()
    units = U.partition_units(frame)
    hl = units[0][3]
    comp = [u for u in units if (u[1] & 15) == U.COMP]
    assert len(comp) >= 6 and hl == 6
    b2, b3, blast = units[2], units[3], units[-1]

    def put(at, value, base=frame):
        return base[:at] + bytes([value]) + base[at + 1:]

    def header(off, last=None, typ=None, size=None):
        bh = int.from_bytes(frame[off:off + 3], "little")
        l, t, s = bh & 1, (bh >> 1) & 3, bh >> 3
        l, t, s = (l if last is None else last), (t if typ is None else typ), (s if size is None else size)
        return frame[:off] + (l | t << 1 | s << 3).to_bytes(3, "little") + frame[off + 3:]

    hufblock = next(u for u in comp if _literals_end(frame[u[0] + 3:u[0] + u[3]])[1])
    lit_end = _literals_end(frame[hufblock[0] + 3:hufblock[0] + hufblock[3]])[0]
    seq_at = hufblock[0] + 3 + lit_end + (hufblock[3] - 3 - lit_end) // 2
    huf_at = hufblock[0] + 3 + lit_end - 1  # the last byte of the last Huffman stream: its top bits hold the end mark
    out = {}

    def case(name, damaged, want, algo=0, part_len=None, wrong_sum=None):
        damaged = damaged[:part_len] if part_len is not None else damaged
        parts = [good, damaged, good]
        img = np.frombuffer(b"".join(parts), np.uint8)
        index = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        sums = None
        if algo:
            sums = np.array([zlib.adler32(p) & 0xFFFFFFFF for p in parts], np.int64)
            if wrong_sum is not None:
                sums[wrong_sum] ^= 1
        out[name] = (img, index, sums, algo, want, np.frombuffer(good_content + src.tobytes() + good_content, np.uint8))

    case("magic", put(1, frame[1] ^ 0x40), E_BAD_FRAME)
    case("reserved_bit", put(4, frame[4] | 0x08), E_BAD_FRAME)
    case("checksum_flag", put(4, frame[4] | 0x04), E_UNSUPPORTED)
    case("did_flag", put(4, frame[4] | 0x01), E_UNSUPPORTED)
    case("window_raised", put(5, 10 << 3), E_UNSUPPORTED)            # Window_Size 1 MiB under window_log_max 10
    case("single_segment_flag", put(4, frame[4] | 0x20), E_BAD_FRAME)  # the window byte becomes a content size of 0
    case("block_type_3", header(b2[0], typ=3), E_BAD_FRAME)
    case("block_size_past_partition", header(b3[0], size=len(frame)), E_BAD_FRAME)
    case("block_size_above_128k", header(b3[0], typ=0, size=(128 << 10) + 1), E_BAD_FRAME)
    case("last_flag_cleared", header(blast[0], last=0), E_BAD_FRAME)  # the partition ends with a frame open
    case("last_flag_set_early", header(b2[0], last=1), E_BAD_FRAME)   # what follows is no frame
    case("sequence_byte", put(seq_at, frame[seq_at] ^ 0x10), E_BAD_FRAME)
    case("huffman_byte", put(huf_at, frame[huf_at] ^ 0x80), E_BAD_FRAME)  # (most flips inside a stream resynchronise and decode: this one moves the end mark)
    case("truncated_in_block", frame, E_BAD_FRAME, part_len=b3[0] + 5)
    case("truncated_in_header", frame, E_BAD_FRAME, part_len=4)
    case("truncated_at_block_boundary", frame, E_BAD_FRAME, part_len=b3[0])
    case("skippable_above_32m", (0x184D2A51).to_bytes(4, "little") + (32 << 20).to_bytes(4, "little") + frame, E_UNSUPPORTED)
    case("wrong_checksum", frame, E_CHECKSUM, algo=1, wrong_sum=1)
    case("wrong_checksum_and_damage", header(b2[0], typ=3), E_CHECKSUM, algo=1, wrong_sum=1)  # the checksum is reported first
    case("wrong_checksum_of_the_partition_behind", frame, E_CHECKSUM, algo=1, wrong_sum=2)  # the frames in front of it are handed out first
    assert list(out) == DAMAGE_NAMES
    _cache["damage"] = out
    return out
