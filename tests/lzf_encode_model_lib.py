"""The host build of the product's LZF writer core (tests/model/lzf_encode_model.cpp) for the tests that have the oracle and
liblzf read its streams and that demand the same bytes of the GPU: a shared object for ctypes (built on demand next to its
source) and an AddressSanitizer program that writes the streams of a file of segments from heap buffers of exactly the
permitted sizes.  Also the readers the tests share: a token-level walk of a stream and liblzf's own decoder."""
import ctypes
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "model", "lzf_encode_model.cpp")
CORE = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", "lzf_encode_core.h")
CHUNK = 65535
MAX_OFF, MAX_REF, MAX_LIT = 8192, 264, 32
LIBLZF_PYTHON = "/opt/conda/bin/python3.9"
LIBLZF_FILTER = os.path.join(HERE, "golden", "make_lzf_golden.py")


def _stale(out):
    return not os.path.exists(out) or max(os.path.getmtime(SRC), os.path.getmtime(CORE)) > os.path.getmtime(out)


def load():
    so = os.path.join(HERE, "model", "lzf_encode_model.so")
    if _stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    m = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    m.le_stream_bound.restype = i64
    m.le_stream_bound.argtypes = [i64]
    m.le_encode_stream.restype = i64
    m.le_encode_stream.argtypes = [vp, i64, vp, i64]
    m.le_encode_block.restype = i64
    m.le_encode_block.argtypes = [vp, i64, vp, i64]
    return m


def asan_program():
    exe = os.path.join(HERE, "model", "lzf_encode_asan")
    if _stale(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DLE_MAIN", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    return exe


def stream_bound(n):
    """ulen + 7 * ceil(ulen / 65535): the oracle's s3o_lzf_max_stream_size."""
    return 0 if n <= 0 else n + 7 * (-(-n // CHUNK))


def encode_stream(model, src):
    src = np.ascontiguousarray(src, dtype=np.uint8)
    cap = int(model.le_stream_bound(src.size))
    assert cap == stream_bound(src.size)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    r = int(model.le_encode_stream(src.ctypes.data, src.size, out.ctypes.data, cap))
    assert 0 <= r <= cap
    return out[:r].copy()


def block_size(model, chunk):
    """Bytes of the liblzf block the writer makes of one chunk (what decides stored / compressed)."""
    chunk = np.ascontiguousarray(chunk, dtype=np.uint8)
    cap = chunk.size + chunk.size // 32 + 4
    out = np.empty(max(cap, 1), dtype=np.uint8)
    r = int(model.le_encode_block(chunk.ctypes.data, chunk.size, out.ctypes.data, cap))
    assert 0 <= r <= cap
    return r


def run_asan(sources, workdir):
    """The streams the sanitised program wrote for the given segments."""
    path_in, path_out = os.path.join(workdir, "cases.bin"), os.path.join(workdir, "streams.bin")
    with open(path_in, "wb") as f:
        f.write(struct.pack("<I", len(sources)))
        for s in sources:
            s = np.ascontiguousarray(s, dtype=np.uint8)
            f.write(struct.pack("<Q", s.size))
            f.write(s.tobytes())
    r = subprocess.run([asan_program(), path_in, path_out], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    streams = []
    with open(path_out, "rb") as f:
        for _ in sources:
            (sz,) = struct.unpack("<q", f.read(8))
            streams.append(np.frombuffer(f.read(max(sz, 0)), dtype=np.uint8))
    return streams


def chunks(stream):
    """[(stored?, ulen, payload bytes)] of a stream; asserts the framing."""
    b = bytes(stream)
    out, ip = [], 0
    while ip < len(b):
        assert b[ip:ip + 2] == b"ZV" and b[ip + 2] in (0, 1), "chunk magic at %d" % ip
        if b[ip + 2] == 0:
            (n,) = struct.unpack_from(">H", b, ip + 3)
            ip += 5
            assert ip + n <= len(b)
            out.append((True, n, b[ip:ip + n]))
            ip += n
        else:
            clen, ulen = struct.unpack_from(">HH", b, ip + 3)
            ip += 7
            assert ip + clen <= len(b)
            out.append((False, ulen, b[ip:ip + clen]))
            ip += clen
    return out


def tokens(block):
    """[("lit", count) | ("ref", length, offset)] of a liblzf block."""
    out, ip = [], 0
    while ip < len(block):
        ctrl = block[ip]
        ip += 1
        if ctrl < 32:
            out.append(("lit", ctrl + 1))
            ip += ctrl + 1
        else:
            ln = ctrl >> 5
            if ln == 7:
                ln += block[ip]
                ip += 1
            out.append(("ref", ln + 2, ((ctrl & 0x1F) << 8 | block[ip]) + 1))
            ip += 1
    assert ip == len(block), "the last token runs past the block"
    return out


def check_tokens(model, stream, src):
    """The token-level conditions on a stream of src; returns [(stored?, tokens or None)] per chunk."""
    src = np.ascontiguousarray(src, dtype=np.uint8)
    got, pos = [], 0
    for stored, ulen, payload in chunks(stream):
        want = min(CHUNK, src.size - pos)
        assert ulen == want, "ulen %d of a chunk of %d bytes" % (ulen, want)
        c = block_size(model, src[pos:pos + ulen])
        if stored:
            assert c >= ulen - 2, "a chunk whose block (%d) is two bytes shorter than its %d bytes was stored" % (c, ulen)
            assert payload == src[pos:pos + ulen].tobytes()
            got.append((True, None))
        else:
            assert len(payload) == c and c < ulen - 2
            toks, at = tokens(payload), 0
            for t in toks:
                if t[0] == "lit":
                    assert 1 <= t[1] <= MAX_LIT
                    at += t[1]
                else:
                    assert 3 <= t[1] <= MAX_REF and 1 <= t[2] <= MAX_OFF
                    assert t[2] <= at, "a reference reaches %d bytes back at byte %d of its chunk" % (t[2], at)
                    at += t[1]
            assert at == ulen
            got.append((False, toks))
        pos += ulen
    assert pos == src.size
    return got


def liblzf_available():
    if not os.path.exists(LIBLZF_PYTHON):
        return False
    return subprocess.run([LIBLZF_PYTHON, "-c", "import imagecodecs"], capture_output=True).returncode == 0


def liblzf_decode_stream(stream):
    """The stream's chunks decoded by liblzf 3.6 itself (compressed chunks; stored ones are copied)."""
    out = bytearray()
    for stored, ulen, payload in chunks(stream):
        if stored:
            out += payload
            continue
        r = subprocess.run([LIBLZF_PYTHON, LIBLZF_FILTER, "--decode", str(ulen)], input=payload, capture_output=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(r.stdout) == ulen
        out += r.stdout
    return np.frombuffer(bytes(out), dtype=np.uint8)


# ---- the inputs the CPU and the GPU tests share: built once, never modified -----------------------------------------------
_cache = {}
NAMED = ("zeros", "random", "terasort", "wide", "kv")
EDGE_SIZES = [0, 1, 2, 3, 65534, 0, 65535, 65536, 131071]


def words(rng, n):
    """n bytes of text from a vocabulary of 200 words."""
    vocab = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += b" ".join(vocab[int(i)] for i in rng.integers(0, 200, 4096)) + b" "
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8)


def inputs():
    """name -> (data, offsets)."""
    if not _cache:
        from s3shuffle import datagen

        offs = np.concatenate([[0], np.cumsum(EDGE_SIZES)]).astype(np.int64)
        _cache["edges"] = (words(np.random.default_rng(17), int(offs[-1])), offs)
        _cache["zeros"] = datagen.skew_block(1 << 20, "zeros", seed=5)
        _cache["random"] = datagen.skew_block(1 << 20, "random", seed=5)
        _cache["terasort"] = datagen.terasort_map_output(4 << 20, 8, seed=2)
        _cache["wide"] = datagen.tpcds_wide_map_output(4 << 20, 8, seed=3)
        _cache["kv"] = datagen.kv_int_map_output(300_000, 7, seed=1)
        for d, _ in _cache.values():
            d.flags.writeable = False
    return _cache


def model_streams(data, offs, name=None):
    """The streams the host build of the writer produces, one per partition (those of the named inputs are kept)."""
    key = ("model", name)
    if name is None or key not in _cache:
        m = load()
        streams = [encode_stream(m, data[offs[p]:offs[p + 1]]) for p in range(len(offs) - 1)]
        if name is None:
            return streams
        _cache[key] = streams
    return _cache[key]


def oracle_image_size(oracle, name):
    """Bytes of the oracle's LZF image of a named input (s3o_lzf_compress_stream per partition): the reference of the size
    conditions, computed at test time."""
    key = ("oracle", name)
    if key not in _cache:
        data, offs = inputs()[name]
        _cache[key] = int(oracle.compress_map_output(4, 0, data, offs)[0].size)
    return _cache[key]


def check_size_conditions(sizes, oracle):
    """sizes: name -> image bytes of the writer under test.  The five conditions."""
    ins = inputs()
    for name in ("terasort", "wide"):
        ref = oracle_image_size(oracle, name)
        print("%-9s source %9d  image %9d  oracle LZF image %9d  (%+.1f %%)" % (name, ins[name][0].size, sizes[name], ref, 100.0 * (sizes[name] / ref - 1)))
        assert sizes[name] <= 1.15 * ref, "%s: more than 15 %% above the oracle's LZF image" % name
    zeros = ins["zeros"][0].size
    print("zeros     source %9d  image %9d  oracle LZF image %9d" % (zeros, sizes["zeros"], oracle_image_size(oracle, "zeros")))
    assert sizes["zeros"] < 0.02 * zeros, "zeros: not below 2 % of the source"
    data, offs = ins["random"]
    n_chunks = sum(-(-int(offs[p + 1] - offs[p]) // CHUNK) for p in range(len(offs) - 1))
    print("random    source %9d  image %9d  oracle LZF image %9d" % (data.size, sizes["random"], oracle_image_size(oracle, "random")))
    assert sizes["random"] == data.size + 5 * n_chunks, "random: a chunk was not stored"
    ref = oracle_image_size(oracle, "kv")
    print("kv        source %9d  image %9d  oracle LZF image %9d" % (ins["kv"][0].size, sizes["kv"], ref))
    assert sizes["kv"] <= ref, "kv: larger than the oracle's image"
