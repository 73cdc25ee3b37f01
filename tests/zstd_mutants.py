"""Deterministic mutants of Zstandard frames for the block, staged and stream paths of the reduce side: TEST INFRASTRUCTURE.

    mutants(family, seed, count) -> [(index, bytes, content size of the seed frame, capacity)]

The same arguments give the same bytes everywhere: the only randomness is np.random.default_rng([seed, family id]), and nothing
is bounded by time.  Seed frames are the smallest that still reach each path (tests/test_zstd_mutants_model.py measures, per
family, how many mutants do):

    flushed4k    libzstd streaming frames of 40 000 bytes, flushed every 4 096 bytes: ~10 blocks with history (staged path)
    flushed1500  the same over 20 000 bytes, flushed every 1 500 bytes: ~14 blocks
    stream300k   libzstd streaming frames of 300 000 bytes as Spark's writer makes them: three 128 KiB blocks
    writer       frames of the map side's writer (host build of zstd_encode_core.h) over 2 * 131072 + 1 + 1000 * kind bytes: three
                 block-independent blocks (block path)
    two_frames   a writer frame, then a flushed4k frame in one partition: the block path claims the prefix, the staged path
                 starts behind it
    crafted      the valid crafted frames of tests/zstd_staged_lib.py: Repeat_Mode tables, Treeless literals, repeat offsets
                 across blocks
    wlog10       level-3 frames with window log 10 over 40 000 bytes: the stream's window edge

The mutations are the eight kinds of tests/model/zstd_asan_fuzz.cpp, one to three repetitions each; MIX gives a family's weights
of the kinds where the uniform mix leaves too few accepted or too few refused mutants."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE, os.path.join(ROOT, "spark-s3-shuffle_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FAMILIES = ["flushed4k", "flushed1500", "stream300k", "writer", "two_frames", "crafted", "wlog10"]
KINDS = (2, 3, 4, 6, 7)  # of corpus.chunk_corpus
BIT_FLIP, TRUNCATE, RANDOM4, HEADER_BYTE, SPLICE, EXTREME, INSERT, DELETE = range(8)
MUTATIONS = ["bit flip", "truncation", "4 random bytes", "a byte among the first 64", "splice", "extreme byte", "inserted run", "deleted run"]
UNIFORM = (1,) * 8
# Weights of the eight kinds per family (tests/test_zstd_mutants_model.py asks for at least 10 % accepted and 40 % refused).
# The writer's frames are mostly entropy-coded bytes and sequence streams, where almost nothing but a single flipped bit or byte
# survives: under the uniform mix 9.3 % of their mutants were accepted, so these two families flip bits three times and set
# extreme bytes twice as often.
MIX = {"writer": (3, 1, 1, 1, 1, 2, 1, 1), "two_frames": (3, 1, 1, 1, 1, 2, 1, 1)}

_cache = {}


def seeds(family):
    """[(frame bytes, content size)] of a family."""
    if family in _cache:
        return _cache[family]
    import zstd_staged_lib as S
    from oracle import zstd_ref

    def src(kind, n):
        return S.source(kind)[:n]

    if family == "flushed4k":
        out = [(S.compress_flushed(src(k, 40_000), 1, 4096).tobytes(), 40_000) for k in KINDS]
    elif family == "flushed1500":
        out = [(S.compress_flushed(src(k, 20_000), 1, 1500).tobytes(), 20_000) for k in KINDS]
    elif family == "stream300k":
        out = [(zstd_ref.compress_stream(src(k, 300_000), 1).tobytes(), 300_000) for k in KINDS]
    elif family == "writer":
        import zstd_encode_model_lib as E

        m = E.load()
        out = [(E.encode_frame(m, src(k, 2 * 131072 + 1 + 1000 * k)).tobytes(), 2 * 131072 + 1 + 1000 * k) for k in KINDS]
    elif family == "two_frames":
        out = [(w + f, wn + fn) for (w, wn), (f, fn) in zip(seeds("writer"), seeds("flushed4k"))]
    elif family == "crafted":
        out = []
        for case in S.VALID_CASES:
            data, content, _ = S.crafted(case)
            out.append((data.tobytes(), int(content.size)))
    elif family == "wlog10":
        out = [(zstd_ref.compress_stream(src(k, 40_000), 3, window_log=10).tobytes(), 40_000) for k in KINDS]
    else:
        raise KeyError(family)
    _cache[family] = out
    return out


def mutate(m, kind, rng, others):
    """One repetition of mutation `kind` on the non-empty bytearray m; `others` are the seeds a splice takes its tail from."""
    def R(n):
        return int(rng.integers(0, n)) if n > 0 else 0

    if kind == BIT_FLIP:
        m[R(len(m))] ^= 1 << R(8)
    elif kind == TRUNCATE:
        del m[1 + R(len(m)):]
    elif kind == RANDOM4:
        i = R(len(m))
        for k in range(i, min(len(m), i + 4)):
            m[k] = R(256)
    elif kind == HEADER_BYTE:
        m[R(min(len(m), 64))] = R(256)
    elif kind == SPLICE:
        o = others[R(len(others))][0]
        a, b = R(len(m)), R(len(o))
        del m[a:]
        m += o[b:]
    elif kind == EXTREME:
        m[R(len(m))] = 0xFF if R(2) else 0x00
    elif kind == INSERT:
        i, n = R(len(m)), 1 + R(16)
        m[i:i] = bytes([R(256)]) * n
    else:
        i, n = R(len(m)), 1 + R(16)
        del m[i:i + n]


def seeded_cuts(family, seed, mutant_list):
    """Per mutant, up to 12 window ends for a stream that is fed it (a generator of their own: the same for every prefix of the list)."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), 12])
    out = []
    for _, data, _, _ in mutant_list:
        n = len(data)
        out.append(sorted(set(int(x) for x in rng.integers(1, max(n, 2), 12))))
    return out


def mutants(family, seed, count):
    """[(index, bytes, content size of the seed frame, capacity)]: capacity is the content size, the content size + 4096 (three
    quarters of the draws between them), the content size - 1, or a random smaller value."""
    fam = seeds(family)
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    w = np.array(MIX.get(family, UNIFORM), dtype=np.float64)
    w /= w.sum()
    out = []
    for index in range(count):
        frame, size = fam[int(rng.integers(0, len(fam)))]
        m = bytearray(frame)
        kind = int(rng.choice(8, p=w))
        for _ in range(1 + int(rng.integers(0, 3))):
            if not m:
                break
            mutate(m, kind, rng, fam)
        draw = int(rng.integers(0, 8))
        cap = size if draw < 3 else size + 4096 if draw < 6 else size - 1 if draw == 6 else int(rng.integers(0, max(size, 1)))
        out.append((index, bytes(m), size, max(cap, 0)))
    return out


# ---- what the serial host model (tests/zstd_model_lib.py) says of a mutant --------------------------------------------------------
def serial_at(model, comp, cap):
    """(code, bytes or None) of the decode pass alone into exactly `cap` bytes in front of a guard band: the verdict the block and
    staged paths must repeat for the same capacity."""
    import ctypes

    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    out = np.full(max(cap, 0) + 64, 0xA5, dtype=np.uint8)
    total = ctypes.c_int64(-1)
    rc = int(model.zs_decode(comp.ctypes.data, comp.size, out.ctypes.data, cap, ctypes.byref(total)))
    assert np.all(out[cap:] == 0xA5), "the serial model wrote past its destination"
    return rc, (out[:total.value].copy() if rc == 0 else None)


def size_pass(model, comp):
    """(code, decoded size) of the size pass alone (it copies nothing, so it cannot see a match that reaches in front of the frame)."""
    import ctypes

    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    total = ctypes.c_int64(-1)
    rc = int(model.zs_decoded_size(comp.ctypes.data, comp.size, ctypes.byref(total)))
    return rc, total.value


def serial_free(model, comp):
    """(code, bytes or None) with all the room the partition asks for: the size pass, then the decode pass into exactly that size
    (what a stream, which has no capacity of the whole, is held against)."""
    import ctypes

    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    total = ctypes.c_int64(-1)
    rc = int(model.zs_decoded_size(comp.ctypes.data, comp.size, ctypes.byref(total)))
    if rc != 0:
        return rc, None
    assert total.value <= 64 << 20, "a mutant of a few hundred KiB that decodes to %d bytes" % total.value
    rc, out = serial_at(model, comp, total.value)
    assert rc != 0 or out.size == total.value, "size pass and decode pass disagree"
    return rc, out
