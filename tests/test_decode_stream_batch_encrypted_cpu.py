"""CPU: the batched feed under IO encryption.  The decrypt pass of all windows of a call - aes_ctr_window_batch_kernel<10>,
COMPILED for gfx950 - run through the instruction interpreter (tests/isa/stream_batch_encrypted_kernel.py), three and four
windows per launch, from the descriptors and the tile -> window map the host builds.  Every stored window is a buffer of
exactly L bytes and every plain destination one of exactly PL bytes, so a byte touched outside them faults; what comes out is
held against keystream(offset, len) of the AES-CTR model (tests/aes_ctr_model_lib.py, itself held against the vectors of
SP 800-38A) and against the stored IVs.  And the surface of the read-only option key 17."""
import os
import re
import sys

import numpy as np
import pytest

import aes_ctr_model_lib as acm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa"))
import stream_batch_encrypted_kernel as sbe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
KEY = bytes(range(16))
TILE = 16384


@pytest.fixture(scope="module")
def rk():
    nr, keys = acm.expand_key(KEY)
    assert nr == 10
    return keys


def _range(sizes, seed):
    """-> (index, stored bytes, the IV of every partition of 16 bytes or more)"""
    rng = np.random.default_rng(seed)
    index = [0]
    for s in sizes:
        index.append(index[-1] + s)
    return index, rng.integers(0, 256, index[-1], dtype=np.uint8)


def _window(index, stored, cur, start, end):
    """One window [start, end) of a range whose open partition is `cur`, as the host lays it out: its pieces are partition cur,
    the partitions that start inside it and the empty ones at its end (ds::piece_count), E their stored offsets, Q the plain
    ones; a piece whose IV the window's end cuts, or whose partition is shorter than an IV, has no plain bytes.
    -> (the kernel's arguments, what it must produce: plain bytes, {piece: IV} of the IVs whole in the window)"""
    n = len(index) - 1
    assert index[cur] <= start and (start == index[cur] or start >= index[cur] + 16)
    E, Q, want, ivs = [0], [0], [], {}
    p = cur
    while p < n and (index[p] < end or index[p + 1] <= end):
        a, b = index[p], index[p + 1]
        lo, hi = max(a, start), min(b, end)
        body = np.zeros(0, np.uint8)
        if b - a >= 16 and (lo > a or hi - lo >= 16):
            iv = stored[a:a + 16].tobytes()
            if lo == a:
                ivs[p - cur] = stored[a:a + 16]
                lo += 16
            body = np.frombuffer(acm.keystream(KEY, iv, lo - a - 16, hi - lo), np.uint8) ^ stored[lo:hi]
        want.append(body)
        E.append(hi - start)
        Q.append(Q[-1] + body.size)
        p += 1
    front = start - index[cur] if cur < n else 0
    iv0 = stored[index[cur]:index[cur] + 16].tobytes() if front > 0 else bytes(16)
    args = dict(stored=stored[start:start + E[-1]], E=E, Q=Q, front=front, iv0=iv0)
    return args, (np.concatenate(want) if want else np.zeros(0, np.uint8)), ivs


def _check(rk, cases, extra_tiles=0):
    """cases: [(args, want plain, want ivs)] -> one launch; every window against what it must produce"""
    got, tile_win = sbe.decrypt_batch(rk, 10, [c[0] for c in cases], extra_tiles=extra_tiles)
    at = 0
    for i, ((args, want, want_ivs), g) in enumerate(zip(cases, got)):
        m, L = len(args["E"]) - 1, args["E"][-1]
        assert g["tiles"] == sbe.tiles_of(m, args["front"], L) and g["tile0"] == at, i
        assert tile_win[at:at + g["tiles"]] == [i] * g["tiles"], i  # the lookup changes exactly where the window's tiles end
        at += g["tiles"]
        assert g["plain"].size == want.size and np.array_equal(g["plain"], want), (i, args["E"], args["front"])
        assert np.all(g["plain_writes"] == 1), (i, "every stored byte that is not part of an IV is written exactly once")
        for p in range(m):
            if p in want_ivs:
                assert np.array_equal(g["ivs"][p], want_ivs[p]) and np.all(g["iv_writes"][p] == 1), (i, p)
            else:
                assert np.all(g["iv_writes"][p] == 0) and np.all(g["ivs"][p] == sbe.PREFILL), (i, p)  # nothing gathered where no IV starts whole
    assert at == len(tile_win)
    return got


def test_one_byte_beside_two_tiles_and_a_window_without_pieces(rk):
    """a window of 1 stored byte, one of 16 KiB + 17 (a second tile: the tile -> window lookup changes inside the grid), one with
    m == 0 between live ones (no tile; its neighbours' tiles do not move), and a workgroup behind the map's end"""
    index, stored = _range([16 + 40, TILE + 17 + 300, 64], 3)
    one = _window(index, stored, 0, 16 + 7, 16 + 8)                      # front = 23, one cipher byte
    big = _window(index, stored, 1, index[1], index[1] + TILE + 17)       # front = 0: an IV and 16 KiB + 1 cipher bytes
    none = (dict(stored=np.zeros(0, np.uint8), E=[0], Q=[0], front=0, iv0=bytes(16)), np.zeros(0, np.uint8), {})
    tail = _window(index, stored, 1, index[1] + 16 + TILE + 5, index[3])  # the rest of partition 1 and all of partition 2
    assert one[0]["E"] == [0, 1] and big[0]["E"][-1] == TILE + 17 and sbe.tiles_of(1, 0, TILE + 17) == 2
    got = _check(rk, [one, big, none, tail], extra_tiles=1)
    assert [g["tiles"] for g in got] == [1, 2, 0, 1] and [g["tile0"] for g in got] == [0, 1, 3, 3]
    got = _check(rk, [big, none, one])
    assert [g["tile0"] for g in got] == [0, 2, 2]
    # a window whose tiles end on the tile edge exactly, and one a byte longer: front's residue moves the edge
    for front_res in (0, 5):
        start = index[1] + 16 + front_res
        _check(rk, [_window(index, stored, 1, start, start + TILE - front_res), one, _window(index, stored, 1, start, start + TILE - front_res + 1)])


def test_every_residue_of_front_and_cut_ivs(rk):
    """front = 0 in one window of every launch and front >= 16 on each of the 16 residues across the others; windows whose end
    cuts an IV at 1, 15 and 16 bytes; a piece of 1 .. 15 stored bytes; a partition shorter than an IV"""
    sizes = [16 + 70, 16 + 33, 9, 16, 16 + 50]
    index, stored = _range(sizes, 11)
    residues, launches = set(), 0
    for r in range(0, 16, 3):
        cases = [_window(index, stored, 0, 0, index[1] + (1, 15, 16, 17, 16 + 33, 16 + 33 + 9)[r // 3])]  # front = 0; the end cuts partition 1's IV
        for rr in range(r, min(r + 3, 16)):
            start = 16 + 16 + rr  # block 1 of partition 0 at residue rr
            cases.append(_window(index, stored, 0, start, (index[1] + 15, index[2] - 3, index[5])[rr % 3]))
            residues.add(cases[-1][0]["front"] % 16)
            assert cases[-1][0]["front"] >= 16
        assert len(cases) in (2, 4) and cases[0][0]["front"] == 0
        if len(cases) == 2:
            cases.append(_window(index, stored, 4, index[4] + 16 + 3, index[4] + 16 + 3 + 9))  # a piece of 9 stored bytes, mid-partition
        _check(rk, cases)
        launches += 1
    assert residues == set(range(16)), "a window start on every residue of a key stream block"
    # the cut IVs contribute nothing and gather nothing
    for cut in (1, 15):
        a, want, ivs = _window(index, stored, 0, 16 + 5, index[1] + cut)
        assert a["Q"][-1] == a["Q"][-2] == 70 - 5 and 1 not in ivs and 0 not in ivs
    a, want, ivs = _window(index, stored, 0, 16 + 5, index[1] + 16)
    assert 1 in ivs and a["Q"][-1] == 70 - 5  # whole: gathered, and still no plain byte of its partition
    # pieces of 1 .. 15 stored bytes at a window's start (the open partition's last bytes), three per launch
    for n0 in range(1, 16, 3):
        _check(rk, [_window(index, stored, 0, index[1] - n, index[2]) for n in range(n0, n0 + 3)])


def test_empty_partitions_at_the_start_in_the_middle_and_at_the_end(rk):
    sizes = [0, 0, 16 + 21, 0, 0, 16 + 5, 16, 0]
    index, stored = _range(sizes, 19)
    a = _window(index, stored, 0, 0, index[8])           # empties in front, between and behind; a partition of an IV alone
    assert a[0]["E"][:3] == [0, 0, 0] and len(a[0]["E"]) == 9 and a[0]["E"][-1] == a[0]["E"][-2] and sorted(a[2]) == [2, 5, 6]
    b = _window(index, stored, 2, index[2] + 16 + 4, index[5])  # mid-partition start, the empties at its end are pieces
    assert len(b[0]["E"]) == 4 and b[0]["E"][1:] == [17, 17, 17]
    c = _window(index, stored, 3, index[3], index[7])    # the open partition is empty: front = 0 and the first IV belongs to piece 2
    assert c[0]["front"] == 0 and sorted(c[2]) == [2, 3]
    d = _window(index, stored, 7, index[8], index[8])    # an empty window that passes an empty partition: no tile
    assert d[0]["E"] == [0, 0] and sbe.tiles_of(1, 0, 0) == 0
    _check(rk, [a, b, c])
    _check(rk, [b, d, a, c])


def test_front_above_2_to_the_36(rk):
    """block numbers above 2^32 in one window of the launch, an IV of ff .. ff so that the counter's carry runs through all 16
    bytes; its neighbours are ordinary"""
    rng = np.random.default_rng(36)
    index, stored = _range([16 + 90, 16 + 30], 36)
    for iv0, front in ((bytes([0xFF] * 16), (1 << 36) + 48 + 5), (bytes(rng.integers(0, 256, 16, dtype=np.uint8)), (1 << 36) + (1 << 33) + 16 + 11)):
        assert (front - 16) // 16 > 1 << 32
        win = rng.integers(0, 256, 100 + 16 + 40, dtype=np.uint8)  # 100 bytes of the far partition, then a whole partition of 56
        want = np.concatenate([np.frombuffer(acm.keystream(KEY, iv0, front - 16, 100), np.uint8) ^ win[:100],
                               acm.xor_stream(KEY, win[100:116].tobytes(), win[116:])])
        far = (dict(stored=win, E=[0, 100, 156], Q=[0, 100, 140], front=front, iv0=iv0), want, {1: win[100:116]})
        _check(rk, [_window(index, stored, 0, 0, index[2]), far, _window(index, stored, 0, 16 + 9, index[1] + 16)])


# ---- the surface: key 17 ----------------------------------------------------------------------------------------------------------
def test_key_17_in_header_and_binding():
    from s3shuffle import codec

    header = open(HEADER).read()
    assert int(re.search(r"S3S_OPT_DSTREAM_BATCH_ENTRIES\s*=\s*(\d+)", header).group(1)) == 17 == codec.OPT_DSTREAM_BATCH_ENTRIES
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11
    keys = {int(x) for x in re.findall(r"\bS3S_OPT_[A-Z0-9_]+\s*=\s*(\d+)", header)}  # (the prose names some keys with a value too)
    assert keys == set(range(1, 18))  # additive: nothing renumbered
    section = re.sub(r"\s*\n \*\s*", " ", header[header.index("the batched feed (ABI 11"):])
    for needle in ("s3s_dstream_open_encrypted", "S3S_OPT_DSTREAM_BATCH_ENTRIES", "one plain buffer per window", "ONE launch of the window form of the AES-CTR pass"):
        assert needle in section, needle
    not_here = section[section.index("Not here"):]
    assert "encrypted" not in not_here


def test_key_17_is_refused_without_a_context(codec_lib):
    assert codec_lib.s3s_set_option(None, 17, 1) == -1 and codec_lib.s3s_get_option(None, 17) == -1
