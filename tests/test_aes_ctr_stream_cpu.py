"""CPU: streams under IO encryption (s3s_dstream_open_encrypted).  The ownership arithmetic of the window form of the AES-CTR
pass (aes_ctr_stream_core.h: which units a 16-byte chunk of a window owns) on the host, held against keystream(offset, len) of
aes_ctr_core.h for every window of small random ranges; the same through an ASan + UBSan program with heap buffers of exactly
the window's size; a window whose partition began more than 2^36 bytes in front of it.  And the surface: the symbol in the
header, exported and bound; the contract's new rules in the header's text."""
import ctypes
import os
import re

import numpy as np
import pytest

import aes_ctr_model_lib as acm
import aes_ctr_stream_model_lib as awm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
KEYS = {16: bytes(range(16)), 24: bytes(range(100, 124)), 32: bytes(range(7, 39))}


def _tables():
    """1 .. 6 partitions of 0 .. 80 stored bytes; every table has an empty partition and one of exactly 16 bytes (an empty
    stream) unless it has a single partition; partitions of 1 .. 15 bytes (shorter than an IV) occur too."""
    rng = np.random.default_rng(1616)
    out = []
    for t in range(7):
        n = t % 6 + 1
        sizes = [int(x) for x in rng.integers(0, 81, n)]
        if n >= 3:
            sizes[int(rng.integers(0, n))] = 0
            sizes[int(rng.integers(0, n))] = 16
        out.append(sizes)
    out.append([16, 0, 80, 7, 33, 17])
    assert any(0 < s < 16 for sizes in out for s in sizes)
    return out


def _range(sizes, key, seed):
    """-> (index, stored bytes, plain bytes of every partition or None where it has no whole IV)"""
    rng = np.random.default_rng(seed)
    index = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    stored = rng.integers(0, 256, int(index[-1]), dtype=np.uint8)
    plain = []
    for p, s in enumerate(sizes):
        body = stored[index[p]:index[p + 1]]
        plain.append(acm.xor_stream(key, body[:16].tobytes(), body[16:]) if s >= 16 else None)
    return index, stored, plain


def _starts(index):
    """where a window may start: never inside an IV (or inside a partition shorter than one)"""
    for p in range(len(index) - 1):
        a, b = int(index[p]), int(index[p + 1])
        if b > a:
            yield a
            yield from range(a + 16, b)


def _expect(index, stored, plain, start, end):
    """-> (plain bytes of the window, per stored byte how often it must be touched, {piece: IV} of the IVs whole in it)"""
    cur, E, front = awm.pieces(index, start, end)
    out, cover, ivs = [], np.zeros(end - start, np.uint8), {}
    for i in range(len(E) - 1):
        p = cur + i
        a, b = int(index[p]), int(index[p + 1])
        lo, hi = max(a, start), min(b, end)
        if b - a < 16:
            continue  # empty, or shorter than an IV: nothing
        if lo == a:
            if hi - lo < 16:
                continue  # the window's end cuts the IV
            ivs[i] = stored[a:a + 16]
            cover[lo - start:lo - start + 16] = 1
            lo += 16
        out.append(plain[p][lo - a - 16:hi - a - 16])
        cover[lo - start:hi - start] = 1
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), cover, ivs


def _all_windows(index):
    total = int(index[-1])
    return [(s, e) for s in _starts(index) for e in range(s + 1, total + 1)]


@pytest.mark.parametrize("t", range(8))
def test_every_window_of_small_ranges(t):
    sizes = _tables()[t]
    key = KEYS[(16, 24, 32)[t % 3]]
    index, stored, plain = _range(sizes, key, 50 + t)
    windows = _all_windows(index)
    assert windows
    residues = set()
    for start, end in windows:
        cur, E, front = awm.pieces(index, start, end)
        Q = awm.plain_offsets(index, cur, E, front)
        iv0 = stored[index[cur]:index[cur] + 16] if front > 0 else np.zeros(16, np.uint8)
        want, want_cover, want_ivs = _expect(index, stored, plain, start, end)
        assert Q[-1] == want.size, (sizes, start, end)
        # tiles of 2 chunks put a tile end every 32 bytes; the kernel's 1024 is one tile here
        for tile_chunks in (2, 1024):
            got, ivs, cover, blocks = awm.window(key, iv0, stored[start:end], E, Q, front, tile_chunks)
            assert np.array_equal(cover, want_cover), (sizes, start, end, tile_chunks)  # every byte once; cut IVs and short partitions never
            assert np.array_equal(got, want), (sizes, start, end, tile_chunks)
            for i, iv in want_ivs.items():
                assert np.array_equal(ivs[i], iv)
            # a unit costs one block encryption: never more units than chunks plus one per partition boundary
            assert blocks <= (end - start + 15) // 16 + len(E) + 1
        residues.add(front % 16 if front else -1)
    if max(sizes) >= 32:
        assert residues >= set(range(16)), "a window start on every residue of a key stream block"


def test_asan_ubsan_heap_buffers_of_exactly_the_window(tmp_path):
    cases, wants = [], []
    for t, sizes in enumerate(_tables()):
        key = KEYS[(16, 24, 32)[t % 3]]
        index, stored, plain = _range(sizes, key, 50 + t)
        for start, end in _all_windows(index)[t % 5::5]:
            cur, E, front = awm.pieces(index, start, end)
            Q = awm.plain_offsets(index, cur, E, front)
            iv0 = stored[index[cur]:index[cur] + 16] if front > 0 else np.zeros(16, np.uint8)
            cases.append((key, iv0.tobytes(), stored[start:end], E, Q, front, 2 if (start + end) % 2 else 1024))
            wants.append(_expect(index, stored, plain, start, end))
    assert len(cases) > 2000
    for (got, ivs, cover), (want, want_cover, want_ivs) in zip(awm.run_asan(cases, str(tmp_path)), wants):
        assert np.array_equal(got, want) and np.array_equal(cover, want_cover)
        assert all(np.array_equal(ivs[i], iv) for i, iv in want_ivs.items())


@pytest.mark.parametrize("key_bytes", [16, 32])
def test_partition_began_2_to_the_36_in_front_of_the_window(key_bytes, tmp_path):
    """the first piece's block numbers are above 2^32; an IV of ff..ff makes the counter's carry run through all 16 bytes"""
    key = KEYS[key_bytes]
    rng = np.random.default_rng(36)
    for iv0, front in ((bytes([0xFF] * 16), (1 << 36) + 48 + 5), (bytes(rng.integers(0, 256, 16, dtype=np.uint8)), (1 << 36) + (1 << 33) + 16 + 11),
                       (bytes([0] * 8 + [0xFF] * 7 + [0xF0]), (1 << 36) + 48)):
        assert (front - 16) // 16 > 1 << 32
        win = rng.integers(0, 256, 100 + 16 + 40, dtype=np.uint8)  # 100 bytes of the far partition, then a whole partition of 56
        E, Q = [0, 100, 156], [0, 100, 140]
        want = np.concatenate([np.frombuffer(acm.keystream(key, iv0, front - 16, 100), np.uint8) ^ win[:100],
                               acm.xor_stream(key, win[100:116].tobytes(), win[116:])])
        got, ivs, cover, blocks = awm.window(key, iv0, win, E, Q, front)
        assert np.array_equal(got, want) and np.all(cover == 1) and np.array_equal(ivs[1], win[100:116])
        assert blocks == (100 + (front % 16) + 15) // 16 + 1 + 3  # the far piece's blocks, the IV, ceil(40 / 16)
        (got2, ivs2, cover2), = awm.run_asan([(key, iv0, win, E, Q, front, 1024)], str(tmp_path))
        assert np.array_equal(got2, want) and np.all(cover2 == 1)


# ---- the surface -----------------------------------------------------------------------------------------------------------
def _header():
    with open(HEADER) as f:
        return f.read()


def test_symbol_in_header_exported_and_bound():
    import s3shuffle
    from s3shuffle import codec as C

    h = _header()
    m = re.search(r"int s3s_dstream_open_encrypted\(([^;]*)\);", h)
    plain = re.search(r"int s3s_dstream_open\(([^;]*)\);", h)
    assert m and plain and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", plain.group(1))  # the same arguments
    assert re.search(r"#define S3S_ABI_VERSION 11\b", h)
    lib = s3shuffle.load_library()
    assert lib.s3s_abi_version() == 11
    assert hasattr(lib, "s3s_dstream_open_encrypted")
    assert lib.s3s_dstream_open_encrypted.argtypes == lib.s3s_dstream_open.argtypes and lib.s3s_dstream_open_encrypted.argtypes is not None
    assert ctypes.sizeof(C.StreamResult) == 40
    import inspect

    assert "encrypted" in inspect.signature(C.DecodeStream.__init__).parameters
    assert inspect.signature(C.Codec.decode_stream).parameters["encrypted"].default is False


def test_header_states_the_iv_unit_and_key_binding_rules():
    h = re.sub(r"\s*\n \*\s*", " ", _header())
    assert "the 16-byte IV of a non-empty partition is a unit" in h
    assert "consumed only when all 16 bytes are in the window" in h
    assert "consumed = 0, need_comp = 16" in h
    assert "never inside an IV" in h
    assert "bound to the key setting it was opened under" in h
    assert "its feeds answer S3S_E_INVALID" in h and "No key material is copied into the stream" in h
    assert "1 .. 15 stored bytes is S3S_E_BAD_FRAME" in h
    assert "one more window-sized buffer" in h  # the memory bound
    # the plain open still refuses, and says where to go
    assert "s3s_dstream_open_encrypted is the opt-in" in h
