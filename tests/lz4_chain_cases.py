"""Inputs for the window block's chain (lz4_window_engine.inc: the next window's duplicate-hash passes run during the current
window; the layout of the run loop): TEST INFRASTRUCTURE shared by tests/test_isa_lz4_chain.py (interpreter) and
tests/test_gpu_lz4_chain.py (hardware).  Every case is a list of chunks of 1 - 4 KiB (one LZ4 block each); the block runs whole
windows from position 64 to 448 bytes in front of a chunk's end, so each chunk gives it 9 - 57 windows.
"""
import numpy as np

from lz4_ring_cases import planted

NEAR = (24, 40, 72, 130, 260)


def period64():
    """a 64-byte pattern repeated, with one byte changed per period (at a position that moves): every lane of a window hashes
    to the slot the same lane of the previous window hashed to, so a window's commit, the early passes of the next window and
    their roll-back all meet in the same slots; matches (offset 64, 128, ..) end at the changed byte, one or two per window"""
    rng = np.random.default_rng(700)
    out = []
    for n, step in ((2048, 23), (4096, 37), (1024, 5)):
        pat = rng.integers(0, 256, 64, dtype=np.uint8)
        a = np.tile(pat, n // 64 + 1)[:n].copy()
        k = 70
        while k < n:
            a[k] = (int(a[k]) + 1 + k % 7) & 0xff
            k += 64 + step if (k // 64) % 3 else 29 + step
        out.append(a)
    return out


def byte_runs():
    """runs of one byte (every lane of a run has the same hash) that start late in a window and reach into the next one, where
    the offset-1 match has made their lanes dead; the same four bytes again further down that window: a live lane whose only
    partners are dead - the early passes flag it, the old ones did not"""
    out = []
    for seed, x in ((710, 0x5a), (711, 0x00)):
        a = planted(3072, seed, NEAR, lit=(4, 8))
        for w in range(3, 40, 4):  # run from lane 50 of window w to lane 20 of window w + 1; the four bytes again at lane 40
            a[64 * w + 50: 64 * w + 84] = x
            a[64 * w + 84] = x ^ 0xff
            a[64 * w + 104: 64 * w + 108] = x
        out.append(a)
    return out


def ip_minus_2():
    """matches that leave their window with ip - 2 in its last two lanes, in the next window (first and last lane) and two
    windows ahead"""
    at = []
    for k, ln in enumerate((34, 35, 36, 37, 99, 100, 162, 163, 164, 200, 226, 227)):
        at.append((64 * (4 + 5 * k) + 30, 24 + 16 * (k % 3), ln))  # ip = 64 w + 30: ipe - 2 = 64 w + 32 + ln
    return [planted(4096, 720, NEAR, at=at), planted(4096, 721, (24, 40, 72), at=[(p + 64, o + 8, ln) for p, o, ln in at])]


def no_event():
    """windows without any event (64 and more random bytes behind a match, fewer than 48 probes into the run) and windows
    whose run ends in them without a match"""
    rng = np.random.default_rng(730)
    a = planted(4096, 731, NEAR)
    for w in range(4, 56, 5):
        n = 66 + 3 * (w % 7)
        a[64 * w + 10: 64 * w + 10 + n] = rng.integers(0, 256, n, dtype=np.uint8)
    return [a]


def hand_back_and_skip():
    """a near match of 244 .. 259 bytes (the ring covers 240: handed back in mid-window, when the next window's passes have
    run and are not rolled back by a commit; one of 300 bytes, which every build hands back) and matches that skip exactly
    one window (the window whose passes ran is not the one that runs next)"""
    at = []
    for k, ln in enumerate((244, 250, 259, 100, 110, 300, 120, 259)):
        at.append((64 * (5 + 7 * k) + 20 + 3 * k, 130 + 40 * k, ln))
    return [planted(4096, 740, NEAR, at=at)]


def lengths():
    """the block stops 448 bytes in front of the chunk's end: chunk lengths 448 + 64 k - 1, + 0, + 1"""
    return [planted(448 + 64 * k + d, 750 + 3 * k + d, NEAR) for k in (1, 9, 30) for d in (-1, 0, 1)]


def generated(n=3):
    """n TeraSort and n wide-row blocks of 32 KiB from the bench generators (the blocks of tests/tools/block_profile.py)"""
    from s3shuffle import datagen

    out = {}
    for name, gen, seed in (("terasort", datagen.terasort_map_output, 2), ("tpcds-wide", datagen.tpcds_wide_map_output, 3)):
        data, offs = gen(8 << 20, 12, seed=seed, map_id=0)
        data = np.asarray(data, dtype=np.uint8)
        p0 = int(offs[3])
        out[name] = [data[p0 + k * 32768: p0 + (k + 1) * 32768].copy() for k in range(n)]
    return out


CRAFTED = {"period64": period64, "byte_runs": byte_runs, "ip_minus_2": ip_minus_2, "no_event": no_event,
           "hand_back_and_skip": hand_back_and_skip, "lengths": lengths}
