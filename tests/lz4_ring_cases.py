"""Inputs for the LZ4 input-ring kernel (S3S_OPT_LZ4_VARIANT 11, lz4_compress_ring_kernel): TEST INFRASTRUCTURE shared by
tests/test_isa_lz4_ring.py (interpreter) and tests/test_gpu_lz4_ring.py (hardware).

The window block keeps the last 4 KiB of its input in LDS (position q at ring address q & 0xfff) and serves a match extension
from it when the offset is below SPAN; ahead of the probe the ring covers COVER bytes behind ip + 4.  Every case is a list
of chunks (one LZ4 block each) built so that matches the greedy parse finds sit on those edges.
"""
import numpy as np

SPAN = 3712          # S3S_RING_SPAN: offsets below it are served from the ring
COVER = 240          # bytes behind ip + 4 the ring path compares (lanes 0..59)
RING = 4096          # the ring's wrap: positions that are multiples of it
BLOCK = 32768


def planted(n, seed, offsets, at=(), mlen=(16, 40), lit=(5, 12)):
    """n bytes: random literals (lit) and copies (mlen bytes, from one of `offsets` back), which LZ4's greedy parse finds as
    matches close enough to each other that the window block keeps running.  at: (position, offset, length) copies placed
    exactly there (literals are stretched to reach the position); the byte behind such a copy differs from the byte that
    would continue it, so its match length is exactly `length`."""
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(0, 256, 8, dtype=np.uint8).tobytes())
    todo = sorted(at)

    def copy(off, ln):
        for _ in range(ln):
            out.append(out[-off])

    while len(out) < n:
        nl = int(rng.integers(lit[0], lit[1] + 1))
        if todo and len(out) + nl + mlen[1] >= todo[0][0]:
            pos, off, ln = todo.pop(0)
            if pos < len(out) + 1 or off > pos:
                continue
            while pos - len(out) > 14:  # short records up to the position: no literal run the block would hand back
                out += rng.integers(0, 256, 5, dtype=np.uint8).tobytes()
                copy(min(24, len(out)), min(16, pos - len(out) - 6))
            out += rng.integers(0, 256, pos - len(out), dtype=np.uint8).tobytes()
            if off < pos:  # the byte in front of the copy differs from the one in front of its source: no backward extension
                out[-1] = (out[-1 - off] + 1) & 0xff
            copy(off, ln)
            out.append((out[-off] + 1) & 0xff)
            continue
        out += rng.integers(0, 256, nl, dtype=np.uint8).tobytes()
        offs = [o for o in offsets if o <= len(out)]
        if offs:
            copy(int(offs[int(rng.integers(0, len(offs)))]), int(rng.integers(mlen[0], mlen[1] + 1)))
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8).copy()


NEAR = (24, 40, 72, 130, 260)             # keeps the block running
MID = (700, 1500, 2300, 3100, 3600)       # inside the ring, far from the probe: a stale ring would show


def span_edge():
    """sources SPAN - 1, SPAN and SPAN + 1 bytes back (ring / global loads / global loads), in the early issue and in the run loop"""
    return [planted(BLOCK, 100 + k, NEAR + (off, off, off), at=[(4200 + 600 * j, off, 30) for j in range(40)])
            for k, off in enumerate((SPAN - 1, SPAN, SPAN + 1))]


def wrap():
    """the ip side and the source side straddling the ring's wrap point, aligned and at every byte phase"""
    at = []
    for k in range(1, 8):
        at.append((RING * k - 10 - k % 4, 100 + k, 40))            # ip side across position 4096 k
        at.append((RING * k + 300 + k % 4, 310 + 2 * (k % 4), 40))  # source side across it
        at.append((RING * k + 700, 700 - 2, 30))                   # source side: its pair's high dword is the ring's first
    return [planted(BLOCK, 110, NEAR + MID, at=at)]


def coverage_edge():
    """a match longer than the ring holds ahead (300), one that ends exactly at the covered edge (and one byte to either
    side), and a 4 KiB run of one byte (offset 1)"""
    at = [(5000, 500, 300), (9000, 900, 4 + COVER - 1), (11000, 1200, 4 + COVER), (13000, 800, 4 + COVER + 1),
          (15000, 2000, 4 + COVER - 4), (21500, 3000, 100)]
    a = planted(BLOCK, 120, NEAR + MID, at=at)
    b = planted(BLOCK, 121, NEAR + MID)
    b[16000:16000 + 4096] = 0x5a
    return [a, b]


def hand_back():
    """events the block hands back (a literal run of 15 or more, a match code of 270 or more, more than 48 probes without a
    match), each followed by matches whose sources lie on both sides of the place the block was left at"""
    rng = np.random.default_rng(130)
    a = planted(BLOCK, 131, NEAR + MID)
    for p in range(6000, 30000, 3000):  # literal runs of 15 .. 40 bytes
        a[p:p + 15 + (p // 3000) * 3] = rng.integers(0, 256, 15 + (p // 3000) * 3, dtype=np.uint8)
    b = planted(BLOCK, 132, NEAR + MID, at=[(6000 + 4000 * j, 1000 + 300 * j, 274 + 40 * j) for j in range(6)])
    c = planted(BLOCK, 133, NEAR + MID)
    for p in range(5000, 30000, 5000):  # stretches without a match: 300 .. 1 500 random bytes
        c[p:p + 300 * (p // 5000)] = rng.integers(0, 256, 300 * (p // 5000), dtype=np.uint8)
    return [a, b, c]


def short_history():
    """the first window the block runs (history shorter than the ring) and candidates in the first four bytes of the chunk"""
    at = [(70, 70, 30), (130, 128, 30), (200, 199, 20), (300, 297, 33), (420, 60, 50)]
    return [planted(BLOCK, 140, (8, 24, 40, 72), at=at, lit=(4, 8))]


def lengths():
    """511 and 512 (the block runs from 512 bytes on), 32 767, 32 768, and 65 535 (ring positions wrap sixteen times)"""
    return [planted(n, 150 + k, NEAR + MID) for k, n in enumerate((511, 512, 32767, 32768, 65535))]


def end_of_allocation():
    """a chunk that ends its allocation, with matches up to its last bytes"""
    return [planted(BLOCK, 160, NEAR + MID, at=[(BLOCK - 500, 3000, 200), (BLOCK - 200, 1000, 150), (BLOCK - 40, 24, 30)])]


def generated():
    """four TeraSort and four wide-row blocks from the bench generators"""
    from s3shuffle import datagen

    out = []
    for gen, seed in ((datagen.terasort_map_output, 2), (datagen.tpcds_wide_map_output, 3)):
        data, offs = gen(8 << 20, 12, seed=seed, map_id=0)
        data = np.asarray(data, dtype=np.uint8)
        p0 = int(offs[3])
        out += [data[p0 + k * BLOCK: p0 + (k + 1) * BLOCK].copy() for k in range(4)]
    return out


CASES = {"span_edge": span_edge, "wrap": wrap, "coverage_edge": coverage_edge, "hand_back": hand_back,
         "short_history": short_history, "lengths": lengths, "end_of_allocation": end_of_allocation, "generated": generated}
