"""Inputs of the IO encryption tests (tests/test_gpu_io_encryption.py; their CPU-side properties are checked in
tests/test_aes_ctr_model.py): small enough for seconds on the GPU, shaped so that the AES-CTR kernel cannot hide a mistake."""
import numpy as np

TILE = 16384  # stored bytes one workgroup of the AES-CTR kernel handles (aes_ctr.hip: kCtrTile)

KEYS = {kb: np.random.default_rng(1000 + kb).bytes(kb) for kb in (16, 24, 32)}
IV_ONES = b"\xff" * 16                            # block 1 wraps to 00..00
IV_LOW_CARRY = bytes(8) + b"\xff" * 7 + b"\xf0"   # the low eight bytes carry into byte 7 after 16 blocks (256 stream bytes)


def words_input(seed=7):
    """20 partitions of words text (a small vocabulary: every codec finds matches), empties among them, sizes from a few
    bytes to ~30 KiB so that the compressed partitions start at assorted residues mod 16.  (data uint8, offsets int64[21])"""
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.integers(97, 123, int(rng.integers(2, 11)), dtype=np.uint8)) for _ in range(300)]
    sizes = [0, 5, 1000, 0, 17, 3001, 12000, 33000, 0, 0, 1, 4097, 700, 15, 16, 9000, 0, 2222, 31, 6001]
    parts = []
    for s in sizes:
        words = [vocab[i] for i in rng.integers(0, len(vocab), s // 3 + 2)]
        parts.append(np.frombuffer(b" ".join(words)[:s], dtype=np.uint8))
    data = np.concatenate(parts).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    assert offs[-1] == sum(sizes)
    return data, offs


def none_sizes_input(seed=8):
    """Codec NONE: partitions of 1, 15, 16, 17, 31, 4095, 4096, 4097 and 70 000 bytes (empties between them), so that streams
    end on and across 16-byte units, 4 KiB and the kernel's tile edges; then four more laid out against the 16 KiB tile itself:
    a stream that ends exactly on a tile edge, the next one's IV starting on it, and an IV that straddles an edge."""
    sizes = [1, 0, 15, 16, 17, 0, 0, 31, 4095, 4096, 4097, 70000]
    stored = sum(s + 16 for s in sizes if s)
    pad = (-stored - 16) % TILE          # this partition's stream ends exactly on a tile edge
    sizes += [pad if pad else TILE, TILE - 16 - 5, 100, 3]   # ... the next one's IV starts there and ITS successor's IV straddles the next edge
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, sum(sizes), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return data, offs


def ivs_for(offs, seed=3):
    """One IV per partition (empty ones included); the first two non-empty partitions of at least 300 bytes get the IVs whose
    counters carry: ff..ff and 00..00 ff..ff ff..f0."""
    n = len(offs) - 1
    ivs = np.frombuffer(np.random.default_rng(seed).bytes(16 * n), dtype=np.uint8).reshape(n, 16).copy()
    special = [IV_ONES, IV_LOW_CARRY]
    for p in range(n):
        if special and offs[p + 1] - offs[p] >= 300:
            ivs[p] = np.frombuffer(special.pop(0), dtype=np.uint8)
    assert not special or n < 3
    return ivs.reshape(-1)
