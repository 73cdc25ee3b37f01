"""Snappy block sizes above 32 KiB (spark.io.compression.snappy.blockSize 64k .. 32m), run on the CPU: the COMPILED map-side
kernels (64 KiB fragments; chunks above one fragment cut into fragment items) and the compiled batch decoder, through the
interpreter of tests/isa/gfx950_emu.py, compared with the oracle (libsnappy 1.1.8's RawCompress restated)."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "spark-s3-shuffle_amd"))
import corpus  # noqa: E402
import framing  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None,
                                reason="hipcc not available")

FRAG_SIZES = [32769, 49152, 65535, 65536]


def _wide_rows(n, seed):
    from s3shuffle import datagen

    d, _ = datagen.tpcds_wide_map_output(n + 4096, 1, seed=seed)
    return np.ascontiguousarray(d[:n])


def _far_matches(n, rng):
    """random bytes whose blocks come back about 60 000 bytes later (zeros between: few table inserts in between)"""
    a = np.zeros(n, np.uint8)
    head = rng.integers(0, 256, 4000, dtype=np.uint8)
    a[:4000] = head
    at = min(60000, n - 4100)
    a[at:at + 4000] = head
    a[at + 4000:] = rng.integers(0, 256, n - at - 4000, dtype=np.uint8)
    return a


def _data(kind, n, rng):
    if kind == "terasort":
        return corpus.chunk_corpus(7, n, rng)
    if kind == "wide":
        return _wide_rows(n, int(rng.integers(1 << 20)))
    if kind == "random":
        return corpus.chunk_corpus(0, n, rng)
    if kind == "zeros":
        return corpus.chunk_corpus(1, n, rng)
    return _far_matches(n, rng)


def _copy_offsets(block):
    """offsets of the copy elements of a raw snappy block"""
    b, i = bytes(block), 0
    while b[i] & 0x80:
        i += 1
    i += 1
    offs = []
    while i < len(b):
        t = b[i]
        ty = t & 3
        if ty == 0:
            n = t >> 2
            if n >= 60:
                nb = n - 59
                n = int.from_bytes(b[i + 1:i + 1 + nb], "little")
                i += nb
            i += 1 + n + 1
        elif ty == 1:
            offs.append(((t >> 5) << 8) | b[i + 1])
            i += 2
        elif ty == 2:
            offs.append(int.from_bytes(b[i + 1:i + 3], "little"))
            i += 3
        else:
            offs.append(int.from_bytes(b[i + 1:i + 5], "little"))
            i += 5
    return offs


@pytest.mark.parametrize("windows", [True, False], ids=["windows", "batch"])
def test_single_fragments_match_libsnappy(oracle, windows):
    """the compiled snappy_compress_kernel on fragments of 32 KiB + 1 .. 64 KiB: bit-exact with snappy_compress_block"""
    import snappy_big_blocks as sb

    rng = np.random.default_rng(90 + windows)
    kinds = ["terasort", "wide", "random", "zeros", "far"]
    frags = [_data(k, n, rng) for k in kinds for n in FRAG_SIZES]
    far_ref = bytes(oracle.snappy_compress_block(frags[-1]))
    assert max(_copy_offsets(far_ref)) > 55000, "the far-match corpus must reach about 60 000 bytes back"
    got = sb.compress_fragments(frags, windows=windows)
    for k, (c, g) in enumerate(zip(frags, got)):
        ref = bytes(oracle.snappy_compress_block(c))
        assert g == ref, "fragment %s / %d bytes differs from libsnappy" % (kinds[k // len(FRAG_SIZES)], c.size)


@pytest.mark.parametrize("block", [65537, 131072, 200000, 1 << 20])
def test_multi_fragment_chunks_match_oracle(oracle, block):
    """chunks above one fragment: head item + fragment items, scan, gather -> the .data image of SnappyOutputStream"""
    import snappy_big_blocks as sb

    rng = np.random.default_rng(block)
    big = block > (1 << 18)
    parts = [
        _data("terasort", block + 70000 if not big else 70000, rng).tobytes(),  # a chunk above and a remainder above 64 KiB
        b"",
        _data("random", block + 1000, rng).tobytes(),                          # remainder of one small chunk
        _data("wide", 3000, rng).tobytes(),
        _data("zeros", block if not big else block + 65537, rng).tobytes(),
        _data("far", 2 * 65536 + 11, rng).tobytes(),
    ]
    if big:
        parts.append(_data("wide", block, rng).tobytes())  # a whole 1 MiB chunk of match-dense rows: 16 fragments
    data = np.frombuffer(b"".join(parts), np.uint8)
    offsets = np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
    ref_img, ref_index, _ = oracle.compress_map_output(oracle.CODEC_SNAPPY, 0, data, offsets, block_size=block)
    st, img, index = sb.compress_map_output(parts, block, len(ref_img))
    assert st == 0
    assert index == [int(x) for x in ref_index]
    assert img == bytes(ref_img)


def test_batched_tails_with_fragment_items(oracle):
    """the batched tails (TaskTail) give every task what the single-task call gives, head items included"""
    import snappy_big_blocks as sb

    rng = np.random.default_rng(7)
    block = 131072
    tasks = [[_data("terasort", 140000, rng).tobytes(), _data("random", 70000, rng).tobytes()],
             [b"", _data("zeros", 300000, rng).tobytes(), _data("wide", 9000, rng).tobytes()]]
    refs = []
    for parts in tasks:
        data = np.frombuffer(b"".join(parts), np.uint8)
        offsets = np.cumsum([0] + [len(p) for p in parts]).astype(np.int64)
        refs.append(oracle.compress_map_output(oracle.CODEC_SNAPPY, 0, data, offsets, block_size=block))
    res = sb.compress_map_outputs_batch(tasks, block, [len(r[0]) for r in refs])
    for (st, img, index), (ref_img, ref_index, _) in zip(res, refs):
        assert st == 0 and index == [int(x) for x in ref_index] and img == bytes(ref_img)


def _hand_blocks(rng):
    """valid blocks other writers may produce: copy-4 tags, far offsets, literal tags 62 / 63"""
    base = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    # offsets 3 000 / 40 000 / 65 000 as copy-2 and copy-4 elements
    els = [("lit", base[:66000])]
    for off, kind in [(3000, 2), (40000, 2), (65000, 2), (3000, 4), (40000, 4), (65000, 4), (65999, 4)]:
        els += [("copy", off, 64, kind), ("lit", base[66000:66003]), ("copy", off, 7, kind)]
    blocks = [framing.snappy_block(els)]
    # literal tags 62 (3 length bytes) and 63 (4 length bytes), short and long
    lit = rng.integers(0, 256, 50000, dtype=np.uint8).tobytes()
    blocks.append(framing.snappy_block([("lit", lit[:100])], force_len_bytes=3))
    blocks.append(framing.snappy_block([("lit", lit)], force_len_bytes=3))
    blocks.append(framing.snappy_block([("lit", lit[:45000])], force_len_bytes=4))
    # tag-63 literals throughout: a long one, a copy-4 30 000 bytes back, then a long run of short elements
    els = [("lit", lit[:40000]), ("copy", 30000, 64, 4)]
    els += [("lit", lit[k:k + 5]) if k % 2 else ("copy", 1000 + k, 9, 1 if 1000 + k < 2048 else 2) for k in range(1, 400)]
    blocks.append(framing.snappy_block(els, force_len_bytes=4))
    return blocks


def test_compiled_batch_decoder_takes_big_snappy_chunks(oracle):
    """decode_blocks(fmt=1): oracle-written chunks of 40 000 .. 1 MiB and hand-built blocks decode byte for byte (before ABI 9
    every chunk above 32 KiB came back S3S_E_UNSUPPORTED)"""
    import decode_kernel as dk

    rng = np.random.default_rng(11)
    datas = [_data("terasort", 40000, rng), _data("wide", 65536, rng), _data("far", 150000, rng),
             np.concatenate([_data("wide", 1 << 19, rng), _data("random", 1 << 18, rng), _data("terasort", 1 << 18, rng)])]
    blocks = [(bytes(oracle.snappy_compress_block(d)), d.tobytes()) for d in datas]
    for b in _hand_blocks(rng):
        want = framing.snappy_decode_py(b, max_out=1 << 22)
        assert want is not None
        blocks.append((b, want))
    res, st, _ = dk.decode_blocks([(b, len(w)) for b, w in blocks], fmt=1)
    assert st == 0, "status %d" % st
    for k, ((b, w), r) in enumerate(zip(blocks, res)):
        assert r == w, "block %d (%d bytes) decodes wrongly" % (k, len(w))


def test_compiled_batch_decoder_refuses_a_copy_in_front_of_a_big_chunk(oracle):
    """a 45 000-byte block whose copy 40 KB in reaches in front of the chunk: a failure status, not a fault or garbage"""
    import decode_kernel as dk

    rng = np.random.default_rng(12)
    lit = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    for kind in (2, 4):
        bad = framing.snappy_block([("lit", lit), ("copy", 40001, 64, kind), ("lit", lit[:4936])])
        res, st, _ = dk.decode_blocks([(bad, 45000)], fmt=1)
        assert st == -3, "status %d" % st
