"""GPU: Zstandard frames with history across their blocks decoded in stages (S3S_OPT_ZSTD_DECODE_STAGED = 1):
entropy per block, copies per frame.  libzstd's streaming frames and the crafted frames of tests/zstd_staged_lib.py (held
against libzstd and the serial host model on the CPU first, tests/test_zstd_staged_model.py) must complete on the staged path -
S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS counts their blocks exactly -, and whatever a call answers with the option at 1 - bytes,
return code, out_len, bad partition, batch statuses - is what the same call answers at 0.

Nothing here provokes a fault: an invalid frame is one the decoder refuses by its own checks (shown on the CPU first)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_staged_lib as S  # noqa: E402

pytestmark = pytest.mark.gpu

ZSTD = 3
ADLER, CRC = 1, 2
OPT_ZSTD_COMPRESS, OPT_VARIANT, OPT_BLOCKS, OPT_STAGED, OPT_STAGED_BLOCKS = 9, 13, 14, 15, 16
CANARY = 4096


@pytest.fixture()
def sc(gpu_codec):
    try:
        yield gpu_codec
    finally:
        gpu_codec.set_option(OPT_STAGED, 0)
        gpu_codec.set_option(OPT_VARIANT, 1)
        gpu_codec.set_option(OPT_ZSTD_COMPRESS, 0)
        gpu_codec.set_io_encryption(None)


def image_of(parts, oracle=None, algo=0):
    index = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=index[1:])
    img = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    sums = np.array([oracle.checksum(algo, p) for p in parts], np.int64) if algo else None
    return img, index, sums


def both(codec, call):
    """call() with key 15 at 1 and at 0 -> ((result, key 16, key 14), (result, key 16, key 14))"""
    res = []
    for v in (1, 0):
        codec.set_option(OPT_STAGED, v)
        assert codec.get_option(OPT_STAGED) == v
        r = call()
        res.append((r, codec.get_option(OPT_STAGED_BLOCKS), codec.get_option(OPT_BLOCKS)))
    return res


def device_call(codec, dev, ranges, algo, oracle, batch=True):
    """ranges: lists of (partition, content or None).  One batched device call (or single device calls) into destinations
    between canary bands -> [(status, out_len, bad partition, destination incl. canaries)]"""
    import s3shuffle

    args, dsts = [], []
    for parts in ranges:
        img, index, sums = image_of([p for p, _ in parts], oracle, algo)
        cap = sum(c.size for _, c in parts if c is not None) + 300
        d = dev.upload(np.full(cap + 2 * CANARY, 0xA5, np.uint8))
        dsts.append((d, cap))
        args.append((dev.upload(img), img.size, index, sums, d + CANARY, cap))
    if batch:
        res = codec.decompress_ranges_batch_device(ZSTD, algo, args, raise_on_error=False)
    else:
        res = []
        for a in args:
            try:
                res.append((0, codec.decompress_range_device(ZSTD, algo, *a), -1))
            except s3shuffle.CodecError as e:
                res.append((e.code, 0, e.partition))
    return [(st, n, bad, dev.download(d, cap + 2 * CANARY)) for (st, n, bad), (d, cap) in zip(res, dsts)]


def same_answers(r1, r0):
    assert len(r1) == len(r0)
    for (st1, n1, bad1, buf1), (st0, n0, bad0, buf0) in zip(r1, r0):
        assert (st1, n1, bad1) == (st0, n0, bad0), "the verdict depends on the option"
        assert np.all(buf1[:CANARY] == 0xA5) and np.all(buf1[buf1.size - CANARY:] == 0xA5), "canary band damaged"
        if st1 == 0:
            assert np.array_equal(buf1[CANARY:CANARY + n1], buf0[CANARY:CANARY + n0]), "the bytes depend on the option"
            assert np.all(buf1[CANARY + n1:] == 0xA5)


# ---- 1. the keys ----------------------------------------------------------------------------------------------------------------------
def test_the_keys(sc):
    lib, h = sc._lib, sc._h
    assert sc.get_option(OPT_STAGED) == 0, "the staged path is opt-in"
    sc.set_option(OPT_STAGED, 1)
    assert sc.get_option(OPT_STAGED) == 1
    assert lib.s3s_set_option(h, OPT_STAGED, 2) == -1 and lib.s3s_set_option(h, OPT_STAGED, -1) == -1
    assert sc.get_option(OPT_STAGED) == 1
    sc.set_option(OPT_STAGED, 0)
    assert sc.get_option(OPT_STAGED) == 0
    assert lib.s3s_set_option(h, OPT_STAGED_BLOCKS, 0) == -1 and lib.s3s_set_option(h, OPT_STAGED_BLOCKS, 5) == -1, "key 16 is read-only"
    assert sc.zstd_decode_staged_blocks == sc.get_option(OPT_STAGED_BLOCKS) >= 0


# ---- 2. libzstd's frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, ADLER, CRC])
def test_libzstd_frames(sc, oracle, algo):
    frames = [S.libzstd_frame(kind, flushed) for kind in S.KINDS for flushed in (False, True)]
    want = [len(S.block_headers(comp)[0]) for comp, _ in frames]
    assert sorted(set(want)) == [5, 129]
    for (comp, src), n in zip(frames, want):  # one partition each
        img, index, sums = image_of([comp], oracle, algo)
        (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, algo, img, index, sums, dst_capacity=src.size).copy())
        assert np.array_equal(o1, src) and k1 == n, "key 16 is not the header walk's block count"
        assert np.array_equal(o0, src) and k0 == 0
    img, index, sums = image_of([c for c, _ in frames], oracle, algo)  # all in one range
    content = np.concatenate([s for _, s in frames])
    (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, algo, img, index, sums, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and k1 == sum(want)
    assert np.array_equal(o0, content) and k0 == 0


# ---- 3. crafted frames ------------------------------------------------------------------------------------------------------------------
def _two_frame_partitions():
    """(f): a frame of the product's writer in front (claimed by key 13's path), and a checksum / a skippable frame behind."""
    import zstd_block_parallel_lib as Z
    import zstd_writer as W

    a, ca, na = S.crafted("c")
    b, cb, nb = S.crafted("a_ll+of+ml_fse")
    w, ws = Z.writer_frame("b+1"), Z.writer_sources()["b+1"][0]
    f = W.Frame(checksum=True)
    f.raw(b"with a checksum").raw(b" in two blocks")
    chk, cchk = f.finish()
    skip = np.frombuffer(W.skippable(b"skip me") + bytes(b), np.uint8)
    return [(np.concatenate([a, b]), np.concatenate([ca, cb]), na + nb, 0),
            (np.concatenate([w, a]), np.concatenate([ws, ca]), na, 2),
            (np.concatenate([a, np.frombuffer(chk, np.uint8)]), np.concatenate([ca, np.frombuffer(cchk, np.uint8)]), na, 0),
            (np.concatenate([a, skip]), np.concatenate([ca, cb]), na, 0)]


@pytest.mark.parametrize("algo", [0, CRC])
def test_crafted_frames(sc, oracle, algo):
    from hipdev import Dev

    valid = [S.crafted(c) for c in S.VALID_CASES]
    two = _two_frame_partitions()
    dev = Dev()
    try:
        # (a) - (e): every frame a partition of one range; every frame a range of its own (single device calls)
        parts = [(d, c) for d, c, _ in valid]
        want = sum(n for _, _, n in valid)
        (r1, k1, _), (r0, k0, _) = both(sc, lambda: device_call(sc, dev, [parts], algo, oracle))
        same_answers(r1, r0)
        assert r1[0][0] == 0 and (k1, k0) == (want, 0), "the crafted frames did not complete on the staged path"
        content = np.concatenate([c for _, c in parts])
        assert r1[0][1] == content.size and np.array_equal(r1[0][3][CANARY:CANARY + content.size], content)
        for d, c, n in valid[:3] + valid[-4:]:
            (r1, k1, _), (r0, k0, _) = both(sc, lambda: device_call(sc, dev, [[(d, c)]], algo, oracle, batch=False))
            same_answers(r1, r0)
            assert r1[0][0] == 0 and (k1, k0) == (n, 0)
        # (f): two frames in one partition
        (r1, k1, k14), (r0, k0, k14_0) = both(sc, lambda: device_call(sc, dev, [[(d, c) for d, c, _, _ in two]], algo, oracle))
        same_answers(r1, r0)
        assert r1[0][0] == 0 and (k1, k0) == (sum(n for _, _, n, _ in two), 0)
        assert k14 == k14_0 == sum(n13 for _, _, _, n13 in two), "key 14 keeps counting the block path's frames only"
        # (g): each invalid frame between two valid partitions, a range each, one batched call
        d_ok, c_ok, n_ok = S.crafted("d")
        e_ok, ce_ok, ne_ok = S.crafted("c")
        bad = [S.crafted(c)[0] for c in S.INVALID_CASES]
        ranges = [[(d_ok, c_ok), (b, None), (e_ok, ce_ok)] for b in bad] + [[(d_ok, c_ok), (e_ok, ce_ok)]]
        (r1, k1, _), (r0, k0, _) = both(sc, lambda: device_call(sc, dev, ranges, algo, oracle))
        same_answers(r1, r0)
        assert [r[0] for r in r1] == [-3] * len(bad) + [0]
        assert (k1, k0) == ((n_ok + ne_ok) * (len(bad) + 1), 0), "key 16 counts the valid neighbours, nothing of the invalid frames"
    finally:
        dev.free()


# ---- 4. the conformance corpus --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    import zstd_conformance as C

    cases = C.fixed_corpus() + [C.generated_case(seed) for seed in range(400)]
    for c in cases:
        C.arbiter(c)
    return cases


def test_conformance_corpus(sc, corpus, oracle):
    """As tests/test_gpu_zstd_conformance.py lays it out: the valid partitions inside the single pass's guesses as one image,
    all valid partitions (two passes), both again without the first partition; every partition alone; the invalid frames in
    a batched call.  Key 15 = 1 against 0, call for call."""
    from hipdev import Dev

    valid = [c for c in corpus if c.content is not None]
    inside = [c for c in valid if len(c.content) <= 8 * len(c.data) + 4096]
    assert len(valid) - len(inside) > 20
    for cases, single_pass in ((inside, True), (inside[1:], True), (valid, False), (valid[1:], False)):
        parts = [np.frombuffer(c.data, np.uint8) for c in cases]
        img, index, sums = image_of(parts, oracle, CRC)
        want = np.frombuffer(b"".join(c.content for c in cases), np.uint8)
        (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, CRC, img, index, sums, dst_capacity=want.size).copy())
        assert np.array_equal(o1, want) and np.array_equal(o0, want) and k0 == 0
        # single pass: exactly what the header walk finds - the call's staging has room for all of it (shown on the CPU:
        # tests/test_zstd_staged_model.py::test_conformance_corpus); two passes: nothing
        found = sum(S.staged_blocks(c.data) for c in cases)
        print("staged blocks", k1, "of", found)
        assert found > 400 and k1 == (found if single_pass else 0)
    sc.set_option(OPT_STAGED, 1)
    for c in valid:
        if not c.data:
            continue
        comp = np.frombuffer(c.data, np.uint8)
        out = sc.decompress_range(ZSTD, 0, comp, np.array([0, comp.size], np.int64), None, dst_capacity=len(c.content))
        assert out.tobytes() == c.content, c.name
    invalid = [c for c in corpus if c.content is None]
    dev = Dev()
    try:
        ranges = [[(np.frombuffer(c.data, np.uint8), None)] for c in invalid]
        (r1, _, _), (r0, _, _) = both(sc, lambda: device_call(sc, dev, ranges, 0, oracle))
        same_answers(r1, r0)
        assert [r[0] for r in r1] == [c.rc for c in invalid]
    finally:
        dev.free()


# ---- 5. more blocks than the entropy grid has workgroups -----------------------------------------------------------------------------
def test_more_blocks_than_the_grid(sc):
    import re

    comp, src = S.libzstd_frame(7, True, n=10 << 20)
    n_blocks = len(S.block_headers(comp)[0])
    header = open(os.path.join(S.ROOT, "spark-s3-shuffle_amd", "csrc", "zstd_decode_staged.h")).read()
    grid = int(re.search(r"constexpr int kStagedGrid = (\d+);", header).group(1))  # workgroups of the entropy grid, a documented constant
    assert n_blocks == 2561 and n_blocks > grid, "every workgroup of the entropy grid must take more than one job"
    index = np.array([0, comp.size], np.int64)
    (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, 0, comp, index, None, dst_capacity=src.size).copy())
    assert np.array_equal(o1, src) and np.array_equal(o0, src) and (k1, k0) == (n_blocks, 0)


# ---- 6. a partition that outgrows its guessed capacity --------------------------------------------------------------------------------
def test_outgrown_guess(sc, oracle):
    from oracle import zstd_ref

    zeros = np.zeros(2_000_000, np.uint8)
    comp = zstd_ref.compress_stream(zeros, 1)
    assert zeros.size > 8 * comp.size + 4096 and len(S.block_headers(comp)[0]) >= 2
    other, csrc = S.libzstd_frame(6, False)
    img, index, sums = image_of([other, comp], oracle, ADLER)
    content = np.concatenate([csrc, zeros])
    (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, ADLER, img, index, sums, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and np.array_equal(o0, content)
    assert (k1, k0) == (0, 0), "the two-pass form stays on the serial decoder"


# ---- 7. entry points and layout -------------------------------------------------------------------------------------------------------
def test_entry_points_and_layout(sc, oracle):
    from hipdev import Dev

    empty = np.zeros(0, np.uint8)
    a, sa = S.libzstd_frame(6, True)
    b, sb = S.libzstd_frame(3, False)
    na, nb = len(S.block_headers(a)[0]), len(S.block_headers(b)[0])
    # empty partitions between full ones, host buffers
    img, index, sums = image_of([empty, a, empty, empty, b, empty], oracle, CRC)
    content = np.concatenate([sa, sb])
    (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, CRC, img, index, sums, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and np.array_equal(o0, content) and (k1, k0) == (na + nb, 0)
    # 64 small partitions
    small = [S.crafted(S.VALID_CASES[i % len(S.VALID_CASES)]) for i in range(64)]
    img, index, sums = image_of([d for d, _, _ in small], oracle, ADLER)
    content = np.concatenate([c for _, c, _ in small])
    (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, ADLER, img, index, sums, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and np.array_equal(o0, content) and (k1, k0) == (sum(n for _, _, n in small), 0)
    dev = Dev()
    try:
        # the batched device entry point with three ranges, one of them invalid; destinations between canary bands
        bad = S.crafted("g_offset")[0]
        ranges = [[(a, sa), (empty, empty)], [(b, sb), (bad, None)], [(b, sb), (a, sa)]]
        (r1, k1, _), (r0, k0, _) = both(sc, lambda: device_call(sc, dev, ranges, CRC, oracle))
        same_answers(r1, r0)
        assert [r[0] for r in r1] == [0, -3, 0] and (k1, k0) == (2 * na + 2 * nb, 0)
    finally:
        dev.free()
    # a host-buffer batch
    keep = [np.ascontiguousarray(x) for x in (a, b)]
    images = [image_of([x], oracle, CRC) for x in keep]
    for v in (1, 0):
        sc.set_option(OPT_STAGED, v)
        houts = [np.zeros(s.size, np.uint8) for s in (sa, sb)]
        res = sc.decompress_ranges_batch(ZSTD, CRC, [(k.ctypes.data, k.size, i[1], i[2], o.ctypes.data, o.size) for k, i, o in zip(keep, images, houts)])
        for s, (st, n, _), o in zip((sa, sb), res, houts):
            assert st == 0 and n == s.size and np.array_equal(o, s)
        # (both ranges fit one group of the host-buffer pipeline: one device call, whose count this is)
        assert sc.zstd_decode_staged_blocks == (na + nb if v else 0)


def test_under_io_encryption(sc, oracle):
    """A libzstd image encrypted by the reference layer: the staged path reads the decrypted workspace like the serial decoder."""
    import io_encryption_inputs as I
    import spark_crypto_ref as R

    a, sa = S.libzstd_frame(2, True)
    b, sb = S.libzstd_frame(7, False)
    img, index, _ = image_of([a, np.zeros(0, np.uint8), b])
    key = I.KEYS[16]
    e_img, e_index, e_sums = R.encrypt_map_output(img, index, key, I.ivs_for(index), ADLER)
    sc.set_io_encryption(key)
    content = np.concatenate([sa, sb])
    (o1, k1, _), (o0, k0, _) = both(sc, lambda: sc.decompress_range(ZSTD, ADLER, e_img, e_index, e_sums, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and np.array_equal(o0, content)
    assert (k1, k0) == (len(S.block_headers(a)[0]) + len(S.block_headers(b)[0]), 0)


# ---- 8. key 13 and key 15 together ----------------------------------------------------------------------------------------------------
def test_block_path_and_staged_path(sc):
    """A partition that holds a frame of the library's writer followed by a libzstd frame: key 14 counts the first frame's
    blocks, key 16 the second's."""
    rng = np.random.default_rng(8)
    src = np.repeat(rng.integers(97, 123, (2 * S.B + 77) // 4 + 1, dtype=np.uint8), 4)[:2 * S.B + 77]
    sc.set_option(OPT_ZSTD_COMPRESS, 1)
    w_img, w_index, _ = sc.compress_map_output(ZSTD, 0, src, np.array([0, src.size], np.int64))
    sc.set_option(OPT_ZSTD_COMPRESS, 0)
    lz, lsrc = S.libzstd_frame(6, True)
    part = np.concatenate([w_img, lz])
    index = np.array([0, part.size], np.int64)
    content = np.concatenate([src, lsrc])
    n_lz = len(S.block_headers(lz)[0])
    sc.set_option(OPT_VARIANT, 1)
    (o1, k16, k14), (o0, k16_0, k14_0) = both(sc, lambda: sc.decompress_range(ZSTD, 0, part, index, None, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and np.array_equal(o0, content)
    assert (k14, k16) == (3, n_lz) and (k14_0, k16_0) == (3, 0)
    sc.set_option(OPT_VARIANT, 0)  # without the block path the staged one takes both frames
    (o1, k16, k14), (o0, k16_0, k14_0) = both(sc, lambda: sc.decompress_range(ZSTD, 0, part, index, None, dst_capacity=content.size).copy())
    assert np.array_equal(o1, content) and np.array_equal(o0, content)
    assert (k14, k16) == (0, 3 + n_lz) and (k14_0, k16_0) == (0, 0)
