"""The Zstandard conformance corpus on the GPU (S3S_CODEC_ZSTD through s3s_decompress_range, s3s_decompressed_size and
s3s_decompress_ranges_batch_device): the frames of tests/zstd_conformance.py - written construct by construct from RFC 8878,
see tests/test_zstd_conformance.py for what they cover and for the CPU legs (host model, ASan, ISA interpreter) that run first -
are the partitions of one `.data` image with an index and Adler32 / CRC32 checksums from the oracle.  libzstd's decoder is the
arbiter of every frame before the product sees it; all comparisons are byte for byte.

Nothing here provokes a fault: an invalid frame is one the decoder refuses by its own checks (shown on the CPU first).

The product's two documented leniencies are out of scope and the corpus stays clear of them: it keeps the whole frame as
history and caps a block at 128 KiB whatever the window descriptor says, where libzstd refuses window logs above 27 and blocks
larger than the window."""
import numpy as np
import pytest

import zstd_conformance as zc

pytestmark = pytest.mark.gpu

ZSTD = 3
ADLER, CRC = 1, 2
N_GENERATED = 400  # seeds 0 .. 399, fixed


@pytest.fixture(scope="module")
def corpus():
    cases = zc.fixed_corpus() + [zc.generated_case(seed) for seed in range(N_GENERATED)]
    for c in cases:
        zc.arbiter(c)
    return cases


def _image(cases, algo):
    from oracle import binding

    parts = [np.frombuffer(c.data, np.uint8) for c in cases]
    index = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([p.size for p in parts], out=index[1:])
    sums = np.array([binding.checksum(algo, p) for p in parts], dtype=np.int64) if algo else None
    want = np.frombuffer(b"".join(c.content for c in cases), np.uint8)
    return np.concatenate(parts), index, sums, want


def _first_difference(cases, out, want):
    at = int(np.argmax(out != want)) if out.size == want.size else -1
    pos = 0
    for c in cases:
        if pos <= at < pos + len(c.content):
            return c.name, at - pos
        pos += len(c.content)
    return None, at


def _check_range(gpu_codec, cases, algo):
    img, index, sums, want = _image(cases, algo)
    assert gpu_codec.decompressed_size(ZSTD, img) == want.size
    out = gpu_codec.decompress_range(ZSTD, algo, img, index, sums, dst_capacity=want.size)
    assert out.size == want.size and np.array_equal(out, want), _first_difference(cases, out, want)


def _inside_the_guess(c):  # the single pass decodes a partition at 8 x its compressed size + 4096 (zstd_decompress.hip)
    return len(c.content) <= 8 * len(c.data) + 4096


ZEROS = None


def _zeros():
    """A partition libzstd wrote from 2 MB of zeros: ~200 bytes, far beyond any guess - the call takes the two-pass form."""
    global ZEROS
    if ZEROS is None:
        from oracle import zstd_ref as z

        data = np.zeros(2_000_000, np.uint8)
        ZEROS = zc.Case("zeros", bytes(z.compress_stream(data, 1)), data.tobytes(), 0, False)
    return ZEROS


@pytest.mark.parametrize("algo", [ADLER, CRC, 0])
def test_corpus_single_pass_two_pass_and_both_parities(gpu_codec, corpus, algo):
    """The valid partitions that stay inside the single pass's guesses as one image: as it is (single pass), with a partition
    of zeros added (two passes), and both again without the first partition (the other slot of every workgroup, another
    neighbour).  Then ALL valid partitions, RLE literals and blocks of 128 KiB from a few bytes among them (two passes)."""
    valid = [c for c in corpus if c.content is not None]
    inside = [c for c in valid if _inside_the_guess(c)]
    assert len(inside) > 300 and len(valid) - len(inside) > 20
    for cases in (inside, inside + [_zeros()], inside[1:], inside[1:] + [_zeros()], valid, valid[1:]):
        _check_range(gpu_codec, cases, algo)


def test_corpus_one_partition_per_call(gpu_codec, corpus):
    """Every valid partition alone (a workgroup with one partition; the failing frame has a name)."""
    for c in corpus:
        if c.content is None or not c.data:
            continue
        comp = np.frombuffer(c.data, np.uint8)
        assert gpu_codec.decompressed_size(ZSTD, comp) == len(c.content), c.name
        out = gpu_codec.decompress_range(ZSTD, 0, comp, np.array([0, comp.size], np.int64), None, dst_capacity=len(c.content))
        assert out.tobytes() == c.content, c.name


def test_corpus_batched_on_the_device_with_painted_destinations(gpu_codec, corpus):
    """s3s_decompress_ranges_batch_device: the corpus cut into ranges of 1 .. 40 partitions, every destination exactly as large
    as its content with a painted tail behind it; once inside the guesses (single pass), once everything (two passes)."""
    from hipdev import Dev

    valid = [c for c in corpus if c.content is not None]
    rng = np.random.default_rng(17)
    for pool in ([c for c in valid if _inside_the_guess(c)], valid):
        groups, at = [], 0
        while at < len(pool):
            n = int(rng.integers(1, 41))
            groups.append(pool[at:at + n])
            at += n
        dev = Dev()
        try:
            args, outs = [], []
            for g in groups:
                img, index, sums, want = _image(g, CRC)
                d_out = dev.upload(np.full(want.size + 64, 0xA5, np.uint8))
                outs.append((d_out, want, g))
                args.append((dev.upload(img if img.size else np.zeros(1, np.uint8)), img.size, index, sums, d_out, want.size))
            res = gpu_codec.decompress_ranges_batch_device(ZSTD, CRC, args, raise_on_error=False)
            for (st, n, bad), (d_out, want, g) in zip(res, outs):
                assert st == 0 and n == want.size, (st, n, bad, g[max(bad, 0)].name)
                back = dev.download(d_out, want.size + 64)
                assert np.array_equal(back[:n], want), _first_difference(g, back[:n], want)
                assert np.all(back[n:] == 0xA5), "wrote behind the destination"
        finally:
            dev.free()


def test_invalid_frames_are_refused_beside_valid_ranges(gpu_codec, corpus):
    """Every invalid frame of the fixed list in a batched call of its own kind: alone in a range, and between valid partitions
    of a range, next to valid ranges.  The invalid ranges report "bad frame" (-3; -6 for a non-zero dictionary id) and write
    nothing behind their destinations, the valid ranges of the same call are intact, and a clean call succeeds afterwards."""
    from hipdev import Dev

    valid = [c for c in corpus if c.content is not None and _inside_the_guess(c)][:60]
    invalid = [c for c in corpus if c.content is None]
    assert len(invalid) >= 20
    g_img, g_index, _, g_want = _image(valid, 0)
    cap_bad = 1 << 17
    for at in range(0, len(invalid), 8):
        chunk = invalid[at:at + 8]
        dev = Dev()
        try:
            args, checks = [], []

            def add(img, index, cap, paint, want, rc, name):
                d_out = dev.upload(np.full(cap + paint, 0xA5, np.uint8))
                args.append((dev.upload(img), img.size, index, None, d_out, cap))
                checks.append((d_out, cap, paint, want, rc, name))

            add(g_img, g_index, g_want.size, 64, g_want, 0, "valid")
            for c in chunk:
                bad = np.frombuffer(c.data, np.uint8)
                add(bad, np.array([0, bad.size], np.int64), cap_bad, 4096, None, c.rc, c.name)
                # [30 valid partitions | the invalid one | 30 valid partitions]
                cut = int(g_index[30])
                mixed = np.concatenate([g_img[:cut], bad, g_img[cut:]])
                add(mixed, np.concatenate([g_index[:31], g_index[30:] + bad.size]), g_want.size + cap_bad, 4096, None, c.rc, c.name + " (mixed)")
                add(g_img, g_index, g_want.size, 64, g_want, 0, "valid")
            res = gpu_codec.decompress_ranges_batch_device(ZSTD, 0, args, raise_on_error=False)
            for (st, n, bad), (d_out, cap, paint, want, rc, name) in zip(res, checks):
                back = dev.download(d_out, cap + paint)
                assert np.all(back[cap:] == 0xA5), name
                if want is None:
                    assert st == rc, (name, st)
                else:
                    assert st == 0 and n == want.size and np.array_equal(back[:n], want), (name, st)
        finally:
            dev.free()
        # and through the single-range entry point: refused with the same status
        import s3shuffle

        for c in chunk:
            bad = np.frombuffer(c.data, np.uint8)
            with pytest.raises(s3shuffle.CodecError) as ei:
                gpu_codec.decompress_range(ZSTD, 0, bad, np.array([0, bad.size], np.int64), None, dst_capacity=cap_bad)
            assert ei.value.code == c.rc, c.name
        assert np.array_equal(gpu_codec.decompress_range(ZSTD, 0, g_img, g_index, None, dst_capacity=g_want.size), g_want)
