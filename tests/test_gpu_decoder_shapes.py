"""GPU: the spec-level corpus of tests/decoder_shapes.py (every token form, offset class and window phase of LZ4, Snappy and
LZF, checked on the CPU by tests/test_decoder_shapes_cpu.py) through every reduce-side path.  The cases of one codec are the
partitions of one fetched range - one case, one partition, checksums computed with zlib on the host - so one call decodes the
whole corpus.  Every leg compares every partition byte for byte with the bytes the writer kept while it wrote the block; the
destination sits between two 4096-byte bands painted 0xA5 that must come back untouched.  A mismatch names the case and its
first differing byte.  What the interpreter cannot see and this can: a missing drain in front of a read-back of flushed bytes,
an LDS ordering slip, an unaligned store that behaves differently on the hardware."""
import zlib

import numpy as np
import pytest

import decoder_shapes as ds
import io_encryption_inputs as I
import spark_crypto_ref as R
from hipdev import Dev
from test_gpu_decode_stream import run_stream

pytestmark = pytest.mark.gpu

LZ4, SNAPPY, LZF = ds.LZ4, ds.SNAPPY, ds.LZF
ADLER = 1
OPT_DECODE_VARIANT = 5
GUARD = 4096
CODECS = pytest.mark.parametrize("codec", [LZ4, SNAPPY, LZF], ids=["lz4", "snappy", "lzf"])
# LZ4 and Snappy under the ring decoder (3) and the batch decoder (4); LZF has the batch decoder only
PATHS = pytest.mark.parametrize("codec,variant", [(LZ4, 3), (LZ4, 4), (SNAPPY, 3), (SNAPPY, 4), (LZF, 4)],
                                ids=["lz4-ring", "lz4-batch", "snappy-ring", "snappy-batch", "lzf-batch"])

_PACKED = {}


RING_MAX_CHUNK = 32768  # the Snappy ring decoder (variant 3) keeps its 32 KiB limit, S3S_E_UNSUPPORTED above it


def _ring_takes(codec, variant, case):
    return not (codec == SNAPPY and variant == 3 and max(len(u[2]) for u in case.units) > RING_MAX_CHUNK)


def _packed(codec, far_only=False, variant=4):
    """(cases, image, index, decoded offsets, Adler32 of every partition's stored bytes), built once and never changed.
    Every case of the codec - but for the Snappy ring decoder, whose documented limit is a chunk of 32 KiB: its range holds
    the cases within the limit, and test_snappy_ring_decoder_refuses_the_larger_chunks holds the others against the refusal."""
    key = (codec, far_only, codec == SNAPPY and variant == 3)
    if key not in _PACKED:
        cases = [c for c in ds.cases(codec) if (ds.is_far(c) or not far_only) and _ring_takes(codec, variant, c)]
        img, index, offs = ds.pack_range(cases)
        sums = np.array([zlib.adler32(img[index[p]:index[p + 1]].tobytes()) for p in range(len(cases))], np.int64)
        for a in (img, index, offs, sums):
            a.setflags(write=False)
        _PACKED[key] = (cases, img, index, offs, sums)
    return _PACKED[key]


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.free()


@pytest.fixture()
def variant_option(gpu_codec):
    """sets S3S_OPT_LZ4_DECODE_VARIANT for the test and puts the default back"""
    default = gpu_codec.get_option(OPT_DECODE_VARIANT)
    yield lambda v: gpu_codec.set_option(OPT_DECODE_VARIANT, v)
    gpu_codec.set_option(OPT_DECODE_VARIANT, default)


def _guarded(dev, size, mis):
    """a destination of `size` bytes at `mis` mod 16 between two painted bands -> (allocation, destination, bytes allocated)"""
    total = size + 2 * GUARD + 16
    d_buf = dev.upload(np.full(total, 0xA5, np.uint8))
    assert d_buf % 16 == 0
    return d_buf, d_buf + GUARD + mis, total


def _bands_intact(dev, d_buf, total, size, mis, what):
    host = dev.download(d_buf, total)
    o = GUARD + mis
    assert (host[:o] == 0xA5).all(), "%s: bytes in front of the destination changed" % what
    assert (host[o + size:] == 0xA5).all(), "%s: bytes behind the destination changed" % what
    return host[o:o + size]


def _one_shot(gpu_codec, dev, codec, cases, img, index, offs, sums, mis, what, d_img=None):
    """decodes the range into a guarded destination of exactly its decoded size; every case compared -> the decoded bytes"""
    size = int(offs[-1])
    d_img = dev.upload(img) if d_img is None else d_img
    d_buf, d_dst, total = _guarded(dev, size, mis)
    n = gpu_codec.decompress_range_device(codec, ADLER if sums is not None else 0, d_img, img.size, index, sums, d_dst, size)
    got = _bands_intact(dev, d_buf, total, size, mis, what)
    dev.release(d_buf)
    assert n == size, (what, n, size)
    bad = ds.first_difference(cases, offs, got, what)
    assert bad is None, bad
    return got


@pytest.mark.parametrize("checksum", [True, False], ids=["adler32", "nosum"])
@PATHS
def test_one_shot(gpu_codec, dev, variant_option, codec, variant, checksum):
    cases, img, index, offs, sums = _packed(codec, variant=variant)
    assert len(cases) == len(ds.cases(codec)) or (codec, variant) == (SNAPPY, 3)
    variant_option(variant)
    d_img = dev.upload(img)
    for mis in (0, 1, 7, 15):  # the `sh` of the window arithmetic
        _one_shot(gpu_codec, dev, codec, cases, img, index, offs, sums if checksum else None, mis,
                  "one-shot, variant %d, destination + %d" % (variant, mis), d_img)


@PATHS
def test_far_and_window_base_cases_at_every_alignment(gpu_codec, dev, variant_option, codec, variant):
    cases, img, index, offs, sums = _packed(codec, far_only=True, variant=variant)
    assert len(cases) >= 6
    variant_option(variant)
    d_img = dev.upload(img)
    for mis in range(16):
        _one_shot(gpu_codec, dev, codec, cases, img, index, offs, sums, mis, "far cases, variant %d, destination + %d" % (variant, mis), d_img)


def test_snappy_ring_decoder_refuses_the_larger_chunks(gpu_codec, dev, variant_option):
    """the cases test_one_shot leaves out of the ring decoder's range: each is refused as S3S_E_UNSUPPORTED (the documented
    answer above 32 KiB, not a wrong one) with nothing written outside the destination, and there are only such cases"""
    import s3shuffle

    left_out = [c for c in ds.cases(SNAPPY) if not _ring_takes(SNAPPY, 3, c)]
    assert 0 < len(left_out) < len(ds.cases(SNAPPY)) // 4
    variant_option(3)
    for c in left_out:
        assert max(len(u[2]) for u in c.units) > RING_MAX_CHUNK
        img, index, offs = ds.pack_range([c])
        size = int(offs[-1])
        d_buf, d_dst, total = _guarded(dev, size, 1)
        with pytest.raises(s3shuffle.CodecError) as e:
            gpu_codec.decompress_range_device(SNAPPY, 0, dev.upload(img), img.size, index, None, d_dst, size)
        assert e.value.code == -6, (c.name, e.value.code)
        _bands_intact(dev, d_buf, total, size, 1, c.name)
        dev.release(d_buf)


@CODECS
def test_batched_ranges_equal_the_one_shot_call(gpu_codec, dev, codec):
    cases, img, index, offs, sums = _packed(codec)
    n = len(cases)
    cuts = [0, n // 6, n // 6 + n // 2, n]  # three ranges of unequal size
    one = _one_shot(gpu_codec, dev, codec, cases, img, index, offs, sums, 0, "one-shot")
    d_img = dev.upload(img)
    args, bufs = [], []
    for k, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        size = int(offs[r1] - offs[r0])
        d_buf, d_dst, total = _guarded(dev, size, (3, 0, 9)[k])
        bufs.append((d_buf, total, size, (3, 0, 9)[k]))
        args.append((d_img + int(index[r0]), int(index[r1] - index[r0]), index[r0:r1 + 1] - index[r0], sums[r0:r1], d_dst, size))
    res = gpu_codec.decompress_ranges_batch_device(codec, ADLER, args)
    for k, ((st, nbytes, bad), (d_buf, total, size, mis), (r0, r1)) in enumerate(zip(res, bufs, zip(cuts[:-1], cuts[1:]))):
        got = _bands_intact(dev, d_buf, total, size, mis, "batched range %d" % k)
        assert (st, nbytes, bad) == (0, size, -1), (k, st, nbytes, bad)
        msg = ds.first_difference(cases[r0:r1], offs[r0:r1 + 1] - offs[r0], got, "batched range %d" % k)
        assert msg is None, msg
        assert np.array_equal(got, one[int(offs[r0]):int(offs[r1])])


@CODECS
def test_streaming_equals_the_one_shot_call(gpu_codec, dev, codec):
    cases, img, index, offs, sums = _packed(codec)
    one = _one_shot(gpu_codec, dev, codec, cases, img, index, offs, sums, 0, "one-shot")
    total = int(index[-1])
    window = total // 12  # (a unit longer than the window makes the stream ask for a longer one, once)
    cap = max(len(u[2]) for c in cases for u in c.units) + 1000
    d_buf, d_dst, allocated = _guarded(dev, cap, 0)
    # the per-partition verdicts: a stream that reaches the end without raising has found every partition's checksum right
    out, feeds, growths, results = run_stream(gpu_codec, dev, codec, ADLER, img, index, sums, window, cap, None, d_dst, 4 * len(cases) + 100)
    _bands_intact(dev, d_buf, allocated, cap, 0, "stream")
    assert feeds - growths >= 8, (feeds, growths)
    assert sum(r[2] for r in results) == total and results[-1][5] == 1
    msg = ds.first_difference(cases, offs, out, "stream")
    assert msg is None, msg
    assert np.array_equal(out, one)


@CODECS
def test_one_shot_under_io_encryption(gpu_codec, dev, codec):
    """the decrypting pass writes the bytes the decoder then reads: one more producer in front of the same kernel"""
    cases, img, index, offs, sums = _packed(codec)
    key = I.KEYS[16]
    e_img, e_index, e_sums = R.encrypt_map_output(img, index, key, I.ivs_for(offs), ADLER)
    gpu_codec.set_io_encryption(key)
    try:
        _one_shot(gpu_codec, dev, codec, cases, e_img, e_index, offs, e_sums, 5, "one-shot under IO encryption")
    finally:
        gpu_codec.set_io_encryption(None)
