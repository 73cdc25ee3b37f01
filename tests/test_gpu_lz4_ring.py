"""GPU: the LZ4 input-ring kernel (S3S_OPT_LZ4_VARIANT 11, lz4_compress_ring_kernel) on the inputs of tests/lz4_ring_cases.py,
which put matches on the ring's edges (span, wrap point, coverage ahead, hand-back and re-entry, short history, lengths around
the block's limits, the end of the allocation, the bench generators' blocks).  Every chunk is one partition of a map output;
index, checksums and image must equal oracle.compress_map_output byte for byte, and the call must have run variant 11."""
import numpy as np
import pytest

import lz4_ring_cases as cases

pytestmark = pytest.mark.gpu

LZ4, CRC = 1, 2
OPT_LZ4_BLOCK_SIZE, OPT_LZ4_VARIANT, OPT_LZ4_VARIANT_USED = 1, 4, 7


@pytest.fixture
def ring_codec(gpu_codec):
    old = gpu_codec.get_option(OPT_LZ4_VARIANT)
    gpu_codec.set_option(OPT_LZ4_VARIANT, 11)
    yield gpu_codec
    gpu_codec.set_option(OPT_LZ4_VARIANT, old)


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_ring_kernel_matches_the_oracle(ring_codec, oracle, case):
    chunks = cases.CASES[case]()
    block = 65536 if max(len(c) for c in chunks) > 32768 else 32768
    data = np.concatenate(chunks)  # the last chunk ends the source buffer
    offs = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
    old = ring_codec.get_option(OPT_LZ4_BLOCK_SIZE)
    ring_codec.set_option(OPT_LZ4_BLOCK_SIZE, block)
    try:
        img, index, sums = ring_codec.compress_map_output(LZ4, CRC, data, offs)
        assert ring_codec.get_option(OPT_LZ4_VARIANT_USED) == 11
    finally:
        ring_codec.set_option(OPT_LZ4_BLOCK_SIZE, old)
    r_img, r_index, r_sums = oracle.compress_map_output(LZ4, CRC, data, offs, block)
    assert np.array_equal(index, r_index), (index[:8], r_index[:8])
    assert np.array_equal(sums, r_sums)
    assert img.size == r_img.size
    if not np.array_equal(img, r_img):
        first = int(np.nonzero(img != r_img)[0][0])
        part = int(np.searchsorted(index, first, side="right") - 1)
        raise AssertionError(f"image differs at byte {first} (partition {part}, +{first - index[part]})")


def test_default_runs_the_ring_kernel_and_variant_10_stays(gpu_codec, oracle):
    """a fresh context runs variant 11; variant 10 (lz4_compress_l2_kernel<true>) stays selectable, same bytes"""
    import s3shuffle

    chunks = cases.generated()[:2]
    data = np.concatenate(chunks)
    offs = np.array([0, data.size], dtype=np.int64)
    want = oracle.compress_map_output(LZ4, CRC, data, offs)
    with s3shuffle.Codec(0) as c:
        assert c.get_option(OPT_LZ4_VARIANT) == 11
        for variant in (11, 10, 11):
            c.set_option(OPT_LZ4_VARIANT, variant)
            img, index, sums = c.compress_map_output(LZ4, CRC, data, offs)
            assert c.get_option(OPT_LZ4_VARIANT_USED) == variant
            assert np.array_equal(img, want[0]) and np.array_equal(index, want[1]) and np.array_equal(sums, want[2])


def test_auto_takes_the_ring_kernel_on_a_batched_call(oracle):
    """S3S_OPT_LZ4_VARIANT 9 (auto) times 1 against 10 on the one-task entry points (tests/test_gpu_compress.py pins that); a
    batched call, which has no timing rounds, runs the windowed parse at once: the ring kernel, same bytes"""
    import s3shuffle

    chunks = cases.generated()
    tasks_in = [np.concatenate(chunks[:4]), np.concatenate(chunks[4:])]
    with s3shuffle.Codec(0) as c:
        c.set_option(OPT_LZ4_VARIANT, 9)
        offs = [np.array([0, d.size // 2, d.size], dtype=np.int64) for d in tasks_in]
        caps = [int(c.max_compressed_size(LZ4, o)) for o in offs]
        dsts = [np.zeros(cap, dtype=np.uint8) for cap in caps]
        res = c.compress_map_outputs_batch(LZ4, CRC, [(d.ctypes.data, o, dst.ctypes.data, cap)
                                                      for d, o, dst, cap in zip(tasks_in, offs, dsts, caps)])
        assert c.get_option(OPT_LZ4_VARIANT_USED) == 11
        for d, o, dst, (total, index, sums) in zip(tasks_in, offs, dsts, res):
            r_img, r_index, r_sums = oracle.compress_map_output(LZ4, CRC, d, o)
            assert total == r_img.size and np.array_equal(index, r_index) and np.array_equal(sums, r_sums)
            assert np.array_equal(dst[:total], r_img)
