"""GPU: the window block's chain on the hardware (lz4_window_engine.inc: the next window's duplicate-hash passes run during the
current window; the run loop's layout).  A fresh context with its default options (the input-ring kernel) compresses three
partitions of two 32 KiB blocks plus an odd tail from each bench generator, and the period-64 chunks of
tests/lz4_chain_cases.py (consecutive windows hash into the same slots), through the one-task and the batched entry points;
index, checksums and image must equal oracle.compress_map_output byte for byte."""
import numpy as np
import pytest

import lz4_chain_cases as cases

pytestmark = pytest.mark.gpu

LZ4, CRC = 1, 2
OPT_LZ4_VARIANT_USED = 7
PART = 2 * 32768 + 1237
_INPUTS, _WANT = {}, {}


def _input(name):
    """(data, offsets) of a map output; built once"""
    if name not in _INPUTS:
        if name == "period64":
            chunks = cases.period64()
            data = np.concatenate(chunks)
            offs = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
        else:
            from s3shuffle import datagen

            gen, seed = {"terasort": (datagen.terasort_map_output, 2), "tpcds-wide": (datagen.tpcds_wide_map_output, 3)}[name]
            raw, _ = gen(1 << 20, 8, seed=seed, map_id=0)
            data = np.asarray(raw, dtype=np.uint8)[4096:4096 + 3 * PART].copy()
            offs = np.arange(4, dtype=np.int64) * PART
        _INPUTS[name] = (data, offs)
    return _INPUTS[name]


def _want(oracle, name):
    if name not in _WANT:
        _WANT[name] = oracle.compress_map_output(LZ4, CRC, *_input(name))
    return _WANT[name]


@pytest.fixture(scope="module")
def default_codec():
    import s3shuffle

    with s3shuffle.Codec(0) as c:
        yield c


def _same(got, want):
    img, index, sums = got
    r_img, r_index, r_sums = want
    assert np.array_equal(index, r_index), (index[:8], r_index[:8])
    assert np.array_equal(sums, r_sums)
    assert img.size == r_img.size
    if not np.array_equal(img, r_img):
        first = int(np.nonzero(img != r_img)[0][0])
        part = int(np.searchsorted(index, first, side="right") - 1)
        raise AssertionError(f"image differs at byte {first} (partition {part}, +{first - index[part]})")


@pytest.mark.parametrize("name", ["terasort", "tpcds-wide", "period64"])
def test_one_task(default_codec, oracle, name):
    data, offs = _input(name)
    got = default_codec.compress_map_output(LZ4, CRC, data, offs)
    assert default_codec.get_option(OPT_LZ4_VARIANT_USED) == 11
    _same(got, _want(oracle, name))


def test_batched(default_codec, oracle):
    names = ["terasort", "tpcds-wide", "period64"]
    c = default_codec
    ins = [_input(n) for n in names]
    caps = [int(c.max_compressed_size(LZ4, o)) for _, o in ins]
    dsts = [np.zeros(cap, dtype=np.uint8) for cap in caps]
    res = c.compress_map_outputs_batch(LZ4, CRC, [(d.ctypes.data, o, dst.ctypes.data, cap)
                                                  for (d, o), dst, cap in zip(ins, dsts, caps)])
    assert c.get_option(OPT_LZ4_VARIANT_USED) == 11
    for n, dst, (total, index, sums) in zip(names, dsts, res):
        assert total == _want(oracle, n)[0].size
        _same((dst[:total], index, sums), _want(oracle, n))
