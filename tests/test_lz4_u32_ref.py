"""tests/lz4_u32_ref.py (the Python restatement of liblz4's byU32 parse) pinned to the liblz4 of the machine, and the inputs of
the big-block tests checked for what they are meant to exercise.  CPU only."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "spark-s3-shuffle_amd"))
import corpus  # noqa: E402
import lz4_u32_ref as R  # noqa: E402

LENGTHS = (65_547, 65_548, 70_000, 131_072, 200_000)


def inputs(lengths=LENGTHS, seed=5):
    """(name, bytes) of TeraSort, wide rows, chunk_corpus, zeros and random at every length, then the far-motif input"""
    from s3shuffle import datagen

    rng = np.random.default_rng(seed)
    tera = datagen.terasort_map_output(1 << 20, 1, seed=3)[0]
    wide = datagen.tpcds_wide_map_output(1 << 20, 1, seed=4)[0]
    out = []
    for n in lengths:
        out += [("terasort", tera[:n]), ("wide", wide[:n]), ("corpus", corpus.chunk_corpus(7, n, rng)), ("zeros", np.zeros(n, np.uint8)),
                ("random", rng.integers(0, 256, n, dtype=np.uint8))]
    out.append(("far_motif", R.far_motif(rng)))
    return [(name, np.ascontiguousarray(d, dtype=np.uint8)) for name, d in out]


def test_model_equals_liblz4_from_65547_bytes_on():
    cases = inputs()
    assert len(cases) == 26
    refused = {}
    for name, d in cases:
        payload, far = R.compress_u32(d.tobytes())
        assert payload == R.liblz4_block(d), (name, d.size)
        refused[(name, d.size)] = far
    # what the inputs exercise: candidates refused by the distance test (figures counted once, pinned here)
    assert refused[("terasort", 131_072)] == 840 and refused[("wide", 131_072)] == 256 and refused[("corpus", 131_072)] == 759
    assert refused[("far_motif", 146_500)] == 840
    assert refused[("zeros", 131_072)] == 0


def test_the_switch_point_is_65547():
    """below LZ4_64Klimit liblz4 is the byU16 parse: the byU32 restatement differs at 65 546 bytes and agrees at 65 547"""
    from s3shuffle import datagen

    tera = datagen.terasort_map_output(1 << 20, 1, seed=3)[0]
    for n, same in ((65_546, False), (65_547, True)):
        d = np.ascontiguousarray(tera[:n])
        assert (R.compress_u32(d.tobytes())[0] == R.liblz4_block(d)) == same, n


def test_far_motif_refuses_candidates_whose_bytes_match():
    d = R.far_motif(np.random.default_rng(5)).tobytes()
    trace = []
    payload, far = R.compress_u32(d, trace)
    assert payload == R.liblz4_block(np.frombuffer(d, np.uint8)) and far > 0
    # the second copy of the motif starts 73 000 bytes after the first: equal bytes, yet no sequence may reach that far back
    assert d[73_000:76_000] == d[0:3_000] and d[143_000:146_000] == d[0:3_000]
    assert all(ip - m <= 65_535 for ip, m, _, _ in trace)
    assert max(R.block_offsets(payload)) <= 65_535


def test_boundary_inputs_sit_exactly_at_the_distance_limit():
    b0, b1 = R.boundary_pair()
    for d, want_max in ((b0, 65_535), (b1, None)):
        ref = R.liblz4_block(d)
        payload, far = R.compress_u32(d.tobytes())
        assert payload == ref
        offs = R.block_offsets(ref)
        if want_max:
            assert max(offs) == 65_535 and far == 0  # the second copy is matched at the largest offset the format has
        else:
            assert max(offs) < 65_535 and far >= 1   # one byte further: refused, found again only through nearer candidates
        assert R.framing.lz4_decode_py(ref, max_out=d.size + 1) == d.tobytes()


def test_level_is_the_ceiling():
    assert [R.level(b) for b in (64, 1024, 1025, 32_768, 65_536, 65_537, 100_000, 131_072, 1 << 20, 1 << 25)] == [0, 0, 1, 5, 6, 7, 7, 7, 10, 15]
