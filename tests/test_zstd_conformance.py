"""Conformance of the Zstandard decoder (csrc/zstd_decode_core.h, zstd_decompress.hip) with the FORMAT, not with what one
compressor emits: the frames of tests/zstd_conformance.py are written construct by construct from RFC 8878
(tests/zstd_writer.py) - RLE and treeless literals in every size format, Huffman codes of depth 11 and of 256 symbols, every
table mode of every field incl. Repeat after each of the others, custom distributions at both accuracy-log limits, every form
of the sequence count, sequences wider than the decoder's 57-bit window next to minimal ones, repeat-offset corner cases,
every frame-header field - plus frames drawn by a seeded generator from all of those controls.

libzstd's DECODER is the arbiter: every test first asserts that libzstd 1.4.8 decodes the frame to exactly the writer's own
content (or refuses an invalid one), and only then consults the product: here the host build of the decoder core (size pass =
decode pass, guard bytes, and once more under ASan / UBSan from exact-size heap buffers) and the compiled kernel under the ISA
interpreter, two partitions to a workgroup; tests/test_gpu_zstd_conformance.py does the same on the GPU.  All comparisons are
byte for byte.

Two documented leniencies of the product are out of scope, and the writer's valid frames stay clear of them: the product keeps
the whole frame as history and caps a block at 128 KiB whatever the window descriptor says, where libzstd refuses window logs
above 27 and blocks (or offsets) larger than the window.  (Found while building the corpus, and likewise left out: libzstd 1.4.8
decodes repeat code 3 with literal length 0 and rep0 == 1 - offset 0 - as offset 1 where the product refuses the frame, and
refuses a compressed block whose Block_Size field is exactly 131 072 where the product accepts it; zstd_writer.Frame(strict=False)
builds one.)"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import zstd_conformance as zc
import zstd_model_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_GENERATED = 600        # seeds 0 .. 599, fixed
N_GENERATED_EMU = 20     # the first ones of at most 10 000 bytes of content: what the interpreter takes in a minute


@pytest.fixture(scope="module")
def fixed():
    return zc.fixed_corpus()


@pytest.fixture(scope="module")
def generated():
    return [zc.generated_case(seed) for seed in range(N_GENERATED)]


@pytest.fixture(scope="module")
def model():
    return zstd_model_lib.load()


arbiter = zc.arbiter  # libzstd's decoder, asked before the product sees a frame


def test_corpus_contains_every_shape_of_the_matrix(fixed):
    """tests/tools/zstd_shapes.py parses the valid frames of the fixed list; not one shape of its MATRIX may be missing (so the
    list cannot lose one silently), and the invalid frames the issue names are there by name."""
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import zstd_shapes

    tally = zstd_shapes.Counter()
    for c in fixed:
        if c.content is not None:
            zstd_shapes.shapes(c.data, tally)
    assert zstd_shapes.missing(tally) == []
    assert tally["max_seq_bits"] > 57
    names = {c.name for c in fixed if c.content is None}
    for want in ("treeless_1s_first_block_invalid", "treeless_4s_first_block_of_second_frame_invalid", "repeat_ll_first_block_invalid",
                 "repeat_of_first_block_invalid", "repeat_ml_first_block_invalid", "offset_one_beyond_the_history_invalid", "fcs_too_large_invalid",
                 "dictionary_id_nonzero_in_1_bytes_unsupported", "reserved_bit_invalid", "checksum_wrong_invalid"):
        assert want in names


def test_libzstd_agrees_with_the_writer_on_every_frame(fixed, generated):
    for c in fixed + generated:
        arbiter(c)
    assert all(c.content is not None for c in generated)


def _model_leg(model, c):
    arbiter(c)
    comp = np.frombuffer(c.data, np.uint8)
    if c.content is None:
        rc, out = zstd_model_lib.decode(model, comp, 1 << 20)
        assert rc == c.rc and out is None, (c.name, rc)
    else:
        rc, out = zstd_model_lib.decode(model, comp, len(c.content))
        assert rc == 0 and out.tobytes() == c.content, (c.name, rc)
        if c.content:  # one byte short: a capacity verdict, nothing behind the destination (checked in decode)
            rc, _ = zstd_model_lib.decode(model, comp, len(c.content) - 1)
            assert rc == -2, (c.name, rc)


def test_host_model_fixed_corpus(model, fixed):
    for c in fixed:
        _model_leg(model, c)


def test_host_model_generated_frames(model, generated):
    for c in generated:
        _model_leg(model, c)


def test_host_model_under_asan_from_exact_size_buffers(fixed, generated):
    """The same decodes under ASan / UBSan (tests/model/zstd_asan_corpus.cpp): source and destination are heap blocks of exactly
    their sizes, so a READ outside the source - invisible to guard bytes, a memory fault on the GPU - ends the run."""
    exe = os.path.join(HERE, "model", "zstd_asan_corpus")
    src = os.path.join(HERE, "model", "zstd_asan_corpus.cpp")
    core = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc", "zstd_decode_core.h")
    if not os.path.exists(exe) or max(os.path.getmtime(src), os.path.getmtime(core)) > os.path.getmtime(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        src, "-o", exe], check=True)
    cases = fixed + generated
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        with open(path, "wb") as f:
            for c in cases:
                content = c.content or b""
                f.write(struct.pack("<IIi", len(c.data), len(content), c.rc) + c.data + content)
        r = subprocess.run([exe, path], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "%d cases, 0 wrong" % len(cases) in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- the compiled kernel under the ISA interpreter ---------------------------------------------------------------------------
def _emu_leg(cases):
    """Partitions k, k + 1 share a workgroup (two sequence wavefronts, one literal wavefront); every buffer has exactly its
    size, so an access outside faults in the interpreter."""
    sys.path.insert(0, os.path.join(HERE, "isa"))
    import zstd_kernel as zk

    for c in cases:
        arbiter(c)
    parts = [(c.data, len(c.content) if c.content is not None else 4096) for c in cases]
    out, rcs, _ = zk.decode_partitions(parts)
    for c, o, rc in zip(cases, out, rcs):
        if c.content is None:
            assert rc == c.rc and o is None, (c.name, rc)
        else:
            assert rc == 0 and o == c.content, (c.name, rc)


def test_compiled_kernel_fixed_corpus(fixed):
    """Every frame of the fixed list that is small enough (Case.emu), in the list's order: valid and invalid partitions end up
    in one workgroup again and again."""
    small = [c for c in fixed if c.emu]
    assert len(small) >= 150
    for at in range(0, len(small), 16):  # (eight workgroups per launch: one launch's buffers stay small)
        _emu_leg(small[at:at + 16])
    # the other parity: every partition gets the other slot of a workgroup and another neighbour
    odd = [c for c in small if len(c.data) < 600 and (c.content is None or len(c.content) < 2000)]
    for at in range(0, len(odd), 15):
        _emu_leg([zc.Case("empty", b"", b"", 0, True)] + odd[at:at + 15])


def test_compiled_kernel_generated_frames(generated):
    small = [c for c in generated if c.emu and len(c.content) <= 10_000][:N_GENERATED_EMU]
    assert len(small) == N_GENERATED_EMU
    _emu_leg(small)


def test_compiled_kernel_crafted_frames_beside_libzstd_written_and_invalid_ones(fixed):
    """A crafted partition shares its workgroup with a partition libzstd wrote, and with invalid ones: one the LITERAL wavefront
    refuses (treeless literals without a table: `err` reaches its sequence side), one the sequence side refuses (an offset beyond
    the history: `quit` releases the literal side) - on either slot; the neighbour decodes untouched."""
    from oracle import zstd_ref as z
    from s3shuffle import datagen

    by = {c.name: c for c in fixed}
    tera = datagen.terasort_map_output(1 << 20, 2, seed=3)[0][:6000]
    written = zc.Case("libzstd_level_1", bytes(z.compress_stream(tera, level=1)), tera.tobytes(), 0, True)
    crafted = [by[n] for n in ("treeless_4s_across_raw_and_rle_blocks", "repeat_after_rle", "wide_sequences_small_fse", "huf_depth11_fse_4streams")]
    bad_lit, bad_seq = by["treeless_4s_first_block_of_second_frame_invalid"], by["offset_one_beyond_the_history_second_frame_invalid"]
    _emu_leg([crafted[0], written, written, crafted[1], crafted[2], bad_lit, bad_lit, crafted[3], crafted[0], bad_seq, bad_seq, crafted[2],
              bad_lit, bad_seq, bad_seq, written, written, bad_lit])
