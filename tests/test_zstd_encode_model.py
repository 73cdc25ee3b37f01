"""The Zstandard WRITER core (spark-s3-shuffle_amd/csrc/zstd_encode_core.h) on the CPU: every frame it writes must decode
under libzstd (oracle.zstd_ref.decompress) AND under the host model of the product's own decoder to exactly its source.

The stages behind the parse are fed crafted sequence lists (counts at every boundary of the count encoding, the extreme
lengths and offsets, literal sections at every size-format boundary, alphabets around the 128-weight limit of the direct
weight header, counts whose plain Huffman tree is deeper than 11, literals Huffman cannot shrink) next to parsed data; the
same cases run once more through an AddressSanitizer build whose buffers are heap allocations of exactly the permitted size.

Two crafted cases of the list cannot exist in a block without history and are covered by their nearest legal neighbour:
a literals section of 0 bytes (the first sequence of a block needs a literal to point at: the smallest section is 1 byte) and
an offset of block length - 1 (a match of 3 bytes at offset o ends at o + 3 at the earliest: the largest offset is length - 3)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))

import zstd_encode_model_lib as E  # noqa: E402
import zstd_model_lib as D  # noqa: E402
from oracle import zstd_ref  # noqa: E402

B = E.BLOCK
RAW, RLE, COMPRESSED = 0, 1, 2          # block types
LIT_RAW, LIT_RLE, LIT_HUF = 0, 1, 2     # literals types


@pytest.fixture(scope="module")
def enc():
    return E.load()


@pytest.fixture(scope="module")
def dec():
    return D.load()


def both_decode(dec, frame, content):
    content = np.ascontiguousarray(content, dtype=np.uint8)
    back = zstd_ref.decompress(frame, content.size)
    assert back is not None, "libzstd refuses the frame"
    assert np.array_equal(back, content), "libzstd decodes other bytes"
    rc, mine = D.decode(dec, frame, content.size)
    assert rc == 0, "the product's decoder refuses the frame (%d)" % rc
    assert np.array_equal(mine, content), "the product's decoder decodes other bytes"


def skewed(rng, nsym, n, power=1.5):
    """n bytes over the values 0 .. nsym-1, every value present, frequencies falling like 1 / rank^power."""
    p = 1.0 / np.arange(1, nsym + 1) ** power
    data = rng.choice(nsym, size=n, p=p / p.sum()).astype(np.uint8)
    data[:nsym] = np.arange(nsym, dtype=np.uint8)
    rng.shuffle(data)
    return data


def text(rng, n):
    words = [bytes(rng.integers(97, 123, rng.integers(2, 9), dtype=np.uint8)) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 300) * rng.random())] + b" "
    return np.frombuffer(bytes(out[:n]), dtype=np.uint8)


def count_case(nseq):
    """nseq sequences of 3 or 4 bytes at offsets 1 .. 4, a literal in front of every 16th."""
    seqs = [(4, 3, 1)]
    for i in range(1, nseq):
        seqs.append((1 if i % 16 == 0 else 0, 3 + (i % 7 == 0), 1 + i % 4))
    nl = sum(s[0] for s in seqs) + 2
    lits = bytes((7 * i + i // 5) & 0xFF for i in range(nl))
    return lits, seqs


def crafted_cases():
    rng = np.random.default_rng(11)
    cases = {}
    for n in (0, 1, 127, 128, 0x7EFF, 0x7F00):
        cases["nseq_%d" % n] = count_case(n) if n else (bytes(skewed(rng, 40, 3000)), [])
    cases["ll0_ml3"] = (b"abcdef", [(6, 3, 2), (0, 3, 1), (0, 3, 9)])
    cases["ml_max_off1"] = (b"z", [(1, B - 1, 1)])
    big = bytes(skewed(rng, 200, B - 3))
    cases["off_max"] = (big, [(B - 3, 3, B - 3)])
    cases["ll_max"] = (big[:B - 4] + b"q", [(B - 4, 3, 5)])
    for nl in (1, 31, 32, 255, 256, 1023, 1024, 16383, 16384):
        cases["lits_%d" % nl] = (bytes(skewed(rng, 30, nl)) if nl >= 30 else bytes(rng.integers(0, 4, nl, dtype=np.uint8)), [])
        cases["lits_%d_seq" % nl] = (bytes(skewed(rng, 30, nl)) if nl >= 30 else bytes(rng.integers(0, 4, nl, dtype=np.uint8)),
                                      [(nl, 40, 1)])
    cases["lits_full_block"] = (bytes(skewed(rng, 60, B)), [])
    for nsym in (1, 2, 128, 129, 130, 256):
        cases["alphabet_%d" % nsym] = (bytes(skewed(rng, nsym, 20_000)) if nsym > 1 else b"\x05" * 5000, [(5000, 9, 3)])
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    deep = np.repeat(np.arange(24, dtype=np.uint8) + 33, fib)
    rng.shuffle(deep)
    cases["fibonacci_depth"] = (bytes(deep), [(deep.size, 3, 7)])
    cases["lits_incompressible"] = (bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), [(3000, 9000, 1)])
    cases["lits_incompressible_only"] = (bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), [])
    return cases


CRAFTED = crafted_cases()


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_sequences_decode(enc, dec, name):
    lits, seqs = CRAFTED[name]
    frame, content = E.encode_crafted(enc, lits, seqs)
    assert frame.size <= E.FRAME_HEADER + 3 + content.size
    assert int.from_bytes(bytes(frame[6:14]), "little") == content.size  # Frame_Content_Size
    both_decode(dec, frame, content)
    frame2, _ = E.encode_crafted(enc, lits, seqs)
    assert np.array_equal(frame, frame2)


def test_forms_chosen(enc):
    """The form the writer picks is the one the case is about: block type, literals type, size format, weight header."""
    def form(name):
        return E.first_block(E.encode_crafted(enc, *CRAFTED[name])[0])

    assert form("lits_incompressible_only")[0] == RAW                      # not smaller: Raw_Block
    assert form("lits_incompressible")[:2] == (COMPRESSED, LIT_RAW)        # Huffman saves nothing: Raw literals
    assert form("alphabet_1")[:2] == (COMPRESSED, LIT_RLE)
    assert form("lits_1_seq")[:3] == (COMPRESSED, LIT_RLE, 1)                # one literal is a one-symbol alphabet
    assert form("lits_255_seq")[:3] == (COMPRESSED, LIT_HUF, 0)            # 1 stream, 3-byte header
    assert form("lits_256_seq")[:3] == (COMPRESSED, LIT_HUF, 1)            # 4 streams, 3-byte header
    assert form("lits_1023_seq")[:3] == (COMPRESSED, LIT_HUF, 1)
    assert form("lits_1024_seq")[:3] == (COMPRESSED, LIT_HUF, 2)           # 4-byte header
    assert form("lits_16383_seq")[:3] == (COMPRESSED, LIT_HUF, 2)
    assert form("lits_16384_seq")[:3] == (COMPRESSED, LIT_HUF, 3)          # 5-byte header
    assert form("lits_full_block")[:3] == (COMPRESSED, LIT_HUF, 3)
    assert form("fibonacci_depth")[:2] == (COMPRESSED, LIT_HUF)
    assert form("alphabet_2")[:2] == (COMPRESSED, LIT_HUF) and form("alphabet_2")[3] == 128   # direct: one weight
    for nsym in (128, 129):  # 127 / 128 weights: both descriptions are legal, the smaller one is written
        assert form("alphabet_%d" % nsym)[:2] == (COMPRESSED, LIT_HUF)
    for nsym in (130, 256):  # more than 128 weights: only the FSE-compressed description exists
        f = form("alphabet_%d" % nsym)
        assert f[:2] == (COMPRESSED, LIT_HUF) and f[3] < 128
    # raw / RLE literal headers of 1, 2 and 3 bytes
    for nl, sf in ((31, (1,)), (32, (2,)), (3000, (2,))):
        lits = bytes(np.random.default_rng(nl).integers(0, 256, nl, dtype=np.uint8))
        fb = E.first_block(E.encode_crafted(enc, lits, [(nl, 2 * nl + 50, 1)])[0])
        assert fb[:2] == (COMPRESSED, LIT_RAW) and fb[2] in sf
    lits = bytes(np.random.default_rng(5).integers(0, 256, 5000, dtype=np.uint8))
    assert E.first_block(E.encode_crafted(enc, lits, [(5000, 9000, 1)])[0])[:3] == (COMPRESSED, LIT_RAW, 3)
    assert E.first_block(E.encode_crafted(enc, b"\x07" * 5000, [(5000, 9, 1)])[0])[:3] == (COMPRESSED, LIT_RLE, 3)


def test_direct_weight_header_decodes(enc, dec):
    """Few symbols, low values: the direct 4-bit description is the smaller one."""
    rng = np.random.default_rng(3)
    lits = bytes(skewed(rng, 9, 4000))
    frame, content = E.encode_crafted(enc, lits, [(4000, 100, 17)])
    fb = E.first_block(frame)
    assert fb[:2] == (COMPRESSED, LIT_HUF) and fb[3] >= 128
    both_decode(dec, frame, content)


def block_lengths():
    rng = np.random.default_rng(21)
    src = text(rng, 2 * B + 5)
    return [(n, src[:n]) for n in (1, 2, 3, B - 1, B, B + 1, 2 * B + 5)]


@pytest.mark.parametrize("n,src", block_lengths(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_block_lengths(enc, dec, n, src):
    frame = E.encode_frame(enc, src)
    assert frame.size < n or n < 64
    both_decode(dec, frame, src)


def test_parsed_corpora(enc, dec):
    sizes = {}
    for name, data in D.corpora():
        data = np.ascontiguousarray(data, dtype=np.uint8)
        frame = E.encode_frame(enc, data)
        assert frame.size <= enc.ze_frame_bound(data.size)
        if data.size == 0:
            assert frame.size == 0
            continue
        both_decode(dec, frame, data)
        assert np.array_equal(frame, E.encode_frame(enc, data)), "two calls, two frames"
        sizes[name] = (data.size, frame.size, E.first_block(frame)[0])
    assert sizes["zeros"][2] == RLE and sizes["zeros"][1] == E.FRAME_HEADER + 4 * 3   # three RLE blocks
    assert sizes["random"][2] == RAW and sizes["random"][1] == E.FRAME_HEADER + 200_000 + 3 * 2
    # not a raw-literal writer: entropy coding alone has to shrink integer key / value records (no matches to speak of)
    assert sizes["kvint"][1] < 0.9 * sizes["kvint"][0]
    assert sizes["wide"][1] < 0.5 * sizes["wide"][0] and sizes["terasort"][1] < 0.25 * sizes["terasort"][0]


def test_equal_block_and_block_boundary(enc, dec):
    """All-equal blocks leave as RLE blocks whatever surrounds them; the Last_Block flag sits on the last one only."""
    rng = np.random.default_rng(8)
    src = np.concatenate([np.full(B, 9, np.uint8), text(rng, B), np.full(700, 3, np.uint8)])
    frame = E.encode_frame(enc, src)
    both_decode(dec, frame, src)
    h0 = int.from_bytes(bytes(frame[14:17]), "little")
    assert h0 & 1 == 0 and (h0 >> 1) & 3 == RLE and h0 >> 3 == B
    tail = int.from_bytes(bytes(frame[-4:-1]), "little")
    assert tail & 1 == 1 and (tail >> 1) & 3 == RLE and tail >> 3 == 700


def test_seeded_sequence_fuzz(enc, dec):
    """Random sequence lists over random alphabets: whatever the parse could hand to the entropy stages."""
    rng = np.random.default_rng(99)
    for round_ in range(60):
        nsym = int(rng.choice([1, 2, 3, 17, 100, 256]))
        nseq = int(rng.choice([0, 1, 2, 50, 500, 3000]))
        seqs, produced = [], 0
        for i in range(nseq):
            ll = int(rng.choice([0, 0, 1, 2, 5, 20, 300])) if produced else int(rng.integers(1, 50))
            produced += ll
            ml = int(rng.choice([3, 3, 4, 5, 8, 35, 130, 1000]))
            off = int(rng.integers(1, produced + 1)) if rng.random() < 0.8 else min(produced, int(rng.choice([1, 2, 3, 4])))
            if produced + ml > B - 40:
                produced -= ll
                break
            seqs.append((ll, ml, off))
            produced += ml
        nl = sum(s[0] for s in seqs) + int(rng.integers(0 if seqs else 1, 40))
        lits = bytes(skewed(rng, nsym, max(nl, nsym))[:nl]) if nsym > 1 else bytes([int(rng.integers(0, 256))]) * nl
        frame, content = E.encode_crafted(enc, lits, seqs)
        both_decode(dec, frame, content)


def test_address_sanitizer_build(enc, dec, tmp_path):
    """The same writer with -fsanitize=address,undefined, every buffer an exact-size heap allocation: the frames equal the
    plain build's, and the program ends without a report."""
    rng = np.random.default_rng(4)
    cases, want = [], []
    for name in sorted(CRAFTED):
        lits, seqs = CRAFTED[name]
        frame, content = E.encode_crafted(enc, lits, seqs)
        cases.append(("crafted", content, seqs, lits))
        want.append(frame)
    sources = [text(rng, n) for n in (1, 2, 3, 5, 63, 64, 65, 4095, B - 1, B, B + 1)]
    sources += [np.zeros(B + 9, np.uint8), rng.integers(0, 256, 70_001, dtype=np.uint8), skewed(rng, 256, 150_000)]
    sources += [data for name, data in D.corpora() if name in ("terasort", "wide", "kvint")]
    for src in sources:
        cases.append(("parse", src))
        want.append(E.encode_frame(enc, src))
    got = E.run_asan(cases, str(tmp_path))
    for case, g, w in zip(cases, got, want):
        assert np.array_equal(g, w), "the sanitised build wrote another frame (%s, %d bytes)" % (case[0], len(case[1]))
    for case, g in zip(cases[len(CRAFTED):], got[len(CRAFTED):]):
        both_decode(dec, g, case[1])


def test_key_9_and_abi_11_everywhere():
    from s3shuffle import codec

    def read(*p):
        return open(os.path.join(ROOT, *p)).read()

    header = read("include", "s3shuffle_codec.h")
    scala = read("scala", "org", "apache", "spark", "shuffle", "gpu", "S3SCodec.scala")
    assert int(re.search(r"S3S_OPT_ZSTD_COMPRESS\s*=\s*(\d+)", header).group(1)) == 9
    assert int(re.search(r"val OPT_ZSTD_COMPRESS = (\d+)", scala).group(1)) == 9
    assert codec.OPT_ZSTD_COMPRESS == 9 and codec.CODEC_ZSTD == 3
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11
    assert int(re.search(r"val ABI_VERSION = (\d+)", scala).group(1)) == 11
    keys = [int(m) for m in re.findall(r"^\s+S3S_OPT_\w+ = (\d+)", header, re.M)]
    assert 9 in keys and len(keys) == len(set(keys)), "two options share a key"
    core = read("spark-s3-shuffle_amd", "csrc", "zstd_encode_core.h")
    internal = read("spark-s3-shuffle_amd", "csrc", "s3s_internal.h")
    assert "kBlock = 1 << 17" in core and "kZstdBlock = 1 << 17" in internal       # one block size, stated twice
    assert "kFrameHeader = 14" in core and "kZstdFrameHeader = 14" in internal
