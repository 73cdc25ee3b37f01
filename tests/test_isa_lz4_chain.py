"""The window block's chain (lz4_window_engine.inc: the next window's duplicate-hash passes run during the current window,
S3S_ENGINE_DUP_AHEAD; the run loop's layout, S3S_ENGINE_LAYOUT) in the COMPILED kernels on the CPU interpreter
(tests/isa/gfx950_emu.py: every global and LDS access bounds-checked), byte for byte against oracle.compress_map_output:
the input-ring kernel (variant 11) and the variant-10 kernel, on blocks of the bench generators and on the crafted chunks
of tests/lz4_chain_cases.py.  Needs hipcc (cross-compiles without a GPU) but no device."""
import os
import shutil
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "isa"))
sys.path.insert(0, HERE)
import lz4_chain_cases as cases  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None,
                                reason="hipcc not available")

LZ4, CRC = 1, 2
BUILDS = {"ring": True, "variant10": False}
OLD_HEAD = ("-DS3S_ENGINE_NO_DUP_AHEAD",)
_GEN = []


def _generated():
    if not _GEN:
        _GEN.append(cases.generated())
    return _GEN[0]


def _check(chunks, oracle, ring, **kw):
    """every chunk as a one-partition map output: the kernel's block (header without the xxHash32 the kernel is handed, and
    payload) against the first frame of oracle.compress_map_output's stream"""
    import lz4_chain_kernel as ck

    res = ck.compress_chunks(chunks, ring=ring, **kw)
    for c, (payload, hdr, w) in zip(chunks, res):
        img, index, _ = oracle.compress_map_output(LZ4, CRC, c, np.array([0, len(c)], dtype=np.int64), 32768)
        img = bytes(np.asarray(img, dtype=np.uint8))
        clen, olen = struct.unpack("<ii", img[9:17])
        assert olen == len(c) and len(img) == 21 + clen + 21
        assert hdr[8:17] == img[8:17], "token / lengths differ (len %d)" % len(c)
        if payload is None:
            assert clen == len(c), "kernel stored RAW a chunk the reference compresses"
        else:
            assert bytes(payload) == img[21:21 + clen], "kernel differs from the oracle (len %d)" % len(c)
    return res


def _visits(profile, label):
    """instructions executed behind the labels of the three window bodies that start with `label`"""
    return sum(v[0] for k, v in profile.items() if k.startswith(".Lw_" + label))


@pytest.mark.parametrize("workload", ["terasort", "tpcds-wide"])
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_generated_blocks(oracle, build, workload):
    prof = {}
    _check(_generated()[workload], oracle, BUILDS[build], profile=prof)
    assert _visits(prof, "winf") > 3 * 400 * 30, "the sequential head ran in nearly every window"
    assert _visits(prof, "exth") > 0 and _visits(prof, "extd") > 0 and _visits(prof, "leave") > 0


@pytest.mark.parametrize("case", sorted(cases.CRAFTED))
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_crafted_chunks(oracle, build, case):
    prof = {}
    _check(cases.CRAFTED[case](), oracle, BUILDS[build], profile=prof)
    assert _visits(prof, "winf") > 0, "the block ran whole windows one after the other"
    want = {"period64": ("commit", "leave"), "byte_runs": ("dupnone",), "ip_minus_2": ("pendb", "leave"), "no_event": ("noev",),
            "hand_back_and_skip": ("x2", "dispx", "winm"), "lengths": ("out0",)}[case]
    for label in want:
        assert _visits(prof, label) > 0, "the case no longer reaches .Lw_" + label


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_dead_partners_only_add_events(oracle, build):
    """a live lane whose hash partners are all dead is an event with the passes over all 64 lanes and none with the passes
    over the live lanes; it resolves through .Lw_dup -> .Lw_dupnone with the same bytes"""
    chunks = cases.byte_runs()
    new, old = {}, {}
    _check(chunks, oracle, BUILDS[build], profile=new)
    _check(chunks, oracle, BUILDS[build], profile=old, flags=OLD_HEAD)
    assert _visits(new, "dupnone") > _visits(old, "dupnone")


@pytest.mark.parametrize("case", ["hand_back_and_skip", "period64", "ip_minus_2"])
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_table_equals_the_sequential_passes(oracle, build, case):
    """the table a chunk leaves behind (mid-window hand-backs, one-window skips, commits into slots the early passes hold)
    equals the one the head's own two passes (-DS3S_ENGINE_NO_DUP_AHEAD) leave, slot for slot"""
    chunks = cases.CRAFTED[case]()
    new = _check(chunks, oracle, BUILDS[build])
    old = _check(chunks, oracle, BUILDS[build], flags=OLD_HEAD)
    for (_, _, wn), (_, _, wo) in zip(new, old):
        assert np.array_equal(wn.lds[:16384], wo.lds[:16384])


@pytest.mark.parametrize("order", ["reversed", "shuffled"])
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_lds_write_order(oracle, build, order):
    """which lane wins a same-address store is the hardware's choice: the passes must not depend on it"""
    rng = np.random.default_rng(7)
    f = (lambda n: np.arange(n)[::-1]) if order == "reversed" else (lambda n: rng.permutation(n))
    chunks = cases.period64()[:1] + cases.byte_runs()[:1] + [_generated()["terasort"][0][:4096]]
    _check(chunks, oracle, BUILDS[build], lds_order=f)


@pytest.mark.parametrize("flags", [(), ("-DS3S_ENGINE_LAYOUT_R6",), OLD_HEAD], ids=["default", "layout_r6", "no_dup_ahead"])
def test_each_part_alone(oracle, flags):
    """the A/B builds of the `exp` target produce the same bytes"""
    chunks = cases.hand_back_and_skip() + cases.period64()[:1] + [_generated()["tpcds-wide"][0][:4096]]
    _check(chunks, oracle, True, flags=flags)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_block_keeps_its_wait_states(build):
    import hazards
    import lz4_chain_kernel as ck
    import lz4_kernel as lk

    if BUILDS[build]:
        _, entry, text = ck.ring_program()
    else:
        text = lk.compile_asm()
        entry = lk.find_kernel(text, "lz4_compress_l2_kernelILb1E")
    asm_viol, cc_viol, _, _ = hazards.check_kernel(text, entry)
    assert not asm_viol, asm_viol[:5]
    assert not cc_viol, ("rule set stricter than the compiler", cc_viol[:3])
