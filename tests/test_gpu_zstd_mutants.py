"""GPU: randomly mutated Zstandard frames (tests/zstd_mutants.py, the first 200 of each family) on the block path (key 13,
S3S_OPT_ZSTD_DECODE_VARIANT = 1), the staged path (key 15, S3S_OPT_ZSTD_DECODE_STAGED = 1, 6k) and the resumable stream decoder
(s3s_dstream_open_zstd, 6l), hundreds of workgroups side by side.  Each mutant is judged by the host models first, in this
process: whatever a call answers - status, out_len, bytes, at keys 13 and 15 both ways - is the serial host model's answer,
the read-only keys 14 and 16 count exactly the blocks the host builds of the two paths complete, and every destination sits
between canary bands that stay intact, refused or not.

Nothing here provokes a fault: an invalid frame is one the decoder refuses by its own checks (shown on the CPU first, with the
sanitizers, for ten times as many mutants of the same generator: tests/test_zstd_mutants_model.py).

Call-level rules the batched calls are shaped around, so that the counts are exact:
  * fewer than 4 x CUs non-empty partitions per call (at most 256 here), so the block path's floor of 10 blocks does not apply;
  * the single pass decodes a partition at a capacity of 8 x its compressed size + 4096 and counts the blocks of every partition
    that decodes there - the range's dst_capacity is looked at afterwards - so the models count at that capacity; no mutant
    outgrows it (asserted), or the call would start over in the two-pass form, which never stages;
  * the staging is sized from the call's compressed bytes and handed out first come, first served: the models get the call's
    budget, and the sum of what they hand out stays inside it (asserted), so no frame's entry depends on the order."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_block_parallel_lib as ZB  # noqa: E402
import zstd_model_lib as ZM  # noqa: E402
import zstd_mutants as M  # noqa: E402
import zstd_staged_lib as S  # noqa: E402
import zstd_stream_lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

ZSTD = 3
ADLER, CRC = 1, 2
OPT_VARIANT, OPT_BLOCKS, OPT_STAGED, OPT_STAGED_BLOCKS = 13, 14, 15, 16
SETTINGS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (key 13, key 15)
CANARY = 4096
SEED = 1
COUNT = 200
GUESS = 8  # the single pass's capacity per compressed byte (zstd_decompress.hip: kGuess)


@pytest.fixture()
def sc(gpu_codec):
    try:
        yield gpu_codec
    finally:
        gpu_codec.set_option(OPT_STAGED, 0)
        gpu_codec.set_option(OPT_VARIANT, 1)


def _set(codec, variant, staged):
    codec.set_option(OPT_VARIANT, variant)
    codec.set_option(OPT_STAGED, staged)
    assert (codec.get_option(OPT_VARIANT), codec.get_option(OPT_STAGED)) == (variant, staged)


class Judged:
    pass


_judged = {}


def judged(family, count=COUNT):
    """The mutants with the one-shot call's answer by the serial host model."""
    key = (family, count)
    if key not in _judged:
        sm = ZM.load()
        j = Judged()
        j.family = family
        j.mutants = M.mutants(family, SEED, count)
        j.comp = [np.frombuffer(b, np.uint8) for _, b, _, _ in j.mutants]
        j.cap = [cap for _, _, _, cap in j.mutants]
        j.free = [M.serial_free(sm, c) for c in j.comp]
        j.answer, j.outgrown = [], []
        for c, cap in zip(j.comp, j.cap):
            # the single pass: the partition at its guessed capacity, then the range's capacity
            rc, out = M.serial_at(sm, c, GUESS * c.size + 4096)
            j.outgrown.append(rc == -2)
            if rc == -2:  # the call starts over in the two-pass form: the size pass, the range's capacity, the decode pass
                rc, total = M.size_pass(sm, c)
                rc, out = (rc, None) if rc != 0 else (-2, None) if total > cap else M.serial_at(sm, c, total)
            elif rc == 0 and out.size > cap:
                rc, out = -2, None
            j.answer.append((rc, out))
        _judged[key] = j
    return _judged[key]


def expected_counts(parts):
    """{(key 13, key 15): (key 14, key 16)} for a call of these partitions: the host builds of the two paths at the single
    pass's capacity and with the call's staging budget, summed over the partitions that decode there."""
    bm, gm = ZB.load(), S.load()
    call_bytes = sum(p.size for p in parts if p.size >= 12)  # (zstd_decode_staged.hip: kMinStagedPartition)
    want = {s: [0, 0] for s in SETTINGS}
    demand = {False: np.zeros(3, np.int64), True: np.zeros(3, np.int64)}
    for comp in parts:
        if comp.size == 0:
            continue
        guess = GUESS * comp.size + 4096
        rb = ZB.decode(bm, comp, guess)
        assert rb.rc != -2, "a mutant outgrows the single pass's guess: the call would take the two-pass form"
        if rb.rc == 0:
            want[(1, 0)][0] += rb.path_blocks
        for block_path in (False, True):
            rg = S.decode(gm, comp, guess, block_path=block_path, budget=max(call_bytes, comp.size))
            assert rg.rc == rb.rc
            demand[block_path] += np.array([rg.table_blocks, rg.lit_bytes, rg.records])
            if rg.rc == 0:
                want[(1, 1) if block_path else (0, 1)][0] += rg.path_blocks
                want[(1, 1) if block_path else (0, 1)][1] += rg.staged_blocks
    caps = np.array(S.staging_caps(gm, call_bytes))
    assert np.all(demand[False] <= caps) and np.all(demand[True] <= caps), "the call's staging budget would decide which frames are staged"
    return {s: tuple(v) for s, v in want.items()}


def batched(codec, dev, ranges, algo=0):
    """ranges: [(partitions, dst_capacity)] -> [(status, out_len, bad partition, destination with its canary bands)]; one call"""
    args, dsts = [], []
    for parts, cap in ranges:
        index = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([p.size for p in parts], out=index[1:])
        img = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        sums = None
        if algo:
            sums = np.array([(zlib.adler32(p.tobytes()) if algo == ADLER else zlib.crc32(p.tobytes())) & 0xFFFFFFFF for p in parts], np.int64)
        d = dev.upload(np.full(cap + 2 * CANARY, 0xA5, np.uint8))
        dsts.append((d, cap))
        args.append((dev.upload(img), img.size, index, sums, d + CANARY, cap))
    assert len(args) <= 256
    res = codec.decompress_ranges_batch_device(ZSTD, algo, args, raise_on_error=False)
    out = [(st, n, bad, dev.download(d, cap + 2 * CANARY)) for (st, n, bad), (d, cap) in zip(res, dsts)]
    dev.free()
    return out


def check_range(got, want, where):
    """One range's answer against the model's (code, bytes or None); the canary bands whatever the answer."""
    st, n, _, buf = got
    code, out = want
    assert np.all(buf[:CANARY] == 0xA5) and np.all(buf[buf.size - CANARY:] == 0xA5), ("canary band damaged", where)
    assert st == code, (where, st, code)
    if code == 0:
        assert n == out.size and np.array_equal(buf[CANARY:CANARY + n], out), ("bytes", where)
        assert np.all(buf[CANARY + n:] == 0xA5), ("bytes behind out_len", where)


def same_entries(a, b, where):
    assert len(a) == len(b)
    for k, ((st1, n1, bad1, buf1), (st0, n0, bad0, buf0)) in enumerate(zip(a, b)):
        assert (st1, n1, bad1) == (st0, n0, bad0), ("the answer depends on keys 13 / 15", where, k)
        if st1 == 0:
            assert np.array_equal(buf1, buf0), ("the bytes depend on keys 13 / 15", where, k)


# ---- 1. batched, one range per mutant ---------------------------------------------------------------------------------------------
def mutant_calls(j):
    """The mutants as one range each, in the calls the rules above ask for: [(indices, expected keys or None)] - all that stay
    inside the single pass's guess in one call with exact counts; the few that outgrow it in a call of their own, which takes the
    two-pass form (key 16 is 0 there, key 14 is not compared)."""
    inside = [k for k in range(len(j.comp)) if not j.outgrown[k]]
    beyond = [k for k in range(len(j.comp)) if j.outgrown[k]]
    assert len(beyond) <= len(j.comp) // 20
    return [(inside, expected_counts([j.comp[k] for k in inside]))] + ([(beyond, None)] if beyond else [])


def run_mutant_calls(sc, dev, j, calls, variant, staged, algo=0):
    _set(sc, variant, staged)
    got = [None] * len(j.comp)
    for indices, want in calls:
        res = batched(sc, dev, [([j.comp[k]], j.cap[k]) for k in indices], algo)
        keys = (sc.get_option(OPT_BLOCKS), sc.get_option(OPT_STAGED_BLOCKS))
        for k, g in zip(indices, res):
            check_range(g, j.answer[k], (j.family, k, variant, staged, algo))
            got[k] = g
        print(j.family, "keys 13, 15 =", (variant, staged), "keys 14, 16 =", keys, "models", want and want[(variant, staged)])
        if want is None:
            assert keys[1] == 0
        else:
            assert keys == want[(variant, staged)], (j.family, variant, staged)
    return got


@pytest.mark.parametrize("family", M.FAMILIES)
def test_one_range_per_mutant(sc, family):
    from hipdev import Dev

    j = judged(family)
    calls = mutant_calls(j)
    want = calls[0][1]
    codes = [a[0] for a in j.answer]
    assert codes.count(0) >= COUNT // 10 and COUNT - codes.count(0) >= COUNT * 4 // 10, "a vacuous subset"
    if family in ("writer", "two_frames"):
        assert want[(1, 0)][0] > 0 and want[(1, 1)][0] == want[(1, 0)][0]
    if family != "writer":
        assert want[(1, 1)][1] > 0 and want[(0, 1)][1] >= want[(1, 1)][1]
    dev = Dev()
    first = None
    try:
        for variant, staged in SETTINGS:
            got = run_mutant_calls(sc, dev, j, calls, variant, staged)
            if first is None:
                first = got
            else:
                same_entries(got, first, (family, variant, staged))
    finally:
        dev.free()


# ---- 2. checksums over the mutated bytes: verify, then decode -----------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ADLER, CRC], ids=["adler32", "crc32"])
def test_checksums_on(sc, algo):
    from hipdev import Dev

    j = judged("two_frames")
    calls = mutant_calls(j)
    dev = Dev()
    try:
        for variant, staged in ((1, 1), (0, 0)):
            run_mutant_calls(sc, dev, j, calls, variant, staged, algo)
    finally:
        dev.free()


# ---- 3. one range of many partitions ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["flushed1500", "writer", "two_frames", "crafted"])
def test_one_range_of_many_partitions(sc, family):
    from hipdev import Dev

    j = judged(family)
    good = [k for k, (rc, _) in enumerate(j.free) if rc == 0 and not j.outgrown[k]]
    bad = [k for k, (rc, _) in enumerate(j.free) if rc != 0 and not j.outgrown[k]]  # (the call stays in the single pass)
    assert len(good) >= COUNT // 10 and bad and all(j.answer[k][0] != 0 for k in bad)
    rng = np.random.default_rng([SEED, M.FAMILIES.index(family), 3])
    refused = bad[int(rng.integers(0, len(bad)))]
    at = int(rng.integers(0, len(good) + 1))
    parts = [j.comp[k] for k in good]
    content = np.concatenate([j.free[k][1] for k in good])
    with_refused = parts[:at] + [j.comp[refused]] + parts[at:]
    cap = content.size + 300
    want = expected_counts(parts)
    dev = Dev()
    first = None
    try:
        for variant, staged in SETTINGS:
            _set(sc, variant, staged)
            got = batched(sc, dev, [(parts, cap)])
            keys = (sc.get_option(OPT_BLOCKS), sc.get_option(OPT_STAGED_BLOCKS))
            got += batched(sc, dev, [(with_refused, cap)])
            check_range(got[0], (0, content), (family, variant, staged))
            assert keys == want[(variant, staged)], (family, variant, staged)
            check_range(got[1], (j.answer[refused][0], None), (family, variant, staged, "with mutant %d at %d" % (refused, at)))
            if first is None:
                first = got
            else:
                same_entries(got, first, (family, variant, staged))
    finally:
        dev.free()


# ---- 4. the single-range entry points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["two_frames", "flushed4k"])
def test_single_range_entry_points(sc, family):
    import s3shuffle
    from hipdev import Dev

    j = judged(family)
    dev = Dev()
    try:
        _set(sc, 1, 1)
        for k in range(32):
            comp, cap, (code, out) = j.comp[k], j.cap[k], j.answer[k]
            index = np.array([0, comp.size], np.int64)
            try:  # host buffers
                got = sc.decompress_range(ZSTD, 0, comp, index, None, dst_capacity=cap)
                assert code == 0 and np.array_equal(got, out), (family, k)
            except s3shuffle.CodecError as e:
                assert e.code == code, (family, k, e.code, code)
            d = dev.upload(np.full(cap + 2 * CANARY, 0xA5, np.uint8))
            d_comp = dev.upload(comp)
            try:
                st, n = 0, sc.decompress_range_device(ZSTD, 0, d_comp, comp.size, index, None, d + CANARY, cap)
            except s3shuffle.CodecError as e:
                st, n = e.code, 0
            check_range((st, n, -1, dev.download(d, cap + 2 * CANARY)), (code, out), (family, k, "device"))
            dev.free()
    finally:
        dev.free()


# ---- 5. the stream ------------------------------------------------------------------------------------------------------------------
STREAM_CAP = 1 << 17
GUARD = 256
RECORD = 9984  # sizeof(ZStreamState) rounded to 256


def _stream(codec, dev, d_img, n, wlog, mode, cuts, d_dst, base):
    """One mutant through a stream, with the windows of tests/model/zstd_stream_model.cpp's run_case (as
    test_gpu_decode_stream_zstd.py's feed_all drives a valid range, but a code ends it): mode 1 - a feed per unit, one byte first
    and then what the feed asks for; mode 0 - the window ends at the next of `cuts` whenever a feed consumes nothing.
    -> (code, output)"""
    import s3shuffle

    lib = codec._lib
    index = np.array([0, n], np.int64)
    cuts = ([] if mode else list(cuts)) + [n]
    ci, wend = 0, (min(n, 1) if mode else cuts[0])
    out, code = [], 0
    s = s3shuffle.DecodeStream(codec, ZSTD, 0, index, None, window_log_max=wlog)
    try:
        for _ in range(1 << 16):
            pos = s.position
            if pos >= n:
                break
            consumed = need = 0
            if wend > pos:
                dev.fill(d_dst, 0xA5, STREAM_CAP + 2 * GUARD)
                try:
                    r = s.feed_device(d_img + pos, wend - pos, d_dst + GUARD, STREAM_CAP)
                except s3shuffle.CodecError as e:
                    code = e.code
                    r = s.last_result
                    assert (r.consumed, r.out_len) == (0, 0) and s.position == pos
                    # (inside dst a refused feed may leave what the units in front of the bad one decoded to: the header
                    # promises nothing about dst after an error; outside it nothing is written)
                    assert (dev.download(d_dst, GUARD) == 0xA5).all() and (dev.download(d_dst + GUARD + STREAM_CAP, GUARD) == 0xA5).all()
                    break
                assert r.code == 0, "a block always fits the feed's capacity"
                got = dev.download(d_dst, STREAM_CAP + 2 * GUARD)
                assert (got[:GUARD] == 0xA5).all() and (got[GUARD + r.out_len:] == 0xA5).all(), "a byte outside dst[0, out_len) was written"
                out.append(got[GUARD:GUARD + r.out_len].copy())
                held = s.held_device_bytes
                assert held <= (1 << wlog) + RECORD and lib.s3s_dstream_held_bytes(None) - base == held
                consumed, need = r.consumed, r.need_comp
            if consumed > 0:
                if mode:
                    wend = min(n, s.position + 1)
                continue
            assert wend < n, "no progress with the whole rest in the window"
            if mode:
                assert pos + need > wend, "need_comp did not grow"
                wend = min(n, pos + need)
            else:
                while cuts[ci] <= wend:
                    ci += 1
                wend = cuts[ci]
        else:
            raise AssertionError("the stream makes no progress")
    finally:
        s.close(check=False)
    assert lib.s3s_dstream_held_bytes(None) == base, "close did not give the history back"
    return code, (np.concatenate(out) if out else np.zeros(0, np.uint8))


@pytest.mark.parametrize("family", ["flushed4k", "wlog10", "two_frames"])
def test_stream(sc, family, tmp_path):
    from hipdev import Dev

    n_mutants = 100
    wlog = 10 if family == "wlog10" else 19
    mutants = M.mutants(family, SEED, n_mutants)
    cuts = M.seeded_cuts(family, SEED, mutants)
    reports = {mode: L.run_report([(b, wlog, STREAM_CAP, mode, c if mode == 0 else []) for (_, b, _, _), c in zip(mutants, cuts)],
                                  str(tmp_path), sanitized=False) for mode in (1, 0)}
    for mode in (1, 0):
        codes = [code for code, _, _ in reports[mode]]
        assert set(codes) <= {0, -3, -6} and codes.count(0) >= n_mutants // 10 and codes.count(-3) >= n_mutants * 4 // 10
    dev = Dev()
    base = sc._lib.s3s_dstream_held_bytes(None)
    try:
        d_dst = dev.alloc(STREAM_CAP + 2 * GUARD)
        for (index, data, _, _), c in zip(mutants, cuts):
            d_img = dev.upload(np.frombuffer(data, np.uint8))
            for mode in (1, 0):
                code, out = _stream(sc, dev, d_img, len(data), wlog, mode, c, d_dst, base)
                want = reports[mode][index]
                assert (code, out.size, zlib.crc32(out.tobytes())) == want, (family, index, "a feed per unit" if mode else "seeded cuts", code, out.size, want)
            dev.release(d_img)
    finally:
        dev.free()
    # the context is intact
    good, content, _ = S.crafted("fcs")
    assert np.array_equal(sc.decompress_range(ZSTD, 0, good, np.array([0, good.size], np.int64), None, dst_capacity=4096), content)
