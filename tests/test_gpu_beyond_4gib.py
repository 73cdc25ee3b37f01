"""Calls above 4 GiB through the device entry points of the C-ABI: source offsets, image offsets, slot offsets, frame
offsets, checksum range starts and range lengths beyond 2^31 and 2^32, and a source buffer whose device addresses carry
from the low into the high dword inside a cluster of small partitions.

Input: corpus.BigMapOutput — a little over 5 GiB, regenerated group by group (256 MiB) from (seed, partition); 82 % of it
incompressible, so that the compressed image passes 2^32 + 64 MiB as well (two thirds of 5 GiB would leave it at 3.7 GiB).  Reference: the oracle, group by group (the image of
a map output is the concatenation of its partitions' streams, the index their running sum); a group's bytes are compared
through their BLAKE2b digests, so that neither side is ever held whole on the host.  liblz4 itself for the 1 MiB blocks,
zlib / the oracle's CRC32C for the checksum ranges.  Never the library's own output on a smaller call.

Every buffer is a real allocation of the size the call is told; destinations are painted 0xA5 and sit between 4 KiB guards
that are checked after the call.  Run with -s to see which partition holds each boundary and the wall time per case
(profiles/beyond_4gib_gpu_tests.txt)."""
import hashlib
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import corpus

pytestmark = pytest.mark.gpu

LZ4, SNAPPY = 1, 2
ADLER, CRC, CRC32C = 1, 2, 3
OPT_LZ4_BLOCK_SIZE, OPT_LZ4_VARIANT, OPT_DECODE_VARIANT, OPT_LZ4_BLOCK_SIZE_LARGE = 1, 4, 5, 8
E_CHECKSUM, E_UNSUPPORTED = -4, -6
SEED = 4401
TOTAL = (5 << 30) + (96 << 20)
GROUP = 256 << 20
GUARD = 4096
B31, B32 = 1 << 31, 1 << 32
FLOOR = B32 + (64 << 20)  # what source and image must exceed
INTERIOR = [1 << 30, 3 << 30, 5 << 30]
RAW_SHARE = 0.82  # of the source: incompressible (stored frames), so that the image is above 2^32 + 64 MiB too
_POOL = ThreadPoolExecutor(8)


def _say(msg):
    print("[beyond-4gib] " + msg, flush=True)


def _digest(a):
    """BLAKE2b of every 16 MiB piece (hashed in parallel: hashlib releases the interpreter lock)"""
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    step = 16 << 20
    return tuple(_POOL.map(lambda o: hashlib.blake2b(a[o:o + step], digest_size=16).digest(), range(0, a.size, step)))


class _Guarded:
    """n bytes of device memory painted 0xA5 between two guards of 4 KiB"""

    def __init__(self, dev, n):
        self.dev, self.n = dev, int(n)
        self.base = dev.alloc(self.n + 2 * GUARD)
        dev.fill(self.base, 0xA5, self.n + 2 * GUARD)
        self.p = self.base + GUARD

    def check(self, what):
        lo, hi = self.dev.download(self.base, GUARD), self.dev.download(self.p + self.n, GUARD)
        assert (lo == 0xA5).all() and (hi == 0xA5).all(), "%s: bytes outside the destination changed" % what

    def free(self):
        self.dev.release(self.base)


class _Ref:
    pass


class _World:
    """the uploaded source, its layout, the references and the images the cases share"""

    def __init__(self):
        import s3shuffle
        from hipdev import Dev

        t0 = time.time()
        self.dev = Dev()
        self.codec = s3shuffle.Codec(0)  # (a context of its own: its workspace of several GiB goes with it)
        room = TOTAL + (8 << 20)         # (the last cluster of the layout may run a little over TOTAL)
        self.d_src = self.dev.alloc(room)
        x = (-self.d_src) % B32          # the source offset whose DEVICE ADDRESS is 4 GiB-aligned
        if x < (4 << 20):
            x += B32
        self.aligned_at = x
        assert (self.d_src + x) % B32 == 0 and x + (4 << 20) < TOTAL
        self.m = m = corpus.BigMapOutput(SEED, TOTAL, [B31, B32, x], INTERIOR, raw_share=RAW_SHARE)
        assert FLOOR < m.total <= room
        self.groups = m.groups(GROUP)
        self.goff = [int(m.offsets[p0]) for p0, _ in self.groups] + [m.total]
        self.src_digest = []
        for p0, p1 in self.groups:
            d = m.generate(p0, p1)
            assert d.size <= GROUP or p1 == p0 + 1
            self.dev.write(self.d_src + int(m.offsets[p0]), d)
            self.src_digest.append(_digest(d))
        self.refs, self.images = {}, {}
        _say("source: %d bytes (2^32 + %.1f MiB), %d partitions, %d groups, device address 0x%x, uploaded in %.1f s"
             % (m.total, (m.total - B32) / 2**20, m.n, len(self.groups), self.d_src, time.time() - t0))
        for name, at in (("2^31", B31), ("2^32", B32), ("4 GiB-aligned device address (source offset 0x%x)" % x, x)):
            p = m.holder(at)
            _say("source offset %s lies in partition %d (%d bytes, kind %d), %d bytes from its start"
                 % (name, p, m.sizes[p], m.kinds[p], at - m.offsets[p]))
            # inside a cluster of small partitions: neighbours on both sides within 1 MiB
            assert m.sizes[p] <= 200_000 and m.offsets[max(p - 3, 0)] >= at - (1 << 20) and m.offsets[min(p + 4, m.n)] <= at + (1 << 20)
        inner = [(at, m.holder(at)) for at in INTERIOR]
        inner = [(at, p) for at, p in inner if min(at - m.offsets[p], m.offsets[p + 1] - at) >= 65536 and m.sizes[p] >= (8 << 20)]
        assert inner, "no multiple of 2^30 in the interior of a large partition"
        for at, p in inner:
            _say("source offset %d x 2^30 lies in the interior of partition %d (%d bytes, kind %d)" % (at >> 30, p, m.sizes[p], m.kinds[p]))
        share = sum(int(s) for s, k in zip(m.sizes, m.kinds) if k == 0) / m.total
        assert RAW_SHARE - 0.03 < share < RAW_SHARE + 0.03, share
        _say("incompressible share of the source: %.2f" % share)

    def close(self):
        self.codec.close()
        self.dev.free()

    # ---- references -------------------------------------------------------------------------------------------------------------
    def _collect(self, results, what):
        """per-group (image bytes, index, sums) -> one _Ref for the whole map output"""
        r = _Ref()
        index, sums, r.goff, r.gdig = [0], [], [0], []
        for size, idx, s, dg in results:
            index += [int(v) + r.goff[-1] for v in idx[1:]]
            sums += [int(v) for v in s]
            r.goff.append(r.goff[-1] + size)
            r.gdig.append(dg)
        r.index, r.sums, r.total = np.array(index, np.int64), np.array(sums, np.int64), r.goff[-1]
        assert r.total > FLOOR, "%s: the image does not pass 2^32 + 64 MiB" % what
        _say("%s: image of %d bytes (2^32 + %.1f MiB)" % (what, r.total, (r.total - B32) / 2**20))
        for name, at in (("2^31", B31), ("2^32", B32)):
            p = int(np.searchsorted(r.index, at, side="right")) - 1
            _say("%s: image offset %s lies in partition %d (%d bytes of image, %d of source)"
                 % (what, name, p, r.index[p + 1] - r.index[p], self.m.sizes[p]))
        return r

    def reference(self, codec, algo, oracle):
        """the oracle's image (as digests per group), index and checksums of the whole map output at 32 KiB blocks"""
        if (codec, algo) not in self.refs:
            t0 = time.time()
            m = self.m

            def one(g):
                p0, p1 = g
                img, idx, sums = oracle.compress_map_output(codec, algo, m.generate(p0, p1), m.offsets[p0:p1 + 1] - m.offsets[p0])
                return img.size, idx, sums[:p1 - p0], _digest(img)

            with ThreadPoolExecutor(3) as pool:
                res = list(pool.map(one, self.groups))
            self.refs[(codec, algo)] = self._collect(res, "oracle codec %d checksum %d" % (codec, algo))
            _say("oracle reference codec %d checksum %d: %.1f s" % (codec, algo, time.time() - t0))
        return self.refs[(codec, algo)]

    def reference_liblz4(self, bs, algo):
        """liblz4's streams at block size bs (tests/lz4_u32_ref.py), zlib's checksums"""
        import lz4_u32_ref as R

        t0 = time.time()
        m = self.m

        def one(g):
            p0, p1 = g
            d, o = m.generate(p0, p1), m.offsets[p0:p1 + 1] - m.offsets[p0]
            img, idx, sums = R.expected_map_output([d[o[k]:o[k + 1]] for k in range(p1 - p0)], bs, algo)
            return len(img), idx, sums, _digest(np.frombuffer(img, np.uint8))

        with ThreadPoolExecutor(3) as pool:
            res = list(pool.map(one, self.groups))
        r = self._collect(res, "liblz4 at %d-byte blocks" % bs)
        _say("liblz4 reference: %.1f s" % (time.time() - t0))
        return r

    # ---- comparisons ------------------------------------------------------------------------------------------------------------
    def compare(self, d_ptr, base, groups, goff, gdig, what, explain=None):
        """device bytes [goff[g] - base, goff[g + 1] - base) at d_ptr against the digests of the groups in `groups`"""
        for g in groups:
            got = self.dev.download(d_ptr + goff[g] - base, goff[g + 1] - goff[g])
            if _digest(got) != gdig[g]:
                pytest.fail("%s: group %d (partitions %d..%d) differs from the reference%s"
                            % (what, g, self.groups[g][0], self.groups[g][1] - 1, explain(g, got) if explain else ""))

    def explain_image(self, codec, algo, oracle, ref):
        def explain(g, got):
            p0, p1 = self.groups[g]
            img, _, _ = oracle.compress_map_output(codec, algo, self.m.generate(p0, p1), self.m.offsets[p0:p1 + 1] - self.m.offsets[p0])
            n = min(img.size, got.size)
            d = np.flatnonzero(img[:n] != got[:n])
            if d.size == 0:
                return ": sizes %d / %d" % (got.size, img.size)
            at = int(d[0]) + ref.goff[g]
            p = int(np.searchsorted(ref.index, at, side="right")) - 1
            return ": first difference at image offset %d (0x%x), partition %d + %d, %d bytes differ in the group" % (
                at, at, p, at - ref.index[p], d.size)
        return explain

    def explain_source(self, g, got):
        p0, p1 = self.groups[g]
        want = self.m.generate(p0, p1)
        d = np.flatnonzero(want != got)
        at = int(d[0]) + self.goff[g]
        p = self.m.holder(at)
        return ": first difference at decoded offset %d (0x%x), partition %d + %d, %d bytes differ in the group" % (
            at, at, p, at - self.m.offsets[p], d.size)

    # ---- the compressed image of the whole map output -----------------------------------------------------------------------
    def compress_and_check(self, oracle, codec, algo, lz4_variant=None, keep=False):
        """case 1: s3s_compress_map_output_device on the whole source: image, index and checksums against the oracle"""
        ref = self.reference(codec, algo, oracle)
        m = self.m
        cap = self.codec.max_compressed_size(codec, m.offsets)
        assert cap >= ref.total
        buf = _Guarded(self.dev, cap)
        old = self.codec.get_option(OPT_LZ4_VARIANT)
        what = "compress codec %d checksum %d%s" % (codec, algo, " lz4 variant %d" % lz4_variant if lz4_variant else "")
        try:
            if lz4_variant is not None:
                self.codec.set_option(OPT_LZ4_VARIANT, lz4_variant)
            t0 = time.time()
            total, index, sums = self.codec.compress_map_output_device(codec, algo, self.d_src, m.offsets, buf.p, cap)
            _say("%s: %d -> %d bytes in %.2f s" % (what, m.total, total, time.time() - t0))
            assert total == ref.total and np.array_equal(index, ref.index), what + ": index differs from the oracle"
            self.compare(buf.p, 0, range(len(self.groups)), ref.goff, ref.gdig, what, self.explain_image(codec, algo, oracle, ref))
            assert np.array_equal(sums, ref.sums), what + ": checksums differ from the oracle"
            buf.check(what)
        except BaseException:
            buf.free()
            raise
        finally:
            self.codec.set_option(OPT_LZ4_VARIANT, old)
        if keep:
            self.images[(codec, algo)] = buf
        else:
            buf.free()
        return ref

    def image(self, oracle, codec, algo):
        """-> (device buffer of the verified image, its reference)"""
        if (codec, algo) not in self.images:
            self.compress_and_check(oracle, codec, algo, keep=True)
        return self.images[(codec, algo)], self.refs[(codec, algo)]

    def drop_image(self, codec, algo):
        self.images.pop((codec, algo)).free()


@pytest.fixture(scope="module")
def world(codec_lib):
    import s3shuffle

    if s3shuffle.device_count() < 1:
        pytest.fail("gpu-marked test running without a HIP device: there is no CPU fallback")
    w = _World()
    yield w
    w.close()


# ---- case 1: the whole map output through s3s_compress_map_output_device -----------------------------------------------------------
@pytest.mark.parametrize("codec,algo,variant", [(LZ4, CRC, None), (SNAPPY, ADLER, None), (LZ4, CRC, 1)],
                         ids=["lz4-crc32", "snappy-adler32", "lz4-crc32-general-batch"])
def test_compress_whole_map_output(world, oracle, codec, algo, variant):
    """source offsets, slot offsets (n_chunks x slot stride: 5 GiB) and image offsets all pass 2^31 and 2^32; the default LZ4
    run leaves most windows to the hand-written block, S3S_OPT_LZ4_VARIANT 1 takes the general batch alone"""
    t0 = time.time()
    if variant is None:
        world.image(oracle, codec, algo)
    else:
        world.compress_and_check(oracle, codec, algo, lz4_variant=variant)
    _say("case 1 (%d, %d, %s): %.1f s" % (codec, algo, variant, time.time() - t0))


# ---- case 2: 1 MiB LZ4 blocks (byU32 kernel, 1 MiB slots) against liblz4 -------------------------------------------------------
def test_lz4_one_mib_blocks_against_liblz4(world):
    """S3S_OPT_LZ4_BLOCK_SIZE_LARGE = 1 MiB on the same input: the byU32 kernel, slots of 1 MiB + 32 bytes whose offsets
    pass 2^32 after 4 096 chunks; expected streams from liblz4 itself, checksums from zlib"""
    t0 = time.time()
    w, m, bs = world, world.m, 1 << 20
    n_chunks = int(((m.sizes + bs - 1) // bs).sum())
    assert n_chunks > 4096 and n_chunks * (32 + bs) > FLOOR
    ref = w.reference_liblz4(bs, ADLER)
    old = w.codec.get_option(OPT_LZ4_BLOCK_SIZE_LARGE)
    w.codec.set_option(OPT_LZ4_BLOCK_SIZE_LARGE, bs)
    try:
        cap = w.codec.max_compressed_size(LZ4, m.offsets)
        buf = _Guarded(w.dev, cap)
        try:
            t1 = time.time()
            total, index, sums = w.codec.compress_map_output_device(LZ4, ADLER, w.d_src, m.offsets, buf.p, cap)
            _say("compress at 1 MiB blocks: %d -> %d bytes in %.2f s (%d chunks)" % (m.total, total, time.time() - t1, n_chunks))
            assert total == ref.total and np.array_equal(index, ref.index), "index differs from liblz4's"
            w.compare(buf.p, 0, range(len(w.groups)), ref.goff, ref.gdig, "1 MiB blocks")
            assert np.array_equal(sums, ref.sums), "checksums differ from zlib's over liblz4's streams"
            buf.check("1 MiB blocks")
        finally:
            buf.free()
    finally:
        w.codec.set_option(OPT_LZ4_BLOCK_SIZE_LARGE, old)
    _say("case 2: %.1f s" % (time.time() - t0))


# ---- case 3: the image as ONE fetched range ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,algo,variant", [(LZ4, CRC, 4), (LZ4, CRC, 3), (SNAPPY, ADLER, 4)],
                         ids=["lz4-batch", "lz4-ring", "snappy-batch"])
def test_decompress_whole_image_as_one_range(world, oracle, codec, algo, variant):
    """s3s_decompress_range_device with comp_len and out_len above 2^32: Frame.comp_off, frame_out[] and the checksum
    ranges pass 2^31 and 2^32; then one flipped byte in a partition beyond image offset 2^32 is S3S_E_CHECKSUM with exactly
    that partition's number"""
    import s3shuffle

    t0 = time.time()
    w, m = world, world.m
    img, ref = w.image(oracle, codec, algo)
    out = _Guarded(w.dev, m.total)
    old = w.codec.get_option(OPT_DECODE_VARIANT)
    w.codec.set_option(OPT_DECODE_VARIANT, variant)
    what = "decode codec %d variant %d" % (codec, variant)
    try:
        t1 = time.time()
        n = w.codec.decompress_range_device(codec, algo, img.p, ref.total, ref.index, ref.sums, out.p, m.total)
        _say("%s: %d -> %d bytes in %.2f s" % (what, ref.total, n, time.time() - t1))
        assert n == m.total
        w.compare(out.p, 0, range(len(w.groups)), w.goff, w.src_digest, what, w.explain_source)
        out.check(what)
        p = next(p for p in range(m.n) if ref.index[p] >= B32 + (1 << 20) and ref.index[p + 1] - ref.index[p] > 100)
        at = int(ref.index[p] + (ref.index[p + 1] - ref.index[p]) // 2)
        one = w.dev.download(img.p + at, 1).copy()
        try:
            w.dev.write(img.p + at, one ^ np.uint8(0x20))
            with pytest.raises(s3shuffle.CodecError) as e:
                w.codec.decompress_range_device(codec, algo, img.p, ref.total, ref.index, ref.sums, out.p, m.total)
            assert e.value.code == E_CHECKSUM and e.value.partition == p, (e.value.code, e.value.partition, p)
            _say("%s: byte at image offset 0x%x flipped -> S3S_E_CHECKSUM for partition %d" % (what, at, p))
        finally:
            w.dev.write(img.p + at, one)
        out.check(what + " (damaged)")
    finally:
        w.codec.set_option(OPT_DECODE_VARIANT, old)
        out.free()
        if codec == SNAPPY:
            w.drop_image(codec, algo)  # (its last user)
    _say("case 3 (%s): %.1f s" % (what, time.time() - t0))


# ---- case 4: the batched forms ---------------------------------------------------------------------------------------------------
def test_batched_calls_whose_sum_passes_4gib(world, oracle):
    """six map tasks / six fetched ranges of about 900 MiB each — every one below 2^31, their sum above 2^32 — through
    s3s_compress_map_outputs_batch_device and s3s_decompress_ranges_batch_device: what the packed TaskTail arrays and the
    batch-wide tile list see.  A task's image is the concatenation of its partitions' streams: every task equals the oracle's
    result for its own partitions."""
    t0 = time.time()
    w, m = world, world.m
    ref = w.reference(LZ4, CRC, oracle)
    runs, first = [], 0  # runs of whole groups, cut where the running size passes k / 6 of the total
    for g in range(len(w.groups)):
        if w.goff[g + 1] >= m.total * (len(runs) + 1) // 6:
            runs.append((first, g + 1))
            first = g + 1
    assert len(runs) == 6 and runs[-1][1] == len(w.groups)
    tasks, bufs, outs = [], [], []
    try:
        for g0, g1 in runs:
            p0, p1 = w.groups[g0][0], w.groups[g1 - 1][1]
            offs = m.offsets[p0:p1 + 1] - m.offsets[p0]
            assert (512 << 20) < offs[-1] < B31
            cap = w.codec.max_compressed_size(LZ4, offs)
            bufs.append(_Guarded(w.dev, cap))
            tasks.append((w.d_src + int(m.offsets[p0]), offs, bufs[-1].p, cap))
        assert sum(int(t[1][-1]) for t in tasks) == m.total > FLOOR
        t1 = time.time()
        res = w.codec.compress_map_outputs_batch_device(LZ4, CRC, tasks)
        _say("batched compress of 6 tasks: %.2f s" % (time.time() - t1))
        ranges = []
        for t, ((g0, g1), (total, index, sums)) in enumerate(zip(runs, res)):
            p0, p1 = w.groups[g0][0], w.groups[g1 - 1][1]
            base = int(ref.index[p0])
            assert total == ref.index[p1] - base and np.array_equal(index, ref.index[p0:p1 + 1] - base), "task %d: index" % t
            assert np.array_equal(sums, ref.sums[p0:p1]), "task %d: checksums" % t
            w.compare(bufs[t].p, base, range(g0, g1), ref.goff, ref.gdig, "batched compress, task %d" % t,
                      w.explain_image(LZ4, CRC, oracle, ref))
            bufs[t].check("batched compress, task %d" % t)
            outs.append(_Guarded(w.dev, int(tasks[t][1][-1])))
            ranges.append((bufs[t].p, total, index, sums, outs[-1].p, outs[-1].n))
        assert sum(r[1] for r in ranges) > FLOOR and all(r[1] < B31 for r in ranges)
        t1 = time.time()
        got = w.codec.decompress_ranges_batch_device(LZ4, CRC, ranges)
        _say("batched decode of 6 ranges: %.2f s" % (time.time() - t1))
        for t, ((g0, g1), (st, n, bad)) in enumerate(zip(runs, got)):
            assert (st, n, bad) == (0, outs[t].n, -1), (t, st, n, bad)
            w.compare(outs[t].p, w.goff[g0], range(g0, g1), w.goff, w.src_digest, "batched decode, range %d" % t, w.explain_source)
            outs[t].check("batched decode, range %d" % t)
    finally:
        for b in bufs + outs:
            b.free()
    _say("case 4: %.1f s" % (time.time() - t0))


# ---- case 5: checksum ranges whose starts and lengths pass 2^31 and 2^32 -----------------------------------------------------------
def test_checksum_ranges_over_the_whole_image(world, oracle):
    """s3s_checksum_ranges_device over the image of case 1: ranges that start and end around 2^31 and 2^32, and the whole
    image as ONE range (more than 262 144 segments of 16 KiB: the folded form, with more than 1 024 groups of 256 segments),
    all three algorithms, against zlib.crc32 / zlib.adler32 / the oracle's CRC32C run incrementally over the downloaded pieces"""
    t0 = time.time()
    w = world
    img, ref = w.image(oracle, LZ4, CRC)
    end = ref.total
    cuts = [0, 1, B31 - 5, B31 + 7, B32 - 1, B32 + 16385, end]
    assert cuts == sorted(cuts) and end > 262144 * 16384 and end > 1024 * 256 * 16384
    step = {ADLER: lambda b, v: zlib.adler32(b, v), CRC: lambda b, v: zlib.crc32(b, v),
            CRC32C: lambda b, v: oracle.crc32c(b, init=v)}
    start = {ADLER: 1, CRC: 0, CRC32C: 0}
    want = {a: [start[a]] * (len(cuts) - 1) for a in step}
    whole = dict(start)
    piece = 64 << 20
    for a0 in range(0, end, piece):
        buf = w.dev.download(img.p + a0, min(piece, end - a0))

        def run(algo):
            whole[algo] = step[algo](buf, whole[algo])
            for k in range(len(cuts) - 1):
                lo, hi = max(cuts[k], a0), min(cuts[k + 1], a0 + buf.size)
                if lo < hi:
                    want[algo][k] = step[algo](buf[lo - a0:hi - a0], want[algo][k])

        list(_POOL.map(run, list(step)))
    _say("checksum references over %d bytes: %.1f s" % (end, time.time() - t0))
    for algo in step:
        t1 = time.time()
        got = w.codec.checksum_ranges_device(algo, img.p, cuts)
        one = w.codec.checksum_ranges_device(algo, img.p, [0, end])
        _say("checksum algo %d: 6 ranges + the whole image in %.2f s" % (algo, time.time() - t1))
        assert [int(x) for x in got] == want[algo], (algo, [hex(int(x)) for x in got], [hex(x) for x in want[algo]])
        assert int(one[0]) == whole[algo], (algo, hex(int(one[0])), hex(whole[algo]))
    assert want[CRC][-1] != want[CRC][-2] and whole[CRC] != want[CRC][-1]  # (the ranges are not trivially alike)
    _say("case 5: %.1f s" % (time.time() - t0))


# ---- case 6: calls of more than 0x7fffff00 blocks / segments are refused before anything is touched ----------------------------
def test_calls_above_the_block_limit_are_refused(world):
    """compress_core (csrc/codec_api.hip) counts the codec blocks of the call on the host and refuses more than 0x7fffff00 of
    them in front of its first allocation; s3s_decompress_range_device (csrc/decode_api.hip) does the same with the checksum
    segments of the range.  The offsets describe terabytes, the buffers are small and real: a call that did NOT stop there
    would be told to read far outside them, so both checks were read before this test was written (and the second one moved in
    front of the staging allocation)."""
    import s3shuffle

    w = world
    small = w.dev.alloc(4096)
    dst = _Guarded(w.dev, 4096)
    old = w.codec.get_option(OPT_LZ4_BLOCK_SIZE)
    try:
        w.codec.set_option(OPT_LZ4_BLOCK_SIZE, 64)
        with pytest.raises(s3shuffle.CodecError) as e:  # 2^31 blocks of 64 bytes (+ the end frame) in one partition
            w.codec.compress_map_output_device(LZ4, CRC, small, [0, 64 << 31], dst.p, 4096)
        assert e.value.code == E_UNSUPPORTED, e.value
        w.codec.set_option(OPT_LZ4_BLOCK_SIZE, old)
        with pytest.raises(s3shuffle.CodecError) as e:  # two partitions of 2^30 checksum segments each
            w.codec.decompress_range_device(LZ4, CRC, small, 1 << 45, [0, 1 << 44, 1 << 45], [0, 0], dst.p, 4096)
        assert e.value.code == E_UNSUPPORTED, e.value
        dst.check("refused calls")
        assert (w.dev.download(dst.p, 4096) == 0xA5).all()
    finally:
        w.codec.set_option(OPT_LZ4_BLOCK_SIZE, old)
        dst.free()
        w.dev.release(small)
