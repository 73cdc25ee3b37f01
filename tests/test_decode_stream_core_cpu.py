"""CPU: the host arithmetic of the streaming reduce side (csrc/decode_stream_core.h), which the single feed and the batched feed
of csrc/decode_stream.hip both call.  tests/model/dstream_model.cpp plays a stream's host side with it as a stand-alone
program under AddressSanitizer and UBSan, with every array exactly as long as the library uses it; the kernels' part - discovery,
the capacity cut, the checksums, the decode status - is played here by the Python model of the contract
(stream_damage.Model.discover over the plain image, zlib over the stored bytes), over a pipe.  Every feed's answer is compared
field for field with stream_damage.Model.feed (plain), stream_damage_encrypted.feed (encrypted) and
stream_units_encrypted.expected_feed_none (S3S_CODEC_NONE under encryption), the position with the model's, and the carry with
the zlib sum of the open partition's stored bytes up to the new position.  One-token mutants of the header must each fail."""
import dataclasses
import os
import subprocess
import zlib

import numpy as np
import pytest

import stream_damage as sd
import stream_damage_encrypted as sde
import stream_units as su
import stream_units_encrypted as sue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc")
CORE = os.path.join(CSRC, "decode_stream_core.h")
MODEL = os.path.join(ROOT, "tests", "model", "dstream_model.cpp")
NONE, LZ4, SNAPPY, LZF = 0, sd.LZ4, sd.SNAPPY, sd.LZF
AMPLE = 1 << 18
IV = sue.IV


def _build(out_dir, include_dir=CSRC):
    exe = os.path.join(str(out_dir), "dstream_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", include_dir, MODEL, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("dstream"))


def test_the_header_builds_without_hip_and_allocates_nothing(tmp_path):
    text = open(CORE).read()
    code = "\n".join(line.split("//")[0] for line in text.split("\n"))
    includes = [line.split()[1] for line in code.split("\n") if line.startswith("#include")]
    assert sorted(includes) == ["<algorithm>", "<stdint.h>"]
    for word in ("s3s_ctx", "hip", "fail(", "new ", "malloc", "std::vector"):
        assert word not in code, word
    unit = tmp_path / "unit.cpp"
    unit.write_text('#include "decode_stream_core.h"\nint main() { return (int)s3s_ds::fresh(1) - 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(unit), "-o", str(tmp_path / "unit")], check=True)


# ---- the program, and the device it talks to ---------------------------------------------------------------------------------
class Dead(AssertionError):
    """the program stopped: a sanitizer report, or a rule that reads past what it was given"""


class Program:
    def __init__(self, exe, tmp_path):
        self.err = open(os.path.join(str(tmp_path), "stderr.txt"), "w+")
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=self.err, text=True, bufsize=1)
        self.feeds = 0

    def _line(self):
        line = self.p.stdout.readline()
        if not line:
            self.p.wait(timeout=60)
            self.err.seek(0)
            raise Dead("the model program stopped (exit %s): %s" % (self.p.returncode, self.err.read()[-3000:]))
        return line.split()

    def _send(self, words):
        try:
            self.p.stdin.write(" ".join(str(int(w)) for w in words) + "\n")
            self.p.stdin.flush()
        except BrokenPipeError:
            self._line()

    def open(self, codec, algo, enc, off, ref):
        self.p.stdin.write("R %d %d %d %d\n" % (codec, algo, int(enc), len(off) - 1))
        self._send(list(off) + list(ref))

    def feed(self, w, cap, device, algo, stored):
        """-> the answer; device(d) -> the ten words of the kernels; the sums are zlib's over `stored`, the window's stored bytes"""
        self.p.stdin.write("F %d %d\n" % (w, cap))
        self.p.stdin.flush()
        self.feeds += 1
        t = self._line()
        if t[0] == "D":
            v = [int(x) for x in t[1:]]
            d = dict(zip(("ppos", "PL", "pleft", "first_mid", "plast_pend", "n", "m"), v[:7]))
            n, m, rest = d["n"], d["m"], v[7:]
            d["off"], d["seed"], rest = rest[:n + 1], rest[n + 1:2 * n + 1], rest[2 * n + 1:]
            d["q"], d["c"] = rest[:m + 1], rest[m + 1:]
            assert len(d["seed"]) == n and len(d["c"]) in (0, m)
            sums = [_sum(algo, stored[d["off"][i]:d["off"][i + 1]], d["seed"][i]) for i in range(n)]
            self._send(list(device(d)) + sums)
            t = self._line()
            if t[0] == "S":
                a, b, seed = (int(x) for x in t[1:])
                assert 0 <= a < b <= len(stored) and algo
                self._send([_sum(algo, stored[a:b], seed)])
                t = self._line()
        assert t[0] == "A", t
        return dict(zip(("code", "consumed", "out_len", "need_comp", "need_dst", "bad", "at_end", "pos", "cur", "carry"), (int(x) for x in t[1:])))

    def close(self):
        self.p.stdin.close()
        rc = self.p.wait(timeout=60)
        self.err.seek(0)
        text = self.err.read()
        assert rc == 0 and not text, text[-3000:]


def _sum(algo, data, seed):
    if not algo:
        return 0
    return (zlib.adler32(data, seed) if algo == sd.ADLER else zlib.crc32(data, seed)) & 0xFFFFFFFF


def _fresh(algo):
    return 1 if algo == sd.ADLER else 0


def _kernels(model, c, ppos, PL, cap):
    """the words of discovery, the cut and the decoders over the plain window [ppos, ppos + PL) of the case's plain image"""
    if PL == 0 or c.codec == NONE:
        return [0] * 10
    k = model.discover(c.codec, c.img, c.index, 0, ppos, PL, cap)
    dec = 0
    if k["status"] == 0 and any(model.payload(c.codec, c.img, *u) is None for u in k["units"][:k["k"]]):
        dec = sd.E_BAD_FRAME
    cut = [0, k["k"], k["consumed"], k["out_len"], k["need_dst"]]
    return [k["status"], k["stop"], k["need"], k["n_frames"]] + cut + [dec]


FIELDS = ("code", "consumed", "out_len", "need_comp", "need_dst", "bad", "at_end")


def _open_carry(algo, img, index, pos, cur):
    return _sum(algo, img[index[cur]:pos], _fresh(algo)) if cur < len(index) - 1 else _fresh(algo)


class PlainStream:
    """one stream of the program next to sd.Model.feed; refs: the reference checksums it was opened with"""

    def __init__(self, prog, model, c, algo):
        self.prog, self.model, self.c, self.algo = prog, model, c, algo
        self.st = dict(pos=0, cur=0, err=0, bad=-1)
        prog.open(c.codec, algo, False, c.index, model.ref_sums(c.image, algo) if algo else [0] * (len(c.index) - 1))

    def feed(self, w, cap):
        model, c, algo, st = self.model, self.c, self.algo, self.st
        pos, cur = st["pos"], st["cur"]

        def device(d):
            n, off, mid, pend = model.pieces(c.index, cur, pos, w)
            assert (d["ppos"], d["PL"], d["pleft"], d["n"], d["m"], d["off"]) == (pos, w, c.index[-1] - pos, n, n, off), d
            assert (d["first_mid"], d["plast_pend"]) == (int(mid), pend), d
            assert d["seed"] == [_open_carry(algo, c.img, c.index, pos, cur)] + [_fresh(algo)] * (n - 1), d
            return _kernels(model, c, pos, w, cap)

        want = model.feed(c, algo, st, w, cap)
        got = self.prog.feed(w, cap, device, algo, c.img[pos:pos + w])
        where = (c.name, algo, pos, cur, w, cap)
        assert tuple(got[f] for f in FIELDS) == tuple(want[f] for f in FIELDS), (where, got, want)
        assert (got["pos"], got["cur"]) == (st["pos"], st["cur"]), (where, got, st)
        assert got["carry"] == _open_carry(algo, c.img, c.index, st["pos"], st["cur"]), (where, got)
        return got


class EncCase(sde.EncCase):
    """sde.EncCase with partitions stored as their IV alone (iv_only: empty in the plain image)"""

    def __init__(self, c, iv_only=()):
        self.c = c
        n = len(c.index) - 1
        enc, eidx, _ = sue.encrypt(np.frombuffer(c.img, np.uint8), c.index, sde.KEY, sue.ivs_for(n, 700 + n), iv_only=iv_only)
        self.img, self.eidx = enc.tobytes(), [int(x) for x in eidx]
        self.total = self.eidx[-1]


def _min_unit_encrypted(codec, eidx, pos, cur):
    """need_comp of an empty window (include/s3shuffle_codec.h): the IV when the position stands in front of one, else the
    codec's smallest header"""
    start = eidx[min(cur, len(eidx) - 1)]
    if pos == start:
        return IV
    return {NONE: 1, LZ4: 21, LZF: 5}.get(codec, 16 if pos == start + IV else 4)


class EncStream:
    """one encrypted stream of the program next to sde.feed (checksums: the true ones, so none is wrong)"""

    def __init__(self, prog, model, e, algo):
        self.prog, self.model, self.e, self.algo = prog, model, e, algo
        self.st = dict(pos=0, plain=dict(pos=0, cur=0, err=0, bad=-1))
        self.cur = 0
        nparts = len(e.eidx) - 1
        prog.open(e.c.codec, algo, True, e.eidx, [_sum(algo, e.img[e.eidx[p]:e.eidx[p + 1]], _fresh(algo)) for p in range(nparts)])

    def feed(self, w, cap):
        model, e, algo, st, c = self.model, self.e, self.algo, self.st, self.e.c
        pos, cur = st["pos"], self.cur
        pidx = sue.plain_index(e.eidx)
        assert pidx == c.index
        ppos = pidx[cur] + max(pos - e.eidx[min(cur, len(pidx) - 2)] - IV, 0)  # the position in plain bytes
        assert c.codec == NONE or ppos == st["plain"]["pos"]

        def device(d):
            L = w
            if c.codec == NONE:  # a unit is a byte: the window is cut at the capacity before anything runs
                L = d["off"][-1]
                assert L in (w, sue.expected_feed_none(e.eidx, pos, w, cap)[0]), (d, w, cap)
            plain, segs, _ = e.window(pos, L)
            stored_len = [e.eidx[cur + i + 1] - e.eidx[cur + i] for i in range(d["m"])]
            assert d["PL"] == plain and d["q"][-1] == plain, (d, plain)
            assert [(d["ppos"] + d["q"][i], pos + d["c"][i]) for i in range(d["m"]) if stored_len[i]] == segs, (d, segs)
            if d["m"]:
                assert d["ppos"] == ppos, (d, ppos)
                assert d["first_mid"] == int(ppos > pidx[cur]) and d["plast_pend"] == pidx[cur + d["m"]] - ppos, (d, pidx, cur)
            assert d["pleft"] == pidx[-1] - d["ppos"], d
            return _kernels(model, c, d["ppos"], d["PL"], cap)

        if c.codec == NONE:
            consumed, out_len = sue.expected_feed_none(e.eidx, pos, w, cap)
            want = dict(code=sd.OK, consumed=consumed, out_len=out_len, need_comp=0, need_dst=0, bad=-1, at_end=0)
            if w > 0 and consumed == 0:  # nothing whole in the window: a cut IV is waited for, a byte that dst cannot hold is refused
                nxt = next((a for a, b in zip(e.eidx, e.eidx[1:]) if b > a and a >= pos), None)
                if nxt == pos and pos + IV > pos + w:
                    want["need_comp"] = IV
                else:
                    want.update(code=sd.E_CAPACITY, need_dst=1)
            st["pos"] = pos + consumed
            want["at_end"] = int(st["pos"] == e.total and want["code"] == sd.OK)
        else:
            want = sde.feed(model, e, st, w, cap)
        got = self.prog.feed(w, cap, device, algo, e.img[pos:pos + w])
        where = (c.name, algo, pos, cur, w, cap)
        if w == 0:
            want["need_comp"] = _min_unit_encrypted(c.codec, e.eidx, got["pos"], got["cur"]) if got["pos"] < e.total else 0
        assert tuple(got[f] for f in FIELDS) == tuple(want[f] for f in FIELDS), (where, got, want)
        assert got["pos"] == st["pos"], (where, got, st)
        assert got["carry"] == _open_carry(algo, e.img, e.eidx, got["pos"], got["cur"]), (where, got)
        self.cur = got["cur"]
        return got


# ---- ranges -------------------------------------------------------------------------------------------------------------------
def _shaped(image):
    """the cut-position image with an empty partition at the start, two in the middle and one at the end -> (case, the middle
    empty one that is stored as its IV alone under encryption)"""
    idx = image.index
    index = [0, 0, idx[1], idx[1], idx[1]] + idx[2:] + [idx[-1]]
    shaped = dataclasses.replace(image, name=image.name + "-shaped", index=index)
    return sd.Case(shaped.name, shaped, shaped.img, index, (0, 0, 0), (0, 0)), 2


@pytest.fixture(scope="module")
def ranges(oracle):
    """[(case, iv_only partition)] for LZ4, Snappy and LZF: the cut-position images of tests/test_isa_decode_stream.py"""
    base = {i.name: i for i in sd.images(oracle)}
    return [_shaped(base[name]) for name in ("lz4", "snappy", "lzf")]


def _none_case(ranges):
    c = ranges[0][0]
    image = dataclasses.replace(c.image, name="none-shaped", codec=NONE, img=c.img[:3000], index=[0, 0, 1500, 1500, 1500, 3000, 3000])
    return sd.Case(image.name, image, image.img, image.index, (0, 0, 0), (0, 0))


def _algo(c):
    return sd.CRC if c.image.crc else sd.ADLER


# ---- every window end from position 0 -------------------------------------------------------------------------------------------
def _sweep_plain(prog, model, c, algo, ends):
    for w in ends:
        s = PlainStream(prog, model, c, algo)
        got = s.feed(w, AMPLE)
        if got["code"] == sd.OK:
            s.feed(c.index[-1] - got["pos"], AMPLE)  # the rest: the carry and the position of the first feed are what it starts from


def _sweep_encrypted(prog, model, e, algo, ends):
    for w in ends:
        s = EncStream(prog, model, e, algo)
        got = s.feed(w, AMPLE)
        if got["code"] == sd.OK:
            s.feed(e.total - got["pos"], AMPLE)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["lz4", "snappy", "lzf"])
def test_every_window_end_plain(oracle, model_exe, ranges, tmp_path, which):
    c = ranges[which][0]
    prog, model = Program(model_exe, tmp_path), sd.Model(oracle)
    _sweep_plain(prog, model, c, _algo(c), range(1, c.index[-1] + 1))
    prog.close()
    assert prog.feeds >= 2 * c.index[-1] - 1


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["lz4", "snappy", "lzf", "none"])
def test_every_window_end_encrypted(oracle, model_exe, ranges, tmp_path, which):
    """the stored range: [empty][IV + A][IV alone][empty][IV + B] ... [empty] - every window end falls 1 .. 15 bytes into each IV"""
    c, iv_only = (_none_case(ranges), 2) if which == 3 else ranges[which]
    e = EncCase(c, (iv_only,))
    assert e.eidx[iv_only + 1] - e.eidx[iv_only] == IV and e.eidx[1] == 0 and e.eidx[-1] == e.eidx[-2]
    prog, model = Program(model_exe, tmp_path), sd.Model(oracle)
    _sweep_encrypted(prog, model, e, sd.ADLER if which % 2 else sd.CRC, range(1, e.total + 1))
    prog.close()
    assert prog.feeds >= 2 * e.total - 1


# ---- random schedules ------------------------------------------------------------------------------------------------------------
def _schedule(rng, stream, units, total, pos_of):
    """the shape of test_compress_stream_cpu._schedule: windows in {0, 1, unit - 1, unit, unit + 1, random, rest}, capacities in
    {0, 1, first unit - 1, first unit, random, ample}; units: [(start, length, decoded)] in the stream's coordinates"""
    for _ in range(300):
        pos = pos_of()
        nxt = next((u for u in units if u[0] >= pos), (pos, 1, 1))
        dec = next((u[2] for u in units if u[0] >= pos and u[2] > 0), 1)
        w = min(int(rng.choice([0, 1, nxt[1] - 1, nxt[1], nxt[1] + 1, int(rng.integers(0, 3 * nxt[1] + 40)), total])), total - pos)
        cap = int(rng.choice([0, 1, dec - 1, dec, int(rng.integers(0, 3 * dec + 2)), AMPLE]))
        got = stream.feed(max(w, 0), cap)
        if got["at_end"] or got["code"] not in (sd.OK, sd.E_CAPACITY):
            return got
    return None


@pytest.mark.parametrize("which", [0, 1, 2], ids=["lz4", "snappy", "lzf"])
def test_random_schedules_plain(oracle, model_exe, ranges, tmp_path, which):
    c = ranges[which][0]
    prog, model, rng = Program(model_exe, tmp_path), sd.Model(oracle), np.random.default_rng(40 + which)
    units = su.units(c.codec, c.img, c.index)
    ended = 0
    for i in range(40):
        s = PlainStream(prog, model, c, (sd.ADLER, sd.CRC, 0)[i % 3])
        last = _schedule(rng, s, units, c.index[-1], lambda: s.st["pos"])
        ended += bool(last and last["at_end"])
    prog.close()
    assert ended >= 20


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["lz4", "snappy", "lzf", "none"])
def test_random_schedules_encrypted(oracle, model_exe, ranges, tmp_path, which):
    c, iv_only = (_none_case(ranges), 2) if which == 3 else ranges[which]
    e = EncCase(c, (iv_only,))
    prog, model, rng = Program(model_exe, tmp_path), sd.Model(oracle), np.random.default_rng(60 + which)
    if c.codec == NONE:  # a unit is a byte, or an IV
        units = [(a, IV, 0) for a, b in zip(e.eidx, e.eidx[1:]) if b > a]
    else:
        units = sue.stored_units(c.codec, c.img, e.eidx)
    ended = 0
    for i in range(40):
        s = EncStream(prog, model, e, (sd.CRC, sd.ADLER, 0)[i % 3])
        if i % 4 == 1:  # the IV alone: the next window starts exactly behind it
            assert s.feed(IV, AMPLE)["consumed"] == IV
        last = _schedule(rng, s, units, e.total, lambda: s.st["pos"])
        ended += bool(last and last["at_end"])
    prog.close()
    assert ended >= 20


# ---- a partition shorter than an IV -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [1, 15])
def test_a_partition_shorter_than_its_iv(oracle, model_exe, ranges, tmp_path, short):
    """[IV + A][`short` stored bytes][IV + B]: corrupt, reported by the feed that consumes everything in front of the short
    partition (include/s3shuffle_codec.h); a feed that stops earlier - the capacity, or a window that does not show it - is
    an ordinary feed, and for discovery the plain side ends there (a unit that would cross it is corrupt, not cut)."""
    c = ranges[0][0]
    a_end = c.index[2]  # partition A of the LZ4 image, plain
    plain_a = dataclasses.replace(c.image, name="lz4-A", img=c.img[:a_end], index=[0, a_end])
    ca = sd.Case("lz4-A", plain_a, plain_a.img, plain_a.index, (0, 0, 0), (0, 0))
    e = EncCase(ca)
    tail = EncCase(c).img[-200:]
    e.img = e.img + bytes(short) + tail
    e.eidx = e.eidx + [e.total + short, e.total + short + len(tail)]
    stored_a, total = e.total, e.eidx[-1]
    units = su.units(LZ4, ca.img, ca.index)
    model = sd.Model(oracle)

    def run(feeds):
        prog = Program(model_exe, tmp_path)
        prog.open(LZ4, 0, True, e.eidx, [0, 0, 0])
        pos, out = 0, []
        for w, cap in feeds:
            def device(d):
                # shown, the short partition ends the plain side; else it counts as empty, like every partition without plain bytes
                assert d["pleft"] == (d["PL"] if pos + w > stored_a else a_end + len(tail) - IV - d["ppos"]), d
                return _kernels(model, ca, d["ppos"], d["PL"], cap)
            got = prog.feed(w, cap, device, 0, e.img[pos:pos + w])
            pos = got["pos"]
            out.append(tuple(got[f] for f in FIELDS))
        prog.close()
        return out

    ok_all = (sd.OK, stored_a, sum(u[2] for u in units), 0, 0, -1, 0)
    corrupt = (sd.E_BAD_FRAME, 0, 0, 0, 0, -1, 0)
    first = units[0]
    # the window does not show the short partition: an ordinary feed; the next one starts at it
    assert run([(stored_a, AMPLE), (total - stored_a, AMPLE), (1, AMPLE)]) == [ok_all, corrupt, corrupt]
    assert run([(stored_a, AMPLE), (1, AMPLE)]) == [ok_all, corrupt]
    # the window shows it (one byte of it, or all of the range): the feed that would take all of A is the one that fails
    assert run([(stored_a + 1, AMPLE)]) == [corrupt] and run([(total, AMPLE)]) == [corrupt]
    # ... a feed that the capacity ends earlier does not
    partial = (sd.OK, IV + first[1], first[2], 0, 0, -1, 0)
    assert run([(total, first[2]), (total - IV - first[1], AMPLE)]) == [partial, corrupt]


# ---- damage: one wrong reference checksum; the ordering rule ----------------------------------------------------------------------
def _wrong_ref(c, p):
    """the case with partition p's reference checksum taken over other bytes (the image the references come from differs in
    one byte of that partition)"""
    a = c.index[p]
    other = c.img[:a] + bytes([c.img[a] ^ 0x55]) + c.img[a + 1:]
    return dataclasses.replace(c, name="%s/wrong-ref-%d" % (c.name, p), image=dataclasses.replace(c.image, img=other, index=c.index))


@pytest.mark.parametrize("name", ["lz4-empties", "snappy-empties", "lzf-empties"])
def test_one_wrong_reference_checksum(oracle, model_exe, tmp_path, name):
    """partitions of 700, 0, 8223, 0 and 900 source bytes; the feed is ended by the window (inside partition 2, at its end, behind
    it) or by the capacity (inside partition 2): the wrong reference lies before, at and behind that point"""
    image = next(i for i in sd.images(oracle) if i.name == name)
    c = sd.Case(name, image, image.img, image.index, (0, 0, 0), (0, 0))
    units = su.units(c.codec, c.img, c.index)
    mid = [u for u in units if c.index[2] <= u[0] < c.index[3] and u[2] > 0]
    total = c.index[-1]
    at = mid[len(mid) // 2]  # the unit of partition 2 that the window's end or the capacity cuts off
    front = sum(u[2] for u in units if u[0] < at[0])
    prog, model = Program(model_exe, tmp_path), sd.Model(oracle)
    codes = set()
    for p in (0, 2, 4):
        bad = _wrong_ref(c, p)
        for algo in (sd.ADLER, sd.CRC):
            for w, cap in ((at[0] + 3, AMPLE), (c.index[3], AMPLE), (c.index[3] + 5, AMPLE), (total, front), (total, AMPLE)):
                s = PlainStream(prog, model, bad, algo)
                got = s.feed(w, cap)
                while got["code"] == sd.OK and not got["at_end"]:
                    got = s.feed(total - got["pos"], AMPLE)
                assert (got["code"], got["bad"]) == (sd.E_CHECKSUM, p)
                codes.add((p, s.st["pos"] > 0))
                assert s.feed(1, 1)["code"] == sd.E_CHECKSUM  # sticky
    prog.close()
    assert {p for p, _ in codes} == {0, 2, 4} and {late for _, late in codes} == {False, True}  # in the first feed, and in a later one


@pytest.mark.parametrize("cls", [sd.HEADER_INVALID, sd.OVERSIZED, sd.PAYLOAD_INVALID], ids=["bad-frame", "unsupported", "decode-status"])
def test_a_wrong_checksum_comes_before_corruption_and_refusal(oracle, model_exe, tmp_path, cls):
    """discovery's S3S_E_BAD_FRAME and S3S_E_UNSUPPORTED and a non-zero decode status, each with and without a wrong checksum of
    a partition whose last byte the window holds"""
    picked = {}
    for c in sd.cases(oracle):
        if c.cls == cls and c.index == c.image.index and c.image.name in ("lz4", "snappy", "lzf") and (cls != sd.OVERSIZED or c.claim > sd.K_MAX):
            picked.setdefault(c.codec, c)
    assert picked
    prog, model = Program(model_exe, tmp_path), sd.Model(oracle)
    seen = set()
    for c in picked.values():
        total, algo = c.index[-1], _algo(c)
        true_refs = dataclasses.replace(c, image=dataclasses.replace(c.image, img=c.img))  # the references are the damaged range's own
        for case, windows in ((true_refs, (total,)), (c, (total, min(c.unit[0] + c.unit[1] + 1, total)))):
            for w in windows:
                s = PlainStream(prog, model, case, algo)
                got = s.feed(w, AMPLE)
                seen.add(got["code"])
                if got["code"] == sd.E_UNSUPPORTED:  # refused, not corrupt: the same feed gets the same answer
                    assert s.feed(w, AMPLE)["code"] == sd.E_UNSUPPORTED and s.st["err"] == 0
    prog.close()
    assert seen >= {sd.E_CHECKSUM, sd.E_UNSUPPORTED if cls == sd.OVERSIZED else sd.E_BAD_FRAME}, seen


# ---- the harness sees a broken rule ------------------------------------------------------------------------------------------------
MUTANTS = [
    ("piece-count", "R.off[p.cur + n + 1] <= wend", "R.off[p.cur + n + 1] < wend"),
    ("iv-step", "else c0 = off[i] + kIv;", "else c0 = off[i];"),
    ("lower-bound", "std::upper_bound(pl.q, pl.q + pl.m, x)", "std::lower_bound(pl.q, pl.q + pl.m, x)"),
    ("carry-swapped", "if (i >= n || consumed <= off[i]) return {Carry::kSeed, seed, 0, 0};\n  if (consumed == off[i + 1]) return {Carry::kKnown, sums[i], 0, 0};",
     "if (i >= n || consumed <= off[i]) return {Carry::kSeed, sums[i], 0, 0};\n  if (consumed == off[i + 1]) return {Carry::kKnown, seed, 0, 0};"),
    ("short-partition", "pl.short_part && consumed == pl.PL", "pl.short_part && consumed >= 0"),
]


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_the_harness_sees_a_broken_rule(oracle, ranges, tmp_path, name, old, new):
    text = open(CORE).read()
    assert text.count(old) == 1
    (tmp_path / "decode_stream_core.h").write_text(text.replace(old, new))
    exe = _build(tmp_path, str(tmp_path))
    c, iv_only = ranges[0]
    model = sd.Model(oracle)
    with pytest.raises(AssertionError):
        if name == "short-partition":
            test_a_partition_shorter_than_its_iv(oracle, exe, ranges, tmp_path, 15)
        else:
            prog = Program(exe, tmp_path)
            _sweep_plain(prog, model, c, sd.ADLER, range(1, c.index[-1] + 1))
            _sweep_encrypted(prog, model, EncCase(c, (iv_only,)), sd.CRC, range(1, c.index[-1] + 1))
            prog.close()
