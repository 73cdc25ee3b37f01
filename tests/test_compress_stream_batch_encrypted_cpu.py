"""CPU: the batched feed of the streaming map side under IO encryption (s3s_cstream_feed_batch* over streams of
s3s_cstream_open_encrypted) as far as it goes without a GPU.

Surface: the read-only key 19 in the header (in parentheses, as key 18) and in the binding with the ABI still 11, a null
context answered before any device work, the section's sentence that key 18 counts plain windows only.
Host arithmetic: csrc/compress_stream_batch_core.h as a stand-alone program under AddressSanitizer and UBSan
(tests/model/cstream_batch_encrypted_model.cpp, run directly) with the kernels played over a pipe: the stand-in of
tests/cstream_batch_lib.py for the codec, the scan, the cut and the checksums, and here the ENCRYPT PASS, played tile by tile
from the tile -> window map, the pass descriptors and the IVs the program laid out, over random rounds of 2 - 9 keyed streams
against tests/cstream_units_encrypted.Model and spark_crypto_ref.encrypt_map_output.  One-token mutants of the new header text
must each fail.
Compiled kernel: aes_ctr_cstream_batch_kernel<10> in the gfx950 interpreter behind the compiled cut and gather
(tests/isa/cstream_batch_encrypted_kernel.py), three windows in one launch, against the reference image and the single kernel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import aes_ctr_model_lib as acm
import cstream_batch_lib as cb
import cstream_units as cu
import cstream_units_encrypted as cue
import spark_crypto_ref as scr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3shuffle_codec.h")
MODEL = os.path.join(ROOT, "tests", "model", "cstream_batch_encrypted_model.cpp")
KEY = bytes((5 * i + 3) & 0xFF for i in range(16))
DST_BIAS = 1 << 44
PASS_TILE = 16384
NOT_RUN = -100


# ---- surface -----------------------------------------------------------------------------------------------------------------
def test_key_19_in_the_header_and_the_binding(codec_lib):
    import s3shuffle
    from s3shuffle import codec

    header = open(HEADER).read()
    assert int(re.search(r"S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES\s*=\s*\((\d+)\)", header).group(1)) == 19 == codec.OPT_CSTREAM_BATCH_ENC_ENTRIES
    assert not re.search(r"S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES\s*=\s*19", header)  # only in parentheses: the pinned set of keys 1..17
    assert int(re.search(r"S3S_OPT_CSTREAM_BATCH_ENTRIES\s*=\s*\((\d+)\)", header).group(1)) == 18
    assert int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1)) == 11 == codec_lib.s3s_abi_version()
    assert isinstance(s3shuffle.Codec.compress_batch_encrypted_entries, property)
    section = header[header.index("the batched feed of s3s_cstream"):header.index("typedef struct s3s_cstream_feed_entry")]
    for needle in ("Key 18 counts plain windows only", "Key 19", "S3S_OPT_CSTREAM_BATCH_ENC_ENTRIES", "ONE encrypt pass", "max(n_ends, 0) + 1",
                   "the IV the\n *          stream carries is used", "kept while the partition stays open, wiped when it closes",
                   "a stream bound to an earlier key setting (S3S_E_INVALID)", "a plain stream\n *          (S3S_E_UNSUPPORTED)",
                   "when the layer is off on the context"):
        assert needle in section, needle
    batched = section[section.index(" * Batched"):section.index(" * One by one")]
    left = section[section.index(" * Left"):]
    assert "ONE encrypt pass" in batched and "ONE encrypt pass" not in left and "S3S_CODEC_NONE" in left and "Zstandard" in left


def test_a_null_context_is_refused_for_get_and_set(codec_lib):
    from s3shuffle import codec

    assert codec_lib.s3s_get_option(None, codec.OPT_CSTREAM_BATCH_ENC_ENTRIES) == -1
    assert codec_lib.s3s_set_option(None, codec.OPT_CSTREAM_BATCH_ENC_ENTRIES, 1) == -1


# ---- the stand-in: a keyed map output, and the kernels with the encrypt pass ---------------------------------------------------
class KeyedCase(cb.StreamCase):
    """cb.StreamCase under a key: img / index / sizes / model are the STORED image's, the plain ones are kept next to them"""

    def __init__(self, oracle, codec, bs, data, offs, ivs, stale=False):
        super().__init__(oracle, codec, bs, data, offs)
        self.plain_img, self.plain_index, self.plain_sizes = self.img, self.index, self.sizes
        self.ivs, self.stale = ivs, stale
        enc, eidx, _ = scr.encrypt_map_output(np.frombuffer(self.plain_img, np.uint8), np.asarray(self.plain_index, np.int64), KEY, ivs.reshape(-1))
        self.img, self.index = np.asarray(enc).tobytes(), [int(x) for x in eidx]
        assert self.index == cue.stored_index(self.plain_index)
        self.sizes = cue.encrypted_unit_sizes(self.plain_sizes)
        self.model = cue.Model(codec, bs, self.sizes)

    def item_size(self, stream_off, length):  # a block item's bytes: without the IV record in front of it
        keyed, self.sizes = self.sizes, self.plain_sizes
        try:
            return super().item_size(stream_off, length)
        finally:
            self.sizes = keyed

    def feed_ivs(self, n_ends, other_iv0):
        a = np.zeros((max(n_ends, 0) + 1, 16), np.uint8)
        for j in range(a.shape[0]):
            if self.model.n_closed + j < len(self.ivs):
                a[j] = self.ivs[self.model.n_closed + j]
        if other_iv0 and self.model.open_img > 0:
            a[0] = 0xEE  # ignored: the stream carries the open partition's
        return a

    def holed(self, true_piece):
        """what the cut gather leaves in dst: the plain image bytes of the window's pieces (stored offsets true_piece), a
        16-byte hole in front of every partition that starts in the output"""
        out, mo = [], self.model
        for j in range(len(true_piece) - 1):
            n = true_piece[j + 1] - true_piece[j]
            if n == 0:
                continue
            part = mo.n_closed + j
            plain = self.plain_img[self.plain_index[part]:self.plain_index[part + 1]]
            if j == 0 and mo.open_img > 0:
                out.append(plain[mo.open_img - 16:mo.open_img - 16 + n])
            else:
                out.append(b"\xa5" * 16 + plain[:n - 16])
        return np.frombuffer(b"".join(out), np.uint8)


class KeyedProgram(cb.Program):
    def __init__(self, exe, tmp_path, codec, bs, algo, streams):
        super().__init__(exe, tmp_path, codec, bs, algo, len(streams))
        self.p.stdin.write(" ".join("0" if s.stale else "1" for s in streams) + "\n")
        self.residues = set()  # front mod 16 of the windows the pass ran over with a carried IV

    def round(self, entries, streams, other_iv0=False, iv_delta=0):
        """cb.Program.round under a key.  iv_delta: IVs more (or fewer) than the slices need.
        -> (answers, windows) or ("V", answers) when the program refused the IV count"""
        ivs = [streams[s].feed_ivs(-1 if ends is None else len(ends), other_iv0) for s, _, _, _, ends in entries]
        flat = np.concatenate(ivs).reshape(-1, 16)
        if iv_delta > 0:
            flat = np.concatenate([flat, np.zeros((iv_delta, 16), np.uint8)])
        elif iv_delta < 0:
            flat = flat[:iv_delta]
        text = "R %d %d\n%s\n" % (len(entries), flat.shape[0], flat.tobytes().hex() or "-")
        for s, addr, src_len, cap, ends in entries:
            text += "%d %d %d %d %d %s\n" % (s, addr, src_len, cap, -1 if ends is None else len(ends), " ".join(map(str, ends or [])))
        try:
            self.p.stdin.write(text)
            self.p.stdin.flush()
        except BrokenPipeError:
            self._line()
        t = self._line()
        windows = 0
        if t[0] == "V":
            windows = "V"
            t = self._line()
        elif t[0] == "P":
            m, N, PP, P, L = (int(x) for x in t[1:])
            windows = m
            wins = [self._ints("W") for _ in range(m)]
            items, marks, pf, seeds, pw = self._ints("I"), self._ints("M"), self._ints("F"), self._ints("S"), self._ints("E")
            if not (len(items) == 4 * N and len(marks) == 3 * N and len(pf) == PP and len(seeds) == P and len(pw) == P):
                raise cb.Dead("the plan's arrays do not have the sizes it states")
            tiles = self._ints("T")[0]
            descs = [self._ints("D") for _ in range(m)]
            tile_win = self._ints("Q")
            h = self._line()
            call_ivs = np.frombuffer(bytes.fromhex(h[1]) if len(h) > 1 else b"", np.uint8)
            if h[0] != "H" or call_ivs.size != 16 * P or len(tile_win) != tiles:
                raise cb.Dead("the IVs or the tile map do not have the sizes the plan states")
            down = self._kernels(entries, streams, wins, items, marks, pf, seeds, pw, N, PP, P, L)
            self._pass(entries, streams, wins, descs, tile_win, call_ivs, down[m:9 * m], down[9 * m:9 * m + PP], PP, P)
            try:
                self.p.stdin.write(" ".join(str(int(x)) for x in down) + "\n")
                self.p.stdin.flush()
            except BrokenPipeError:
                self._line()
            t = self._line()
            if t[0] == "X":
                raise cb.Dead("the program found the stand-in's words impossible")
        out = []
        for i in range(len(entries)):
            if i:
                t = self._line()
            if t[0] != "A":
                raise cb.Dead("expected A, got %s" % t[:4])
            v = [int(x) for x in t[1:-1]]
            n = v[6]
            d = dict(zip(("code", "consumed", "out_len", "need_src", "need_dst", "parts_closed"), v[:6]))
            d["lengths"] = v[7:7 + n]
            rest = v[7 + n:]
            d["sums"] = rest[:n] if self.algo else []
            d["pos"], d["written"], d["open_bytes"], d["open_img"], d["carry"] = rest[-5:]
            d["iv"] = bytes.fromhex(t[-1])
            out.append(d)
        return out, windows

    def _pass(self, entries, streams, wins, descs, tile_win, call_ivs, res, piece, PP, P):
        """aes_ctr_cstream_batch_kernel, from what the program laid out: every tile of the launch finds its window through the
        map, reads that window's descriptor and encrypts its tile of that window's output in place.  What the launch leaves in
        every destination must be the stored image of the stream"""
        m = len(wins)
        dst, own = {}, []
        for wi, w in enumerate(wins):
            e, first_pp, n_pieces = w[0], w[3], w[4]
            sc = streams[entries[e][0]]
            true_piece = piece[first_pp:first_pp + n_pieces + 1]
            dst[entries[e][1] + DST_BIAS] = sc.holed(true_piece).copy()
            own.append(entries[e][1] + DST_BIAS)
        covered = {a: np.zeros(d.size, bool) for a, d in dst.items()}
        enc = {}
        for t, w in enumerate(tile_win):
            if not 0 <= w < m:
                raise cb.Dead("tile %d belongs to window %d" % (t, w))
            e_off, iv_off, cut_off, n, tile0, front, out = descs[w]
            if out not in dst or cut_off % 8 or not (0 <= cut_off < 8 * m and 0 <= e_off and e_off + n + 1 <= PP and 0 <= iv_off and iv_off + n <= P):
                raise cb.Dead("descriptor %d points outside the call's arrays" % w)
            L = res[cut_off + 2]
            ti = t - tile0
            if ti < 0:
                raise cb.Dead("tile %d lies in front of its window's first tile" % t)
            lo, hi = max(PASS_TILE * ti - (front & 15), 0), min(PASS_TILE * (ti + 1) - (front & 15), L)
            if L <= 0 or lo >= hi:
                continue
            if hi > dst[out].size:
                raise cb.Dead("tile %d writes beyond out_len of its destination" % t)
            if w not in enc:  # the window's whole output as THIS descriptor encrypts it
                E, parts = piece[e_off:e_off + n + 1], []
                for j in range(n):
                    a, b = E[j], E[j + 1]
                    if b <= a:
                        continue
                    iv = call_ivs[16 * (iv_off + j):16 * (iv_off + j) + 16].tobytes()
                    if j == 0 and front > 0:
                        parts.append(acm.xor_stream(KEY, iv, dst[out][a:b], offset=front - 16))
                    else:
                        parts.append(np.concatenate([np.frombuffer(iv, np.uint8), acm.xor_stream(KEY, iv, dst[out][a + 16:b], offset=0)]))
                enc[w] = np.concatenate(parts + [np.zeros(0, np.uint8)])
                if enc[w].size != L:
                    raise cb.Dead("descriptor %d: the pieces end at %d, out_len is %d" % (w, enc[w].size, L))
            covered[out][lo:hi] = True
        for wi, w in enumerate(wins):
            sc = streams[entries[w[0]][0]]
            out_len = res[8 * wi + 2]
            holed = dst[own[wi]]
            played = np.where(covered[own[wi]], enc.get(wi, holed)[:holed.size] if wi in enc else holed, holed)
            want = np.frombuffer(sc.img[sc.model.written:sc.model.written + out_len], np.uint8)
            if holed.size != out_len or not np.array_equal(played, want):
                raise cb.Dead("window %d: the pass leaves other bytes than the stored image (front %d)" % (wi, w[10]))
            if w[10] > 0 and out_len > 0:
                self.residues.add(w[10] % 16)


def build(out_dir, include_dir=cb.CSRC):
    exe = os.path.join(str(out_dir), "cstream_batch_encrypted_model")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", include_dir, MODEL, "-o", exe], check=True)
    return exe


def run_rounds(oracle, exe, tmp_path, codec, bs, algo, seed, n_streams, max_rounds=300):
    """cb.run_rounds under a key: random rounds of one window of each of n_streams keyed streams (one of them bound to an
    earlier key setting in every other run) until every stream has closed its map output; a round in seven is first sent with
    a wrong IV count.  -> dict(rounds, batched, refused, hosted, stale, wrong_ivs, residues)"""
    rng = np.random.default_rng(seed)
    streams = []
    for i in range(n_streams):
        data, offs = cb.map_output(rng, bs, int(rng.integers(2, 6)))
        ivs = rng.integers(0, 256, (len(offs) - 1, 16), dtype=np.uint8)
        streams.append(KeyedCase(oracle, codec, bs, data, offs, ivs, stale=(seed % 2 == 1 and i == 1)))
    prog = KeyedProgram(exe, tmp_path, codec, bs, algo, streams)
    try:
        return _rounds(prog, streams, rng, codec, bs, algo, seed, max_rounds)
    except BaseException:
        prog.kill()
        raise


def _state(s, algo, g):
    mo = s.model
    open_at = s.index[mo.n_closed] if mo.n_closed < len(s.index) - 1 else s.index[-1]
    carry = cb.checksum(algo, s.img[open_at:open_at + mo.open_img], cb.fresh(algo)) if algo else g["carry"]
    iv = s.ivs[mo.n_closed].tobytes() if mo.open_img > 0 else bytes(16)  # kept while the partition is open, wiped when it closes
    return (mo.pos, mo.written, mo.open_bytes, mo.open_img, carry, iv)


def _rounds(prog, streams, rng, codec, bs, algo, seed, max_rounds):
    n_streams = len(streams)
    big = max(max((x for p in s.sizes for x in p), default=1) for s in streams)
    tally = dict(rounds=0, batched=0, refused=0, hosted=0, stale=0, wrong_ivs=0)
    live = lambda s: not s.done and not s.stale  # noqa: E731
    while any(live(s) for s in streams) and tally["rounds"] < max_rounds:
        tally["rounds"] += 1
        slots = rng.permutation(n_streams)  # where the windows lie: later entries may lie below the first
        entries, bad = [], []
        for i, s in enumerate(streams):
            total, mo = s.offs[-1], s.model
            wlen = min(int(rng.choice([0, 1, bs - 1, bs, bs + 1, 3 * bs - 1, int(rng.integers(0, 4 * bs)), total])), total - mo.pos)
            ends = cu.ends_in_window(s.offs, mo.pos, mo.n_closed, wlen)
            cap = int(rng.choice([0, 20, 36, 37, big - 1, big, big + 1, 2 * big + 5, int(rng.integers(0, 5 * big)), 1 << 40]))
            kind = int(rng.integers(0, 12))
            if kind == 0 and len(ends) >= 2 and ends[0] != ends[-1]:
                ends = ends[::-1]  # descending: that entry's own S3S_E_INVALID
                bad.append(i)
            elif kind == 1:
                cap = -1
                bad.append(i)
            elif kind == 2 and ends:
                ends = ends[:-1] + [wlen + 1]  # beyond the window
                bad.append(i)
            elif kind == 3:
                ends = None  # n_ends = -1: refused, and under IO encryption still one IV of the call's
                bad.append(i)
            elif kind == 4 and ends and ends[-1] == wlen:
                ends = ends[:-1]  # an end at the window's very end held back: a later window passes it, maybe one that launches nothing
            entries.append((i, 1 << 20 | int(slots[i]) << 24, wlen, cap, ends))
        other_iv0 = bool(tally["rounds"] % 2)
        if tally["rounds"] % 7 == 3:  # a wrong IV count: refused before anything runs, with every stream unchanged
            got, verdict = prog.round(entries, streams, other_iv0, iv_delta=[1, -1][tally["rounds"] % 2])
            assert verdict == "V", verdict
            tally["wrong_ivs"] += 1
            for (i, *_), g in zip(entries, got):
                assert g["code"] == NOT_RUN and (g["pos"], g["written"], g["open_bytes"], g["open_img"], g["carry"], g["iv"]) == _state(streams[i], algo, g)
        got, windows = prog.round(entries, streams, other_iv0)
        assert windows != "V", "the program refused the right IV count"
        tally["batched"] += windows
        tally["hosted"] += len(entries) - len(bad) - windows - sum(streams[i].stale and i not in bad for i, *_ in entries)
        for (i, _, wlen, cap, ends), g in zip(entries, got):
            s = streams[i]
            if i in bad or s.stale:
                tally["refused" if i in bad else "stale"] += 1
                want = cu.Feed(code=-1)
            else:
                before = s.model.n_closed
                want = s.model.feed(wlen, ends, cap)
                want.sums = [cb.checksum(algo, s.img[s.index[p]:s.index[p + 1]], cb.fresh(algo)) for p in range(before, before + want.parts_closed)]
            assert (g["code"], g["consumed"], g["out_len"], g["need_src"], g["need_dst"], g["parts_closed"], tuple(g["lengths"])) == want.fields(), \
                (codec, seed, tally["rounds"], i, entries[i], g, want.fields())
            assert (g["pos"], g["written"], g["open_bytes"], g["open_img"], g["carry"], g["iv"]) == _state(s, algo, g), (codec, seed, tally["rounds"], i, g)
            if algo and i not in bad and not s.stale:
                assert g["sums"] == want.sums, (codec, seed, tally["rounds"], i, g["sums"], want.sums)
    prog.close()
    assert not any(live(s) for s in streams), "the schedule did not end"
    tally["residues"] = prog.residues
    return tally


# ---- host arithmetic against the Python model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("cstream_batch_enc"))


CASES = [(cu.LZ4, 64, cb.ADLER, 6), (cu.LZ4, 64, 0, 3), (cu.SNAPPY, 1024, cb.CRC, 6), (cu.LZF, 65535, cb.ADLER, 2)]


@pytest.mark.parametrize("codec,bs,algo,runs", CASES, ids=["lz4-adler", "lz4-nosum", "snappy-crc", "lzf-adler"])
def test_host_arithmetic_against_the_python_model(oracle, model_exe, tmp_path, codec, bs, algo, runs):
    total = dict(batched=0, refused=0, hosted=0, stale=0, wrong_ivs=0)
    residues = set()
    for run in range(runs):
        n_streams = int(np.random.default_rng(run).integers(2, 4)) if codec == cu.LZF else [2, 9, 5, 3, 7, 4][run % 6]
        t = run_rounds(oracle, model_exe, tmp_path, codec, bs, algo, seed=1000 * codec + run, n_streams=n_streams)
        for k in total:
            total[k] += t[k]
        residues |= t["residues"]
    # healthy windows, refused entries, entries that launch nothing, a stale stream and wrong IV counts next to each other
    assert total["batched"] >= 5 * runs and total["refused"] > 0 and total["hosted"] > 0 and total["stale"] > 0 and total["wrong_ivs"] > 0, total
    assert residues, "no window continued an open partition"
    if codec == cu.LZ4 and algo:  # ... and the carried IV at EVERY residue of front mod 16, sixteen streams in one call
        assert residues | _residue_rounds(oracle, model_exe, tmp_path) == set(range(16))


MUTANTS = [
    ("if (c.open_img > 0)\n    for (size_t i = 0; i < kIvBytes; i++) mine[i] = carried[i];",
     "if (c.open_img < 0)\n    for (size_t i = 0; i < kIvBytes; i++) mine[i] = carried[i];"),                      # the carried IV does not replace entry 0
    ("const int64_t mine = at;", "const int64_t mine = at + 1;"),                                                 # the IV slice offset of entry i
    ("for (int64_t t = 0; t < tiles; t++) tile_win[tile0 + t] = w;", "for (int64_t t = 0; t < tiles; t++) tile_win[tile0 + t] = w + 1;"),  # the map, off by one
    ("p.front = cuts[w].open_img;", "p.front = cuts[0].open_img;"),                                               # front of another entry
    ("if (st.open_img == 0) {\n    wipe_iv(iv);", "if (st.open_img < 0) {\n    wipe_iv(iv);"),                    # the IV not wiped on close
    ("return (len + (front & 15) + kPassTile - 1) / kPassTile;", "return (len + (front & 0) + kPassTile - 1) / kPassTile;"),  # the grid without the lead
    ("p.ivs = ivs + kIvBytes * (size_t)cuts[w].first_piece;", "p.ivs = ivs + kIvBytes * (size_t)cuts[w].first_pp;"),  # the IVs of an n + 1 array
    ("} else if (parts_closed > 0 || front == 0) {", "} else if (parts_closed > 0 && front == 0) {"),             # the next open partition's IV kept
    ("if (lead) emit_iv(u, c->first_item + it);", "if (lead) emit_iv(u, it);"),                                   # the IV record of the call, not of the entry
    # the rules both feeds share: the take step's IV bookkeeping, the slice of a refused entry, the empty window's IV
    ("if (iv) commit_iv(iv, *st, before.open_img,", "if (iv) commit_iv(iv, before, before.open_img,"),            # the state from before the commit
    ("return (int64_t)(n_ends > 0 ? n_ends : 0) + 1;", "return (int64_t)(n_ends > -2 ? n_ends : 0) + 1;"),        # an entry with n_ends < 0 has one IV too
    ("if (iv) commit_nothing_iv(iv, c.parts_closed);", "if (iv) commit_nothing_iv(iv, 0);"),
]


def _mutant_rounds(oracle, exe, tmp_path, old):
    if "kPassTile - 1) / kPassTile" in old:
        _tile_lead_round(oracle, exe, tmp_path)
    if "commit_nothing_iv" in old:
        _held_back_end_round(oracle, exe, tmp_path)
    for run in range(4):
        run_rounds(oracle, exe, tmp_path, cu.LZ4, 64, cb.ADLER, seed=1000 * cu.LZ4 + run, n_streams=[2, 9, 5, 3][run])


def _residue_rounds(oracle, exe, tmp_path):
    """forty candidate streams whose first block of 64 bytes starts with k random bytes and ends in zeros: sixteen of them, one
    per residue of open_img mod 16 behind that block, take it in round one and the rest of their map output in round two,
    where entry 0 of every slice is another IV.  -> the residues the pass ran over"""
    rng = np.random.default_rng(3)
    cases = []
    for k in range(40):
        data = np.zeros(264, np.uint8)
        data[:k] = rng.integers(1, 256, k, dtype=np.uint8)
        data[64:] = rng.integers(0, 256, 200, dtype=np.uint8)
        cases.append(KeyedCase(oracle, cu.LZ4, 64, data, np.array([0, 230, 264], np.int64), rng.integers(0, 256, (2, 16), dtype=np.uint8)))
    by_residue = {}
    for c in cases:
        by_residue.setdefault(c.sizes[0][0] % 16, c)
    assert sorted(by_residue) == list(range(16))
    streams = [by_residue[r] for r in range(16)]
    prog = KeyedProgram(exe, tmp_path, cu.LZ4, 64, cb.ADLER, streams)
    try:
        for wlen in (64, 200):
            entries = [(i, 1 << 20 | i << 24, wlen, 1 << 30, cu.ends_in_window(s.offs, s.model.pos, s.model.n_closed, wlen)) for i, s in enumerate(streams)]
            got, windows = prog.round(entries, streams, other_iv0=True)
            assert windows == 16
            for (i, _, w, cap, ends), g in zip(entries, got):
                want = streams[i].model.feed(w, ends, cap)
                assert (g["code"], g["consumed"], g["out_len"], g["parts_closed"], tuple(g["lengths"])) == (0, want.consumed, want.out_len, want.parts_closed, tuple(want.lengths))
                assert (g["pos"], g["written"], g["open_bytes"], g["open_img"], g["carry"], g["iv"]) == _state(streams[i], cb.ADLER, g)
        prog.close()
    except BaseException:
        prog.kill()
        raise
    assert all(s.done for s in streams)
    return prog.residues


def _tile_lead_round(oracle, exe, tmp_path):
    """two streams whose second windows continue a partition at front = 16 + 21 + 64 = 101 (residue 5) and write 16380 and
    16379 stored bytes into destinations of exactly that size: the first one's last byte lies in the second tile of the pass,
    which starts 5 bytes in front of the output's 16 KiB"""
    rng = np.random.default_rng(1)
    streams = []
    for r in (18, 17):  # 64 + 192 blocks of 64 incompressible bytes and a tail: 192 x 85 + 21 + r + 21 for the end frame
        n = 64 + 192 * 64 + r
        streams.append(KeyedCase(oracle, cu.LZ4, 64, rng.integers(0, 256, n, dtype=np.uint8), np.array([0, n], np.int64),
                                 rng.integers(0, 256, (1, 16), dtype=np.uint8)))
    prog = KeyedProgram(exe, tmp_path, cu.LZ4, 64, cb.ADLER, streams)
    try:
        for wlen, caps in ((64, (1 << 30, 1 << 30)), (1 << 20, (16380, 16379))):
            entries = [(i, 1 << 20 | i << 24, min(wlen, s.offs[-1] - s.model.pos), caps[i],
                        cu.ends_in_window(s.offs, s.model.pos, 0, min(wlen, s.offs[-1] - s.model.pos))) for i, s in enumerate(streams)]
            got, _ = prog.round(entries, streams)
            for (i, _, w, cap, ends), g in zip(entries, got):
                want = streams[i].model.feed(w, ends, cap)
                assert (g["code"], g["out_len"], g["parts_closed"]) == (0, want.out_len, want.parts_closed)
        assert [g["out_len"] for g in got] == [16380, 16379]
        prog.close()
    except BaseException:
        prog.kill()
        raise


def _held_back_end_round(oracle, exe, tmp_path):
    """two Snappy streams whose first partition is one whole block: round one takes the block and holds the end back, round
    two is an empty window with that end - it launches nothing, closes a partition that has image bytes and wipes its IV -
    round three takes the rest.  (An LZ4 partition with bytes closes with its end frame: a window with a unit.)"""
    rng = np.random.default_rng(5)
    streams = [KeyedCase(oracle, cu.SNAPPY, 1024, rng.integers(0, 256, 1024 + r, dtype=np.uint8), np.array([0, 1024, 1024 + r], np.int64),
                         rng.integers(1, 256, (2, 16), dtype=np.uint8)) for r in (5, 1024)]
    prog = KeyedProgram(exe, tmp_path, cu.SNAPPY, 1024, cb.CRC, streams)
    try:
        for wlen, ends, windows in ((1024, [], 2), (0, [0], 0), (1 << 20, None, 2)):
            entries = []
            for i, s in enumerate(streams):
                w = min(wlen, s.offs[-1] - s.model.pos)
                entries.append((i, 1 << 20 | i << 24, w, 1 << 30, cu.ends_in_window(s.offs, s.model.pos, s.model.n_closed, w) if ends is None else ends))
            got, m = prog.round(entries, streams)
            assert m == windows
            for (i, _, w, cap, e), g in zip(entries, got):
                want = streams[i].model.feed(w, e, cap)
                assert (g["code"], g["consumed"], g["out_len"], g["need_src"], g["need_dst"], g["parts_closed"], tuple(g["lengths"])) == want.fields()
                assert (g["pos"], g["written"], g["open_bytes"], g["open_img"], g["carry"], g["iv"]) == _state(streams[i], cb.CRC, g)
        prog.close()
    except BaseException:
        prog.kill()
        raise
    assert all(s.done for s in streams)


def test_the_unmutated_header_passes_the_mutants_rounds(oracle, model_exe, tmp_path):
    _tile_lead_round(oracle, model_exe, tmp_path)
    _held_back_end_round(oracle, model_exe, tmp_path)


@pytest.mark.parametrize("old,new", MUTANTS, ids=[str(i) for i in range(len(MUTANTS))])
def test_one_token_mutants_of_the_new_header_text_fail(oracle, tmp_path, old, new):
    text = open(cb.CORE).read()
    assert text.count(old) == 1, old
    inc = tmp_path / "inc"
    inc.mkdir()
    (inc / "compress_stream_batch_core.h").write_text(text.replace(old, new))
    (inc / "compress_stream_core.h").write_text(open(os.path.join(cb.CSRC, "compress_stream_core.h")).read())
    exe = build(tmp_path, include_dir=str(inc))
    with pytest.raises(AssertionError):
        _mutant_rounds(oracle, exe, tmp_path, old)


# ---- the compiled encrypt pass of the batch through the gfx950 interpreter ---------------------------------------------------
def _reference(oracle, parts, tail, open_img, ivs):
    """the stored bytes of a window's whole output and its stored piece offsets: every piece but a continued piece 0 starts
    its partition with an IV; a continued piece goes on in its key stream at open_img - 16"""
    pieces = list(parts) + ([tail] if tail else [])
    data = np.frombuffer(b"".join(pieces), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.int64)
    img, index, _ = oracle.compress_map_output(cu.LZ4, 0, data, offs, block_size=64)
    img, index = np.asarray(img), [int(x) for x in index]
    if tail:  # the open piece has no end frame yet
        img, index[-1] = img[:index[-1] - cu.LZ4_END], index[-1] - cu.LZ4_END
    out, stored = [], [0]
    for j in range(len(pieces)):
        plain = img[index[j]:index[j + 1]]
        iv = ivs[j].tobytes()
        if plain.size == 0:
            pass
        elif j == 0 and open_img > 0:
            out.append(acm.xor_stream(KEY, iv, plain, offset=open_img - 16))
        else:
            out += [np.frombuffer(iv, np.uint8), acm.xor_stream(KEY, iv, plain, offset=0)]
        stored.append(sum(x.size for x in out))
    return np.concatenate(out).tobytes(), stored


def test_the_compiled_batch_pass_behind_the_cut_in_the_interpreter(oracle):
    """Three windows in one launch at block size 64, every destination of exactly dst_capacity bytes.  Window 0 (one block of a
    fresh open partition) answers need_dst: it owns a tile, which returns whole, and its destination keeps the prefill.
    Window 1 continues an open partition at front = 16 + 9 and is cut inside its second partition.  Window 2 takes
    everything: incompressible partitions of 192 blocks + 1 byte and of 100 bytes, the second of which starts at stored
    offset 16379, within the last 16 bytes of the first 16 KiB tile."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "isa"))
    import cstream_batch_encrypted_kernel as bek

    rng = np.random.default_rng(21)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    text = lambda n: bytes(np.resize(np.frombuffer(b"abcdabcdabcdabce0123", np.uint8), n))  # noqa: E731
    nr, rk = acm.expand_key(KEY)
    assert nr == 10
    wins = [dict(parts=[], tail=text(64), open_img=0), dict(parts=[text(100) + rnd(28), rnd(150) + text(106)], tail=b"", open_img=25),
            dict(parts=[rnd(192 * 64 + 1), rnd(100)], tail=b"", open_img=0)]
    for w in wins:
        w["ivs"] = rng.integers(0, 256, (len(w["parts"]) + 1, 16), dtype=np.uint8)
        w["want"], w["stored"] = _reference(oracle, w["parts"], w["tail"], w["open_img"], w["ivs"])
    assert wins[2]["stored"][1] == 16379 and len(wins[2]["want"]) > PASS_TILE
    cut1 = wins[1]["stored"][1] + 16 + 21 + 64 + 30  # the second partition's IV and first block fit, its second block does not
    caps = [len(wins[0]["want"]) - 1, cut1, len(wins[2]["want"])]
    for w, cap in zip(wins, caps):
        w["cap"] = cap
    got = bek.feed_batch_lz4_encrypted(wins, 64, rk, extra_tiles=1)
    assert [g["tiles"] for g in got] == [1, 1, 2] and [g["tile0"] for g in got] == [0, 1, 2]
    g = got[0]
    assert (g["k"], g["out_len"], g["need_dst"], g["parts_closed"]) == (0, 0, len(wins[0]["want"]), 0)
    assert g["dst"] == b"\xa5" * caps[0] and not g["pass_writes"].any()
    for i in (1, 2):
        g, w = got[i], wins[i]
        n = g["out_len"]
        assert g["status"] == 0 and g["need_dst"] == 0 and 0 < n <= caps[i]
        assert g["piece_off"] == [min(x, n) for x in w["stored"]] + ([n] if not w["tail"] else [])
        assert g["dst"] == w["want"][:n] + b"\xa5" * (caps[i] - n), i      # the reference image up to the cut, the prefill behind it
        assert g["dst"] == g["single"], i                                   # byte for byte the single kernel on the same plan
        assert (g["pass_writes"][:n] == 1).all() and not g["pass_writes"][n:].any(), i  # every stored byte once, nothing at or beyond out_len
    assert got[1]["parts_closed"] == 1 and got[1]["out_len"] == wins[1]["stored"][1] + 16 + 21 + 64 < caps[1]
    assert got[2]["parts_closed"] == 2 and got[2]["out_len"] == caps[2]
