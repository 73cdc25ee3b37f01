"""The damaged ranges of tests/stream_damage.py under IO encryption (s3s_dstream_open_encrypted): each case's range encrypted by
the reference layer (tests/spark_crypto_ref.py through tests/stream_units_encrypted.py), and the contract model's prediction
translated by the IV-unit mapping - the model answers for the PLAIN bytes a stored window shows (IVs dropped, nothing of a
partition whose IV the window's end cuts), and what it consumed is mapped back: 16 more for every IV passed, an IV in front
of the next plain byte included.  Test infrastructure for tests/test_gpu_decode_stream_encrypted_damage.py."""
from __future__ import annotations

import bisect

import numpy as np

import stream_damage as sd
import stream_units as su
import stream_units_encrypted as sue

IV = sue.IV
KEY = sue.KEYS[16]


class EncCase:
    """one case of stream_damage.cases(), stored under the layer"""

    def __init__(self, c: sd.Case):
        self.c = c
        n = len(c.index) - 1
        enc, eidx, _ = sue.encrypt(np.frombuffer(c.img, np.uint8), c.index, KEY, sue.ivs_for(n, 700 + n))
        self.img, self.eidx = enc, [int(x) for x in eidx]
        self.total = self.eidx[-1]
        # the units of the UNDAMAGED image, stored: what bounds the number of feeds
        base = sue.encrypt(np.frombuffer(c.image.img, np.uint8), c.image.index, KEY, sue.ivs_for(len(c.image.index) - 1, 1))[1]
        self.n_units = len(sue.stored_units(c.codec, c.image.img, base))

    def to_stored(self, x: int) -> int:
        return sue.to_stored(self.eidx, x)

    def window(self, pos: int, w: int):
        """the plain side of the stored window [pos, pos + w) -> (plain bytes visible, segments [(plain start, stored start)] of
        the partitions that show plain bytes or a whole IV, whether the window's end cuts an IV)"""
        pidx, eidx, wend = self.c.index, self.eidx, pos + w
        segs, plain, cut = [], 0, False
        for p in range(len(eidx) - 1):
            a, b = eidx[p], eidx[p + 1]
            if b <= pos or b == a:
                continue
            if a >= wend:
                break
            if pos > a:
                c0, p0 = pos, pidx[p] + (pos - a - IV)
            elif a + IV > wend:
                cut = True
                break
            else:
                c0, p0 = a + IV, pidx[p]
            segs.append((p0, c0))
            plain += min(b, wend) - c0
        return plain, segs, cut


def _map_back(segs, pos, x):
    """the stored offset of plain offset x inside the window whose segments are segs"""
    if not segs:
        return pos
    i = bisect.bisect_right([s[0] for s in segs], x) - 1
    return segs[i][1] + (x - segs[i][0])


def feed(model: sd.Model, e: EncCase, st: dict, w: int, cap: int) -> dict:
    """One feed of an encrypted stream in state st = {pos (stored), plain: the model's own state}: the words of
    s3s_dstream_result, `code` and the decoded bytes.  Checksums off."""
    r = dict(code=sd.OK, consumed=0, out_len=0, need_comp=0, need_dst=0, at_end=0, bad=-1, data=b"")
    pst = st["plain"]
    if pst["err"]:
        r["code"] = pst["err"]
        return r
    pos = st["pos"]
    if w == 0:
        r["at_end"] = int(pos == e.total)
        return r
    plain, segs, cut = e.window(pos, w)
    ppos = pst["pos"]
    if plain == 0:  # IVs and nothing else: the whole ones are taken
        consumed_plain, m = 0, dict(code=sd.OK, need_comp=0, out_len=0, data=b"")
    else:
        m = model.feed(e.c, 0, pst, plain, cap)
        assert pst["pos"] - ppos == m["consumed"]
        if m["code"] in (sd.E_BAD_FRAME, sd.E_UNSUPPORTED):
            r["code"] = m["code"]
            return r
        if m["code"] == sd.E_CAPACITY and _map_back(segs, pos, ppos) == pos:
            r["code"], r["need_dst"] = sd.E_CAPACITY, m["need_dst"]
            return r
        consumed_plain = m["consumed"]  # (E_CAPACITY behind a whole IV: the IV is taken - a unit of no output always fits)
    r["consumed"] = _map_back(segs, pos, ppos + consumed_plain) - pos
    if m["code"] == sd.OK:
        r["out_len"], r["data"] = m["out_len"], m["data"]
    if r["consumed"] == 0:
        r["need_comp"] = IV if (cut and not segs) else m["need_comp"]
    st["pos"] = pos + r["consumed"]
    r["at_end"] = int(st["pos"] == e.total)
    return r


def run(e: EncCase, sched: sd.Schedule, feed_fn, max_feeds: int):
    """sd.Model.run in stored coordinates: the first window ends where the schedule's plain offset is stored, the later ones are
    the rest of the range (unit-at-a-time: every window starts at one byte); a window grows to need_comp, dst to need_dst.
    feed_fn(st, pos, window length, capacity) -> one feed's result, advancing st.  -> (trace, bytes handed out)"""
    st = dict(pos=0, plain=dict(pos=0, cur=0, err=0, bad=-1))
    cap = sched.capacity(e.c)
    trace, out = [], []
    win = 1 if sched.unit_at_a_time else max(1, e.to_stored(min(sched.first_end, e.c.index[-1])))
    while True:
        pos = st["pos"]
        w = max(0, min(win, e.total - pos))
        r = feed_fn(st, pos, w, cap)
        trace.append((pos, w, cap, r))
        assert len(trace) <= max_feeds, ("the stream makes no progress", e.c.name, sched)
        if r["code"] == sd.E_CAPACITY:
            assert r["need_dst"] > cap, ("asked for no more than it had", e.c.name, r["need_dst"], cap)
            cap = r["need_dst"]
            if cap > sd.K_MAX:
                break
            continue
        if r["code"] != sd.OK or r["at_end"]:
            break
        out.append(r["data"])
        if r["consumed"] == 0:
            assert r["need_comp"] > w, ("asked for no more than it had", e.c.name, pos, w, r["need_comp"])
            win = r["need_comp"]
        else:
            win = 1 if sched.unit_at_a_time else e.total
    if r["code"] == sd.OK:
        out.append(r["data"])
    return trace, b"".join(out)


SCHEDULES = (("behind-field", "ample"), ("whole", "claim-1"), ("unit-at-a-time", "front"))  # three of the 18: each window rule, each capacity once


def thinned(oracle):
    """every third case of every (codec, class), in the fixed order: every class kept, at least a third of each"""
    seen, out = {}, []
    for c in sd.cases(oracle):
        k = (c.codec, c.cls)
        if seen.get(k, 0) % 3 == 0:
            out.append(c)
        seen[k] = seen.get(k, 0) + 1
    return out
