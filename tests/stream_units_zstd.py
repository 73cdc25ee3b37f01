"""The contract of a resumable Zstandard stream (s3s_dstream_open_zstd, include/s3shuffle_codec.h) as a Python model: TEST
INFRASTRUCTURE.  Written from RFC 8878 with a header walk of its own - it does not call the library - and checked against the
host build of the library's walk (tests/test_zstd_stream_units_cpu.py) before the GPU tests lean on it.

Units: a frame header (6 .. 18 bytes), a block (3 + Block_Size bytes, an RLE block 3 + 1), a skippable frame (8 + n bytes).
"""
import ctypes

import numpy as np

OK, E_CAPACITY, E_BAD_FRAME, E_UNSUPPORTED = 0, -2, -3, -6
FRAME, SKIP, RAW, RLE, COMP, LAST = 0, 1, 2, 3, 4, 0x10
MAX_BLOCK = 128 << 10
SKIP_MAX = 32 << 20


class Bad(Exception):
    pass


class Refused(Exception):
    pass


def header_length(descriptor):
    fcs_flag, single, did_flag = descriptor >> 6, (descriptor >> 5) & 1, descriptor & 3
    return 5 + (0 if single else 1) + (0, 1, 2, 4)[did_flag] + ((1 if single else 0), 2, 4, 8)[fcs_flag]


def window_size(hdr):
    """Window_Size of the frame header bytes `hdr` (whole header): a single-segment frame's is its content size."""
    d = hdr[4]
    fcs_flag, single, did_flag = d >> 6, (d >> 5) & 1, d & 3
    ip = 5
    if not single:
        wd = hdr[ip]
        ip += 1
        base = 1 << (10 + (wd >> 3))
        return base + (base >> 3) * (wd & 7)
    ip += (0, 1, 2, 4)[did_flag]
    nb = (1, 2, 4, 8)[fcs_flag]
    v = int.from_bytes(hdr[ip:ip + nb], "little")
    return v + 256 if nb == 2 else v


def walk(win, pend, open_, wlog):
    """The whole units of one piece of a partition: `win` is what the window shows of it, the partition ends pend >= len(win)
    bytes from the piece's start, `open_` says whether a frame is open there.  -> (units, stop, need, open at stop); units are
    (offset, kind, payload, unit length).  Raises Bad / Refused."""
    end, ip, out, need = len(win), 0, [], 0

    class Stop(Exception):
        pass

    def want(x):
        nonlocal need
        if x > pend - ip:
            raise Bad("a unit runs past the partition's end")
        if x > end - ip:
            need = x
            raise Stop()

    try:
        while ip < end:
            if not open_:
                want(6)
                magic = int.from_bytes(win[ip:ip + 4], "little")
                if magic & 0xFFFFFFF0 == 0x184D2A50:
                    want(8)
                    n = 8 + int.from_bytes(win[ip + 4:ip + 8], "little")
                    if n > SKIP_MAX:
                        raise Refused("skippable frame above 32 MiB")
                    want(n)
                    out.append((ip, SKIP, n, n))
                    ip += n
                    continue
                if magic != 0xFD2FB528:
                    raise Bad("magic")
                d = win[ip + 4]
                if d & 0x08:
                    raise Bad("reserved bit")
                hl = header_length(d)
                want(hl)
                if d & 0x04:
                    raise Refused("Content_Checksum")
                if d & 3:
                    raise Refused("Dictionary_ID")
                if window_size(win[ip:ip + hl]) > 1 << wlog:
                    raise Refused("Window_Size")
                out.append((ip, FRAME, hl, hl))
                ip += hl
                open_ = True
            else:
                want(3)
                bh = int.from_bytes(win[ip:ip + 3], "little")
                last, typ, size = bh & 1, (bh >> 1) & 3, bh >> 3
                if typ == 3 or size > MAX_BLOCK or (typ == 2 and size < 2):
                    raise Bad("block header")
                n = 3 + (1 if typ == 1 else size)
                want(n)
                out.append((ip, (RAW + typ) | (LAST if last else 0), size, n))
                ip += n
                if last:
                    open_ = False
    except Stop:
        pass
    if ip == pend and open_:
        raise Bad("the partition ends with a frame open")
    return out, ip, need, open_


def partition_units(part, wlog=27):
    """All units of a whole partition."""
    u, stop, need, open_ = walk(bytes(part), len(part), False, wlog)
    assert stop == len(part) and not open_
    return u


def boundaries(img, offsets, wlog=27):
    """Every unit boundary of a range, range-relative and ascending (partition ends included)."""
    out = {0}
    for p in range(len(offsets) - 1):
        a, b = int(offsets[p]), int(offsets[p + 1])
        out.add(b)
        for off, _, _, n in partition_units(bytes(img[a:b]), wlog):
            out.add(a + off + n)
    return sorted(out)


def decoded_sizes(part):
    """{unit offset: decoded bytes} of the blocks of a whole valid partition: libzstd's streaming decoder hands out every
    whole block it has seen, so the output position behind each unit boundary is the running sum."""
    from oracle import zstd_ref

    z = zstd_ref.lib()
    part = np.ascontiguousarray(np.frombuffer(bytes(part), np.uint8))
    units = partition_units(part.tobytes())
    cap = 1 << 20
    out = np.empty(cap, np.uint8)
    dctx = z.ZSTD_createDCtx()
    sizes, done = {}, 0
    try:
        for off, kind, _, n in units:
            ib = zstd_ref._Buf(part.ctypes.data, off + n, done)
            got = 0
            while True:
                ob = zstd_ref._Buf(out.ctypes.data, cap, 0)
                r = z.ZSTD_decompressStream(dctx, ctypes.byref(ob), ctypes.byref(ib))
                assert not z.ZSTD_isError(r)
                got += ob.pos
                if ib.pos == ib.size and ob.pos < cap:
                    break
            done = off + n
            sizes[off] = got
    finally:
        z.ZSTD_freeDCtx(dctx)
    return sizes


class StreamModel:
    """Position and open-frame flag of a stream over a range; `feed` says what a window of `length` bytes must give:
    (code, consumed, out_len or None, need_comp, need_dst).  sizes: {range-relative unit offset: decoded bytes} - needed only
    for a capacity cut and for out_len."""

    def __init__(self, img, offsets, wlog, sizes=None):
        self.img, self.off, self.wlog, self.sizes = bytes(img), [int(x) for x in offsets], wlog, sizes
        self.pos, self.cur, self.open = 0, 0, False

    def feed(self, length, cap=None):
        np_, wend = len(self.off) - 1, self.pos + length
        units, consumed, need, open_ = [], 0, 0, self.open
        p, bad, refused = self.cur, False, False
        while p < np_ and (self.off[p] < wend or self.off[p + 1] <= wend):
            a, b = max(self.off[p], self.pos), self.off[p + 1]
            e = min(b, wend)
            try:  # (every piece of the window is walked: corruption in any of them wins over a refusal in another)
                u, stop, need, op = walk(self.img[a:e], b - a, self.open if p == self.cur else False, self.wlog)
                units += [(a + o, k, pl, n) for o, k, pl, n in u]
                consumed, open_ = a + stop - self.pos, op
            except Bad:
                bad = True
            except Refused:
                refused = True
            p += 1
        if bad:
            return E_BAD_FRAME, 0, 0, 0, 0
        if refused:
            return E_UNSUPPORTED, 0, 0, 0, 0
        out = None
        if self.sizes is not None:
            out = 0
            for i, (o, k, pl, n) in enumerate(units):
                d = self.sizes.get(o, 0)
                if cap is not None and out + d > cap:
                    if i == 0:
                        return E_CAPACITY, 0, 0, 0, d
                    consumed, need = o - self.pos, 0
                    open_ = True  # (only a block has output: the cut lies inside a frame)
                    break
                out += d
        self.pos += consumed
        while self.cur < np_ and self.off[self.cur + 1] <= self.pos:
            self.cur += 1
        self.open = open_ if consumed else self.open
        return OK, consumed, out, (need if consumed == 0 else 0), 0

    @property
    def at_end(self):
        return self.pos == self.off[-1]
