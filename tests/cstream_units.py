"""The contract of the streaming map side (s3s_cstream_*, include/s3shuffle_codec.h) as a Python model.

The model knows nothing of the library: it is given the codec, the block size and, per partition of a map output, the image
sizes of the partition's units (read from a one-shot image, `unit_sizes_from_image`), and says for every feed of a schedule what
the stream must answer: consumed / out_len / need_src / need_dst / parts_closed / lengths.

Units: a block (block-size source bytes of the open partition, or what is left of a partition whose end lies in the window;
Snappy's 16-byte stream header belongs to the first block's unit), and the 21-byte end frame of a non-empty LZ4 partition.  An
end without bytes of its own is passed as soon as every unit in front of it is taken.  S3S_CODEC_NONE: a unit is a byte.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Callable, List, Sequence

NONE, LZ4, SNAPPY, ZSTD, LZF = 0, 1, 2, 3, 4
E_CAPACITY = -2
LZ4_END = 21
LZF_BLOCK = 65535


def block_size(codec: int, configured: int) -> int:
    """The block size in force: what need_src reports."""
    if codec == LZF:
        return LZF_BLOCK
    if codec == SNAPPY:
        return max(int(configured), 1024)
    if codec == NONE:
        return 1
    return int(configured)


def unit_sizes_from_image(codec: int, image: bytes, index: Sequence[int]) -> List[List[int]]:
    """Per partition of a .data image: the image sizes of its units, in order."""
    image = bytes(image)
    out = []
    for p in range(len(index) - 1):
        a, b = int(index[p]), int(index[p + 1])
        sizes = []
        pos = a
        if codec == LZ4:
            while pos < b:
                assert image[pos:pos + 8] == b"LZ4Block"
                clen = struct.unpack_from("<i", image, pos + 9)[0]
                sizes.append(21 + clen)
                pos += 21 + clen
            assert not sizes or sizes[-1] == LZ4_END
        elif codec == SNAPPY:
            head = 0
            if pos < b:
                assert image[pos:pos + 8] == b"\x82SNAPPY\x00"
                head, pos = 16, pos + 16
            while pos < b:
                clen = struct.unpack_from(">i", image, pos)[0]
                sizes.append(head + 4 + clen)
                head = 0
                pos += 4 + clen
        elif codec == LZF:
            while pos < b:
                assert image[pos:pos + 2] == b"ZV"
                clen = struct.unpack_from(">H", image, pos + 3)[0]
                n = (7 if image[pos + 2] == 1 else 5) + clen
                sizes.append(n)
                pos += n
        else:
            sizes = [1] * (b - a)
        assert pos == b or codec == NONE, (codec, p, pos, b)
        out.append(sizes)
    return out


@dataclass
class Feed:
    code: int = 0
    consumed: int = 0
    out_len: int = 0
    need_src: int = 0
    need_dst: int = 0
    parts_closed: int = 0
    lengths: List[int] = field(default_factory=list)

    def fields(self):
        return (self.code, self.consumed, self.out_len, self.need_src, self.need_dst, self.parts_closed, tuple(self.lengths))


class Model:
    def __init__(self, codec: int, bs: int, unit_sizes: List[List[int]]):
        self.codec, self.bs, self.sizes = codec, (1 if codec == NONE else bs), unit_sizes
        self.pos = self.written = self.open_bytes = self.open_img = self.n_closed = 0

    def _units(self, src_len: int, ends: Sequence[int]):
        """(source offset behind the unit, image size, piece) of every unit the window shows, in order."""
        units, start, bs = [], 0, self.bs
        for j in range(len(ends) + 1):
            closes = j < len(ends)
            had = self.open_bytes if j == 0 else 0
            length = (ends[j] if closes else src_len) - start
            take = length if closes else length - length % bs
            part = self.n_closed + j
            for p in range(0, take, bs):
                units.append((start + min(p + bs, take), 1 if self.codec == NONE else self.sizes[part][(had + p) // bs], j))
            if closes and self.codec == LZ4 and had + length > 0:
                units.append((ends[j], LZ4_END, j))
            if closes:
                start = ends[j]
        return units

    def feed(self, src_len: int, ends: Sequence[int], cap: int) -> Feed:
        ends = [int(e) for e in ends]
        assert all(0 <= e <= src_len for e in ends) and ends == sorted(ends)
        units = self._units(src_len, ends)
        k = out = 0
        piece_img = [0] * (len(ends) + 1)
        while k < len(units) and out + units[k][1] <= cap:
            out += units[k][1]
            piece_img[units[k][2]] += units[k][1]
            k += 1
        closed = units[k][2] if k < len(units) else len(ends)  # every end in front of the first unit left behind
        f = Feed()
        if k == 0 and units and closed == 0:
            f.code, f.need_dst = E_CAPACITY, units[0][1]
            return f
        f.consumed = units[k - 1][0] if k else 0
        f.out_len, f.parts_closed = out, closed
        f.lengths = [piece_img[j] + (self.open_img if j == 0 else 0) for j in range(closed)]
        if not units and not ends:
            f.need_src = self.bs
        self.pos += f.consumed
        self.written += out
        if closed:
            self.n_closed += closed
            self.open_bytes = f.consumed - ends[closed - 1]
            self.open_img = piece_img[closed]
        else:
            self.open_bytes += f.consumed
            self.open_img += out
        return f


def ends_in_window(offsets: Sequence[int], pos: int, n_closed: int, wlen: int) -> List[int]:
    """The window-relative ends of the partitions that are not closed yet and end inside [pos, pos + wlen]."""
    return [int(offsets[p + 1]) - pos for p in range(n_closed, len(offsets) - 1) if int(offsets[p + 1]) <= pos + wlen]


def drive(offsets: Sequence[int], feed: Callable[[int, int, List[int], int], Feed], window_of: Callable[[int, int], int],
          cap_of: Callable[[int, int, int], int], max_steps: int = 100000) -> int:
    """Runs a schedule to the end of the map output: window_of(step, pos) -> window length, cap_of(step, wlen, n_ends) ->
    capacity; feed(pos, wlen, ends, cap) performs the feed (on the model, the stream, or both) and returns its Feed.  A feed
    that asks for more (need_dst, need_src) is repeated with what it asked for.  Returns the number of feeds."""
    total, nparts = int(offsets[-1]), len(offsets) - 1
    pos = n_closed = steps = 0
    want_w = want_c = 0
    while pos < total or n_closed < nparts:
        assert steps < max_steps, "the schedule does not end"
        wlen = min(max(window_of(steps, pos), want_w), total - pos)
        ends = ends_in_window(offsets, pos, n_closed, wlen)
        cap = max(cap_of(steps, wlen, len(ends)), want_c)
        f = feed(pos, wlen, ends, cap)
        steps += 1
        want_w = want_c = 0
        if f.code == E_CAPACITY:
            assert f.need_dst > cap and f.consumed == 0 and f.out_len == 0 and f.parts_closed == 0
            want_w, want_c = wlen, f.need_dst
            continue
        assert f.code == 0
        if f.consumed == 0 and f.parts_closed == 0:
            assert f.need_src > wlen or wlen == 0, (f.fields(), wlen)
            want_w = f.need_src
            continue
        pos += f.consumed
        n_closed += f.parts_closed
    return steps
