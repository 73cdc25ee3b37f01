"""The contract of the streaming map side under IO encryption (s3s_cstream_open_encrypted, include/s3shuffle_codec.h) as a
Python model, built on the plain stream's (cstream_units.py).

The deltas: the 16-byte IV of a non-empty partition belongs to the unit of the partition's first block (S3S_CODEC_NONE: the unit
of a partition's first byte is 17 image bytes), an empty partition stays 0 bytes, and every size the stream answers counts stored
bytes.  So the model is the plain one over unit sizes that have 16 added to the first unit of each non-empty partition; the unit
sizes are still read from the PLAIN one-shot image.  need_dst and feed_bound are restated here."""
from __future__ import annotations

from typing import List, Sequence

import cstream_units as cu
from cstream_units import E_CAPACITY, LZ4, LZ4_END, LZF, NONE, SNAPPY, Feed, block_size, drive, ends_in_window  # noqa: F401

IV = 16


def encrypted_unit_sizes(plain_sizes: Sequence[Sequence[int]]) -> List[List[int]]:
    """unit sizes of the plain image -> of the stored image: 16 on the first unit of each non-empty partition"""
    return [[int(s[0]) + IV] + [int(x) for x in s[1:]] if len(s) else [] for s in plain_sizes]


def unit_sizes_from_plain_image(codec: int, image: bytes, index: Sequence[int]) -> List[List[int]]:
    return encrypted_unit_sizes(cu.unit_sizes_from_image(codec, image, index))


def stored_index(plain_index: Sequence[int]) -> List[int]:
    """the .index of the stored image: 16 more for every non-empty partition"""
    out = [0]
    for p in range(len(plain_index) - 1):
        n = int(plain_index[p + 1]) - int(plain_index[p])
        out.append(out[-1] + (n + IV if n else 0))
    return out


def need_dst_first(codec: int, first_unit_plain: int) -> int:
    """need_dst of a feed whose first unit is a partition's first block (NONE: 17, else 1 inside a partition)"""
    return (1 if codec == NONE else first_unit_plain) + IV


def feed_bound(codec: int, bs: int, src_len: int, n_ends: int) -> int:
    """s3s_cstream_feed_bound of an encrypted stream: the plain bound and one IV for every piece"""
    if codec == NONE:
        plain = src_len
    else:
        blocks = src_len // bs + n_ends + 1
        plain = {LZ4: src_len + 21 * (blocks + n_ends), SNAPPY: src_len + src_len // 6 + 37 * blocks + 16 * (n_ends + 1),
                 LZF: src_len + 7 * blocks}[codec]
    return plain + IV * (n_ends + 1)


class Model(cu.Model):
    """cu.Model over stored unit sizes.  For NONE the sizes are not looked up: a byte is a unit, the first of a partition 17."""

    def _units(self, src_len: int, ends: Sequence[int]):
        if self.codec != NONE:
            return super()._units(src_len, ends)
        units, start = [], 0
        for j in range(len(ends) + 1):
            had = self.open_bytes if j == 0 else 0
            end = ends[j] if j < len(ends) else src_len
            for p in range(end - start):
                units.append((start + p + 1, 1 + IV if had + p == 0 else 1, j))
            start = end
        return units
