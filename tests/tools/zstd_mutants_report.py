"""(CPU) The figures of profiles/zstd_mutants.md: the mutants of tests/zstd_mutants.py through the host models, per family - verdict
histogram, shares that complete blocks on the block and staged paths, the two deviations from libzstd - and, for the mutants the
product refuses and libzstd decodes, where the damage lies in the seed frame (TEST INFRASTRUCTURE).

    python tests/tools/zstd_mutants_report.py [--seed 1] [--count 2000]

Reported, not asserted: tests/test_zstd_mutants_model.py holds the hard properties."""
import argparse
import collections
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, os.path.join(ROOT, "spark-s3-shuffle_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def sections(part):
    """[(first byte, one past the last, name)] of a valid partition: frame headers, block headers, literals and sequences sections."""
    import zstd_staged_lib as S
    import zstd_stream_lib as L

    out, at = [], 0
    while at < len(part):
        hb = S.frame_header_bytes(part, at)[0]
        out.append((at, at + hb, "frame header"))
        p = at + hb
        for last, t, size in S.block_headers(part, at)[0]:
            out.append((p, p + 3, "block header"))
            stored = 1 if t == 1 else size
            if t == 2:
                lit_end, huf = L._literals_end(part[p + 3:p + 3 + size])
                out.append((p + 3, p + 3 + lit_end, "Huffman literals" if huf else "raw / RLE literals"))
                out.append((p + 3 + lit_end, p + 3 + size, "sequences section"))
            else:
                out.append((p + 3, p + 3 + stored, "raw / RLE block"))
            p += 3 + stored
        at = p
    return out


def where_damaged(data, family):
    """The sections of the closest seed frame that a same-length mutant changed (None: the length changed)."""
    import zstd_mutants as M

    same = [f for f, _ in M.seeds(family) if len(f) == len(data)]
    if not same:
        return None
    a = np.frombuffer(data, np.uint8)
    seed = min(same, key=lambda f: int(np.count_nonzero(np.frombuffer(f, np.uint8) != a)))
    diff = np.flatnonzero(np.frombuffer(seed, np.uint8) != a)
    names = set()
    for lo, hi, name in sections(seed):
        if np.any((diff >= lo) & (diff < hi)):
            names.add(name)
    return " + ".join(sorted(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--count", type=int, default=2000)
    a = ap.parse_args()
    import zstd_block_parallel_lib as ZB
    import zstd_model_lib as ZM
    import zstd_mutants as M
    import zstd_staged_lib as S
    from oracle import zstd_ref

    sm, bm, gm = ZM.load(), ZB.load(), S.load()
    total = collections.Counter()
    places = collections.Counter()
    print("| family | mutants | accepted | bad frame | capacity | unsupported | blocks on the block path | on the staged path | behind the block path | "
          "product refuses, libzstd decodes (at the seed's full length) | product decodes, libzstd refuses |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for family in M.FAMILIES:
        v = collections.Counter()
        n_path = n_staged = n_staged13 = strict = strict_full = lenient = 0
        for index, data, size, cap in M.mutants(family, a.seed, a.count):
            comp = np.frombuffer(data, np.uint8)
            rc, out = M.serial_at(sm, comp, cap)
            v[rc] += 1
            n_path += ZB.decode(bm, comp, cap).path_blocks > 0
            n_staged += S.decode(gm, comp, cap).staged_blocks > 0
            n_staged13 += S.decode(gm, comp, cap, block_path=True).staged_blocks > 0
            ref = zstd_ref.decompress(comp, cap)
            if rc != 0 and ref is not None:
                strict += 1
                strict_full += ref.size == size
                places[(rc, where_damaged(data, family) or "length changed (splice, insertion, deletion, truncation)")] += 1
            elif rc == 0 and ref is None:
                lenient += 1
        pc = lambda n: "%d (%.1f %%)" % (n, 100.0 * n / a.count)  # noqa: E731
        print("| %s | %d | %s | %d | %d | %d | %s | %s | %s | %d (%d) | %d |"
              % (family, a.count, pc(v[0]), v[-3], v[-2], v[-6], pc(n_path), pc(n_staged), pc(n_staged13), strict, strict_full, lenient))
        total.update({"mutants": a.count, "strict": strict, "strict_full": strict_full, "lenient": lenient, "accepted": v[0]})
    print("\nall families:", dict(total))
    print("\nproduct refuses, libzstd decodes - the product's code and the sections of the seed frame that were changed:")
    for (rc, name), n in sorted(places.items(), key=lambda kv: -kv[1]):
        print("| %d | %s | %d |" % (rc, name, n))


if __name__ == "__main__":
    main()
