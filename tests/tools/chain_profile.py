"""The window block's chain in the interpreter model, per build (TEST INFRASTRUCTURE, no GPU): instructions, taken branches
and model cycles per 32 KiB block of both bench generators, and the same per label of the hand-written block.

    python tests/tools/chain_profile.py [--l2] [--blocks N] [--rows N] [--labels a,b,..] [-DFLAG ...]

Builds the input-ring kernel (variant 11; --l2: the variant-10 kernel) with the given -D flags and runs N TeraSort and N
wide-row blocks (the blocks of block_profile.py).  Run it once per build and set the outputs side by side: the gate for a
change of the block is "model cycles drop on TeraSort and do not rise on wide rows"."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, os.path.join(TESTS, "isa"), os.path.join(ROOT, "spark-s3-shuffle_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402

from s3shuffle import datagen  # noqa: E402

import lz4_chain_kernel as ck  # noqa: E402

WORKLOADS = (("terasort", datagen.terasort_map_output, 2), ("tpcds-wide", datagen.tpcds_wide_map_output, 3))


def blocks(gen, seed, n):
    data, offs = gen(8 << 20, 12, seed=seed, map_id=0)
    data = np.asarray(data, dtype=np.uint8)
    p0 = int(offs[3])
    return [data[p0 + k * 32768: p0 + (k + 1) * 32768] for k in range(n)]


def profile(chunks, ring, flags):
    prof = {}
    out = ck.compress_chunks(chunks, ring=ring, flags=flags, profile=prof)
    ws = [o[2] for o in out]
    agg = {}
    for k, v in prof.items():
        # .Lw_<name><body 0..2>_<number of the asm statement>: the three bodies of a label count as one (the name may end in a digit)
        kk = re.sub(r"[012]?_\d+$", "", k) if k.startswith(".Lw_") else "compiled code"
        a = agg.setdefault(kk, [0, 0, 0])
        a[0] += v[0]
        a[1] += v[1]
        a[2] += v[2] if len(v) > 2 else 0
    return agg, sum(w.clock for w in ws), sum(w.n_taken for w in ws)


def main():
    args = sys.argv[1:]
    flags = tuple(a for a in args if a.startswith("-D"))
    ring = "--l2" not in args
    opt = lambda name, d: args[args.index(name) + 1] if name in args else d  # noqa: E731
    n, rows = int(opt("--blocks", "3")), int(opt("--rows", "14"))
    only = [x for x in opt("--labels", "").split(",") if x]
    print("build: %s %s" % ("ring (variant 11)" if ring else "variant 10", " ".join(flags) or "(default)"))
    for name, gen, seed in WORKLOADS:
        agg, cycles, taken = profile(blocks(gen, seed, n), ring, flags)
        tot_i = sum(v[0] for v in agg.values())
        print("%-10s per block: instructions %7d  taken branches %5d  model cycles %8d" % (name, tot_i / n, taken / n, cycles / n))
        keys = [".Lw_" + x for x in only] if only else [k for k, _ in sorted(agg.items(), key=lambda kv: -kv[1][2])[:rows]]
        for k in keys:
            v = agg.get(k, [0, 0, 0])
            print("   %-16s instructions %7d (%4.1f %%)  taken branches %5d  model cycles %8d (%4.1f %%)" % (
                k, v[0] / n, 100 * v[0] / tot_i, v[1] / n, v[2] / n, 100 * v[2] / cycles))


if __name__ == "__main__":
    main()
