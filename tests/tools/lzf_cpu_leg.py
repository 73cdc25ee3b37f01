"""(CPU) The fallback host leg of tools/lzf_compress_bench.py for machines without liblzf (TEST INFRASTRUCTURE: the oracle's
16-thread map-task bench with its own greedy LZF encoder - NOT liblzf -, kept under tests/ like every other user of the oracle).
Prints one JSON line.

    python tests/tools/lzf_cpu_leg.py --input wide|terasort --mib 128 --threads 16"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "spark-s3-shuffle_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", default="wide")
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from oracle import binding as oracle
    from s3shuffle import datagen

    if a.input == "terasort":
        data, offs = datagen.terasort_map_output(a.mib << 20, 200, seed=2, map_id=0)
    else:
        data, offs = datagen.tpcds_wide_map_output(a.mib << 20, 64, seed=3, map_id=0)
    s, _ = oracle.mt_compress_bench(oracle.CODEC_LZF, oracle.CHECKSUM_NONE, data, offs, a.threads, 1)  # one map task per thread
    size = oracle.compress_map_output(oracle.CODEC_LZF, oracle.CHECKSUM_NONE, data, offs)[0].size
    print(json.dumps(dict(gbs=a.threads * data.size / s / 1e9 if s > 0 else 0.0, out_bytes=int(size))), flush=True)


if __name__ == "__main__":
    main()
