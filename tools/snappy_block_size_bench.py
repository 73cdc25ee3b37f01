"""(GPU) Snappy at spark.io.compression.snappy.blockSize = 32k (the default) / 64k / 128k / 1m (ABI 9: chunks above one 64 KiB
fragment are compressed one wavefront per fragment, and the batch decoder takes chunks of any size up to 32 MiB).
Map side: compress + Adler32 through the batched device entry point, 2 map tasks per call and 4 calls in flight like
bench.py's headline.  Reduce side: verify + decode of the same images through s3s_decompress_ranges_batch_device, 4 calls in
flight.  Inputs: TeraSort and TPC-DS-like wide rows, map outputs of --mib MiB (200 / 64 partitions) resident in HBM.  Also the
compression ratio at each size and the 16-core libsnappy leg at the same block sizes (oracle.mt_compress_bench, run as a child
process by tests/tools/snappy_cpu_leg.py: the oracle is test infrastructure and stays under tests/).
usage: python tools/snappy_block_size_bench.py [--maps 8] [--steps 5] [--mib 128] [--json out.json]"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SIZES = (32768, 65536, 131072, 1 << 20)
N_THREADS = 4


def _threads(fn, steps):
    th = [threading.Thread(target=fn, args=(t, steps)) for t in range(N_THREADS)]
    for x in th:
        x.start()
    for x in th:
        x.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--json", default="")
    ap.add_argument("--sizes", default=",".join(str(x) for x in SIZES), help="block sizes, comma separated")
    ap.add_argument("--inputs", default="terasort,wide", help="terasort and / or wide")
    ap.add_argument("--no-cpu", action="store_true", help="skip the libsnappy leg (profiling runs)")
    args = ap.parse_args()
    import torch

    import s3shuffle
    from s3shuffle import datagen

    dev = torch.device("cuda", 0)
    SN, ADLER = s3shuffle.CODEC_SNAPPY, s3shuffle.CHECKSUM_ADLER32
    sizes = [int(x) for x in args.sizes.split(",")]
    inputs = {}
    if "terasort" in args.inputs:
        inputs["terasort"] = [datagen.terasort_map_output(args.mib << 20, 200, seed=2, map_id=m) for m in range(args.maps)]
    if "wide" in args.inputs:
        inputs["wide rows"] = [datagen.tpcds_wide_map_output(args.mib << 20, 64, seed=3, map_id=m) for m in range(args.maps)]
    codecs = [s3shuffle.Codec(0) for _ in range(N_THREADS)]
    per = args.maps // N_THREADS
    rows = []
    for name, outs in inputs.items():
        d_src = [torch.from_numpy(d.copy()).to(dev) for d, _ in outs]
        raw = sum(d.size for d, _ in outs[: per * N_THREADS])
        for bs in sizes:
            for c in codecs:
                c.set_option(2, bs)
            caps = [codecs[0].max_compressed_size(SN, o) for _, o in outs]
            d_dst = [torch.empty(cap, dtype=torch.uint8, device=dev) for cap in caps]
            res_all = [None] * N_THREADS

            def comp(t, steps):
                tasks = [(d_src[i].data_ptr(), outs[i][1], d_dst[i].data_ptr(), caps[i]) for i in range(t * per, (t + 1) * per)]
                for _ in range(steps):
                    res_all[t] = codecs[t].compress_map_outputs_batch_device(SN, ADLER, tasks)

            _threads(comp, 2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _threads(comp, args.steps)
            torch.cuda.synchronize()
            dt_c = (time.perf_counter() - t0) / args.steps
            res = [r for rs in res_all for r in rs]
            comp_bytes = sum(r[0] for r in res)
            d_out = [torch.empty(d.size, dtype=torch.uint8, device=dev) for d, _ in outs]

            def dec(t, steps):
                rng = [(d_dst[i].data_ptr(), res[i][0], res[i][1], res[i][2], d_out[i].data_ptr(), outs[i][0].size)
                       for i in range(t * per, (t + 1) * per)]
                for _ in range(steps):
                    codecs[t].decompress_ranges_batch_device(SN, ADLER, rng)

            _threads(dec, 2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _threads(dec, args.steps)
            torch.cuda.synchronize()
            dt_d = (time.perf_counter() - t0) / args.steps
            for i in range(per * N_THREADS):  # the decode is checked once per block size, outside the timing
                assert torch.equal(d_out[i], d_src[i]), f"{name} {bs}: map output {i} does not decode back"
            cpu = 0.0
            if not args.no_cpu:  # the first map output of this input, compressed by 16 libsnappy map tasks
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "snappy_cpu_leg.py"), "--input",
                                    "terasort" if name == "terasort" else "wide", "--mib", str(args.mib), "--threads",
                                    str(args.cpu_threads), "--sizes", str(bs)], check=True, capture_output=True, text=True)
                cpu = json.loads(r.stdout.strip().splitlines()[-1])["gbs"]
            row = dict(input=name, block=bs, compress_gbs=raw / dt_c / 1e9, decode_gbs=raw / dt_d / 1e9, ratio=raw / comp_bytes,
                       cpu_libsnappy_gbs=cpu)
            rows.append(row)
            print(f"{name:9s} snappy.blockSize {bs >> 10:5d}k: compress + Adler32 {row['compress_gbs']:6.1f} GB/s, verify + decode "
                  f"{row['decode_gbs']:6.1f} GB/s, ratio {row['ratio']:.3f}, {args.cpu_threads}-core libsnappy "
                  f"{row['cpu_libsnappy_gbs']:5.2f} GB/s", flush=True)
            del d_dst, d_out
        del d_src
    for name in inputs:
        base = next((r for r in rows if r["input"] == name and r["block"] == 32768), None)
        if base is None:
            continue
        for r in rows:
            if r["input"] == name and r["block"] != 32768:
                print(f"{name:9s} {r['block'] >> 10:5d}k / 32k: compress {r['compress_gbs'] / base['compress_gbs']:.2f}, "
                      f"decode {r['decode_gbs'] / base['decode_gbs']:.2f}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(maps=args.maps, mib=args.mib, steps=args.steps, rows=rows), f, indent=1)
    for c in codecs:
        c.close()


if __name__ == "__main__":
    main()
