"""(GPU) map-side LZ4 compress + Adler32 across spark.io.compression.lz4.blockSize: 16k / 32k (the default) / 48k / 64k through
S3S_OPT_LZ4_BLOCK_SIZE (liblz4's 16-bit-table parse), 128k / 256k / 1m / 4m through S3S_OPT_LZ4_BLOCK_SIZE_LARGE (ABI 10: chunks of
65 547 bytes and more are its 32-bit-table parse, one wavefront per chunk).  TeraSort map outputs of 200 partitions (and wide rows)
resident in HBM, the batched device entry point with 2 map tasks per call and 4 calls in flight like bench.py's headline.  The CPU
leg is liblz4 itself through ctypes on 16 host cores over the same blocks (worker processes, windows of at least 0.6 s, median
of five and their range: see cpu_leg).

usage: python tools/lz4_block_size_bench.py [--maps 8] [--steps 10] [--sizes 32768,131072] [--inputs terasort,wide]
                                            [--variant 1|10] [--cpu-threads 16] [--out profiles/lz4_big_blocks_tool]
A library older than ABI 10 (S3S_CODEC_LIB) runs the sizes up to 64k."""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
import numpy as np  # noqa: E402

OPT_LZ4_BLOCK_SIZE, OPT_LZ4_VARIANT, OPT_LZ4_BLOCK_SIZE_LARGE = 1, 4, 8


_LEG = {}
CPU_WINDOW_S, CPU_REPEATS = 0.6, 5   # every timed window covers at least this many seconds; this many windows, median reported


def _leg_share(k):
    """one worker's share of the blocks: a warm pass, then CPU_REPEATS windows of `passes` passes each, every window started
    behind a barrier -> [(start, end)] per window on the shared clock"""
    L, data, bs, shares, passes = _LEG["lib"], _LEG["data"], _LEG["bs"], _LEG["shares"], _LEG["passes"]
    bound = L.LZ4_compressBound(bs)
    out = np.empty(bound, np.uint8)
    base = data.ctypes.data

    def one_pass():
        for p, ln in shares[k]:
            L.LZ4_compress_default(base + p, out.ctypes.data, ln, bound)

    one_pass()
    spans = []
    for _ in range(CPU_REPEATS):
        _LEG["barrier"].wait()  # the windows of all workers run side by side
        t0 = time.time()
        for _ in range(passes):
            one_pass()
        spans.append((t0, time.time()))
    return spans


def cpu_leg(data, bs, workers):
    """(median, min, max) GB/s of liblz4's LZ4_compress_default (ctypes) over the blocks of one map output on `workers` host
    cores, blocks dealt out in contiguous runs.  One pass over 128 MiB takes 16 cores a few milliseconds - a window that
    measures the scheduler - so a window is as many passes as fill CPU_WINDOW_S (sized from a first pass), first worker's start
    to last worker's end, and CPU_REPEATS of them are taken.  Worker PROCESSES, forked before this process opens the GPU: with
    threads the interpreter lock between two 10 us calls, not liblz4, sets the figure at small block sizes."""
    import multiprocessing

    L = ctypes.CDLL("liblz4.so.1")
    L.LZ4_compress_default.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.LZ4_compressBound.argtypes = [ctypes.c_int]
    blocks = [(p, min(bs, data.size - p)) for p in range(0, data.size, bs)]
    per = (len(blocks) + workers - 1) // workers
    shares = [blocks[i:i + per] for i in range(0, len(blocks), per)]
    # one share on this core alone gives the length of a pass (an underestimate once all cores run: the window only gets longer)
    out = np.empty(L.LZ4_compressBound(bs), np.uint8)
    t0 = time.time()
    for p, ln in shares[0]:
        L.LZ4_compress_default(data.ctypes.data + p, out.ctypes.data, ln, out.size)
    passes = max(1, int(CPU_WINDOW_S / max(time.time() - t0, 1e-4)) + 1)
    mp = multiprocessing.get_context("fork")
    _LEG.update(lib=L, data=data, bs=bs, shares=shares, passes=passes, barrier=mp.Barrier(len(shares)))
    with mp.Pool(len(shares)) as pool:
        spans = pool.map(_leg_share, range(len(shares)), chunksize=1)
    rates = sorted(passes * data.size / (max(w[r][1] for w in spans) - min(w[r][0] for w in spans)) / 1e9 for r in range(CPU_REPEATS))
    return rates[len(rates) // 2], rates[0], rates[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--sizes", default="16384,32768,49152,65536,131072,262144,1048576,4194304")
    ap.add_argument("--inputs", default="terasort,wide")
    ap.add_argument("--variant", type=int, default=0, help="S3S_OPT_LZ4_VARIANT (0: the library's default)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="0: no liblz4 leg")
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    args = ap.parse_args()
    from s3shuffle import datagen

    def make(name, m):
        return (datagen.terasort_map_output(args.mib << 20, 200, seed=2, map_id=m) if name == "terasort"
                else datagen.tpcds_wide_map_output(args.mib << 20, 64, seed=3, map_id=m))

    sizes = [int(x) for x in args.sizes.split(",")]
    cpu = {}
    if args.cpu_threads > 0:  # (before the GPU is opened: the workers are forked)
        for name in args.inputs.split(","):
            d0 = make(name, 0)[0]
            for bs in sizes:
                cpu[(name, bs)] = cpu_leg(d0, bs, args.cpu_threads)
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    n_threads = 4
    codecs = [s3shuffle.Codec(0) for _ in range(n_threads)]
    abi = int(codecs[0]._lib.s3s_abi_version())
    lines, rows = [], []
    for name in args.inputs.split(","):
        outs = [make(name, m) for m in range(args.maps)]
        d_src = [torch.from_numpy(d.copy()).to(dev) for d, _ in outs]
        for bs in sizes:
            if bs > 65536 and abi < 10:
                continue
            for c in codecs:
                c.set_option(OPT_LZ4_BLOCK_SIZE_LARGE if bs > 65536 else OPT_LZ4_BLOCK_SIZE, bs)
                if args.variant:
                    c.set_option(OPT_LZ4_VARIANT, args.variant)
            caps = [codecs[0].max_compressed_size(s3shuffle.CODEC_LZ4, o) for _, o in outs]
            d_dst = [torch.empty(cap, dtype=torch.uint8, device=dev) for cap in caps]
            per = args.maps // n_threads
            totals = [0] * n_threads

            def work(t, steps):
                tasks = [(d_src[i].data_ptr(), outs[i][1], d_dst[i].data_ptr(), caps[i]) for i in range(t * per, (t + 1) * per)]
                for _ in range(steps):
                    res = codecs[t].compress_map_outputs_batch_device(s3shuffle.CODEC_LZ4, s3shuffle.CHECKSUM_ADLER32, tasks)
                totals[t] = sum(r[0] for r in res)

            def run(steps):
                th = [threading.Thread(target=work, args=(t, steps)) for t in range(n_threads)]
                for x in th:
                    x.start()
                for x in th:
                    x.join()
                torch.cuda.synchronize()

            run(3)
            t0 = time.perf_counter()
            run(args.steps)
            dt = (time.perf_counter() - t0) / args.steps
            raw = sum(d.size for d, _ in outs[: per * n_threads])
            gbs = raw / dt / 1e9
            cpu_gbs, cpu_lo, cpu_hi = cpu.get((name, bs), (0.0, 0.0, 0.0))
            chunks = sum(int(np.sum((np.diff(o) + bs - 1) // bs)) for _, o in outs[: per * n_threads]) // n_threads
            line = (f"{name:9s} lz4.blockSize {bs >> 10:5d}k: {gbs:6.1f} GB/s compress + Adler32 ({dt * 1e3:.2f} ms per {per * n_threads} x {args.mib} MiB, "
                    f"{chunks} chunks per call), ratio {raw / sum(totals):.3f}"
                    + (f", liblz4 on {args.cpu_threads} cores {cpu_gbs:5.2f} GB/s (median of {CPU_REPEATS} windows of >= {CPU_WINDOW_S} s, {cpu_lo:.2f} - {cpu_hi:.2f}), GPU / CPU {gbs / cpu_gbs:5.2f}" if cpu_gbs else "")
                    + (f", parse variant {args.variant}" if args.variant else ""))
            print(line, flush=True)
            lines.append(line)
            rows.append(dict(input=name, block=bs, gbs=round(gbs, 2), ms=round(dt * 1e3, 3), ratio=round(raw / sum(totals), 4),
                             chunks_per_call=chunks, cpu_threads=args.cpu_threads, cpu_gbs=round(cpu_gbs, 3), cpu_gbs_min=round(cpu_lo, 3), cpu_gbs_max=round(cpu_hi, 3), variant=args.variant, abi=abi))
            del d_dst
        del d_src
    for c in codecs:
        c.close()
    if args.out:
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
