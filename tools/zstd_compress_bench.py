"""(GPU) map-side Zstandard compress + Adler32 (S3S_OPT_ZSTD_COMPRESS = 1, ABI 11) next to the LZ4 line of the same machine:
TeraSort map outputs of 200 partitions and wide rows resident in HBM, the batched device entry point with 2 map tasks per call and
4 calls in flight like bench.py's headline.  Reports GB/s of SOURCE bytes, output / source, and - from one profiled call on one
context (S3S_OPT_PROFILE) - the stage times.  The CPU leg is libzstd level 1 (Spark's default, one frame per partition) through
ctypes on 16 host processes over the same partitions: windows of at least 0.6 s, median of five and their range.

usage: python tools/zstd_compress_bench.py [--maps 8] [--steps 5] [--mib 128] [--inputs terasort,wide] [--cpu-threads 16]
                                           [--out profiles/zstd_compress_tool]"""
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

OPT_PROFILE, OPT_ZSTD_COMPRESS = 3, 9
_LEG = {}
CPU_WINDOW_S, CPU_REPEATS = 0.6, 5


def _zstd():
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_compress.restype = ctypes.c_size_t
    z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return z


def _leg_share(k):
    z, data, shares, passes = _LEG["lib"], _LEG["data"], _LEG["shares"], _LEG["passes"]
    bound = z.ZSTD_compressBound(max(ln for _, ln in shares[k]))
    out = np.empty(bound, np.uint8)
    base = data.ctypes.data

    def one_pass():
        return sum(z.ZSTD_compress(out.ctypes.data, bound, base + p, ln, 1) for p, ln in shares[k])

    size = one_pass()
    spans = []
    for _ in range(CPU_REPEATS):
        _LEG["barrier"].wait()
        t0 = time.time()
        for _ in range(passes):
            one_pass()
        spans.append((t0, time.time()))
    return spans, size


def cpu_leg(data, offs, workers):
    """(median, min, max GB/s, compressed bytes) of ZSTD_compress(level 1), one frame per partition, partitions dealt out in
    contiguous runs to `workers` processes forked before this process opens the GPU."""
    import multiprocessing

    z = _zstd()
    parts = [(int(offs[p]), int(offs[p + 1] - offs[p])) for p in range(len(offs) - 1) if offs[p + 1] > offs[p]]
    per = (len(parts) + workers - 1) // workers
    shares = [parts[i:i + per] for i in range(0, len(parts), per)]
    out = np.empty(z.ZSTD_compressBound(max(ln for _, ln in parts)), np.uint8)
    t0 = time.time()
    for p, ln in shares[0]:
        z.ZSTD_compress(out.ctypes.data, out.size, data.ctypes.data + p, ln, 1)
    passes = max(1, int(CPU_WINDOW_S / max(time.time() - t0, 1e-4)) + 1)
    mp = multiprocessing.get_context("fork")
    _LEG.update(lib=z, data=data, shares=shares, passes=passes, barrier=mp.Barrier(len(shares)))
    with mp.Pool(len(shares)) as pool:
        res = pool.map(_leg_share, range(len(shares)), chunksize=1)
    spans = [r[0] for r in res]
    rates = sorted(passes * data.size / (max(w[r][1] for w in spans) - min(w[r][0] for w in spans)) / 1e9 for r in range(CPU_REPEATS))
    return rates[len(rates) // 2], rates[0], rates[-1], sum(r[1] for r in res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--inputs", default="terasort,wide")
    ap.add_argument("--cpu-threads", type=int, default=16, help="0: no libzstd leg")
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    args = ap.parse_args()
    from s3shuffle import datagen

    def make(name, m):
        return (datagen.terasort_map_output(args.mib << 20, 200, seed=2, map_id=m) if name == "terasort"
                else datagen.tpcds_wide_map_output(args.mib << 20, 64, seed=3, map_id=m))

    cpu = {}
    if args.cpu_threads > 0:  # (before the GPU is opened: the workers are forked)
        for name in args.inputs.split(","):
            cpu[name] = cpu_leg(*make(name, 0), args.cpu_threads)
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    n_threads = 4
    codecs = [s3shuffle.Codec(0) for _ in range(n_threads)]
    for c in codecs:
        c.set_option(OPT_ZSTD_COMPRESS, 1)
    lines, rows = [], []
    for name in args.inputs.split(","):
        outs = [make(name, m) for m in range(args.maps)]
        d_src = [torch.from_numpy(d.copy()).to(dev) for d, _ in outs]
        per = args.maps // n_threads
        raw = sum(d.size for d, _ in outs[: per * n_threads])
        for codec_id, label in ((s3shuffle.CODEC_ZSTD, "zstd"), (s3shuffle.CODEC_LZ4, "lz4 32k")):
            caps = [codecs[0].max_compressed_size(codec_id, o) for _, o in outs]
            d_dst = [torch.empty(cap, dtype=torch.uint8, device=dev) for cap in caps]
            totals = [0] * n_threads

            def work(t, steps):
                tasks = [(d_src[i].data_ptr(), outs[i][1], d_dst[i].data_ptr(), caps[i]) for i in range(t * per, (t + 1) * per)]
                for _ in range(steps):
                    res = codecs[t].compress_map_outputs_batch_device(codec_id, s3shuffle.CHECKSUM_ADLER32, tasks)
                totals[t] = sum(r[0] for r in res)

            def run(steps):
                th = [threading.Thread(target=work, args=(t, steps)) for t in range(n_threads)]
                for x in th:
                    x.start()
                for x in th:
                    x.join()
                torch.cuda.synchronize()

            run(2)
            t0 = time.perf_counter()
            run(args.steps)
            dt = (time.perf_counter() - t0) / args.steps
            gbs = raw / dt / 1e9
            # stage times: one profiled call of one map task on one context, nothing else in flight
            codecs[0].set_option(OPT_PROFILE, 1)
            codecs[0].compress_map_output_device(codec_id, s3shuffle.CHECKSUM_ADLER32, d_src[0].data_ptr(), outs[0][1], d_dst[0].data_ptr(), caps[0])
            stages = {k: round(codecs[0].stage_ms(v), 3) for k, v in (("total", 0), ("codec", 1), ("assemble", 2), ("checksum", 3), ("hash", 5))}
            codecs[0].set_option(OPT_PROFILE, 0)
            line = (f"{name:9s} {label:8s}: {gbs:6.2f} GB/s compress + Adler32 of source bytes ({dt * 1e3:.1f} ms per {per * n_threads} x {args.mib} MiB), "
                    f"output / source {sum(totals) / raw:.4f}; one {args.mib} MiB task alone, ms: {stages}")
            if codec_id == s3shuffle.CODEC_ZSTD and name in cpu:
                med, lo, hi, csize = cpu[name]
                line += (f"; libzstd level 1 on {args.cpu_threads} processes {med:.2f} GB/s (median of {CPU_REPEATS} windows of >= {CPU_WINDOW_S} s, "
                         f"{lo:.2f} - {hi:.2f}), output / source {csize / outs[0][0].size:.4f}, GPU / CPU {gbs / med:.2f}")
            print(line, flush=True)
            lines.append(line)
            rows.append(dict(input=name, codec=label, gbs=round(gbs, 3), ms=round(dt * 1e3, 2), out_over_src=round(sum(totals) / raw, 5), stages_ms=stages,
                             cpu=[round(x, 4) for x in cpu[name][:3]] + [round(cpu[name][3] / outs[0][0].size, 5)] if codec_id == s3shuffle.CODEC_ZSTD and name in cpu else None))
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
