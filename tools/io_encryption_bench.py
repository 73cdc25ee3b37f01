"""(GPU) what the Spark IO encryption layer (AES/CTR/NoPadding, s3s_set_io_encryption) costs: map outputs resident in HBM,
LZ4 + Adler32, compress and verify + decompress with the layer off and on, on the same library in the same run; and the AES-CTR
kernel's own rate over a 1 GiB image, from the library's HIP events on s3s_stream (S3S_OPT_PROFILE: with codec NONE and the
layer on, the assemble stage brackets exactly the kernel's launch).  The comparison is off against on, never against a target.
The host figure beside it is libcrypto's EVP aes-128-ctr on 16 processes, where the machine has libcrypto.

This process never opens the GPU: every input is one GPU step, a child process of its own under `timeout`, one after the other;
the first step that fails ends the run.

usage: python tools/io_encryption_bench.py [--maps 8] [--steps 5] [--mib 128] [--inputs terasort,wide] [--cpu-procs 16]
                                           [--step-timeout 240] [--out profiles/io_encryption_tool]"""
import argparse
import ctypes
import ctypes.util
import json
import multiprocessing
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
import numpy as np  # noqa: E402

OPT_PROFILE = 3
STAGES = (("total", 0), ("codec", 1), ("assemble", 2), ("checksum", 3), ("discover", 4), ("hash", 5))


def make(name, mib, m):
    from s3shuffle import datagen

    return (datagen.terasort_map_output(mib << 20, 200, seed=2, map_id=m) if name == "terasort"
            else datagen.tpcds_wide_map_output(mib << 20, 64, seed=3, map_id=m))


def _evp_worker(mib):
    """seconds one process needs for EVP aes-128-ctr over mib MiB (in place, 16 MiB at a time)"""
    name = ctypes.util.find_library("crypto")
    c = ctypes.CDLL(name)
    vp = ctypes.c_void_p
    c.EVP_CIPHER_CTX_new.restype = vp
    c.EVP_aes_128_ctr.restype = vp
    c.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, vp, vp]
    c.EVP_EncryptUpdate.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_int), vp, ctypes.c_int]
    c.EVP_CIPHER_CTX_free.argtypes = [vp]
    buf = np.random.default_rng(os.getpid()).integers(0, 256, 16 << 20, dtype=np.uint8)
    ctx = c.EVP_CIPHER_CTX_new()
    assert c.EVP_EncryptInit_ex(ctx, c.EVP_aes_128_ctr(), None, bytes(range(16)), bytes(16)) == 1
    n = ctypes.c_int(0)
    t0 = time.perf_counter()
    for _ in range(max(mib // 16, 1)):
        assert c.EVP_EncryptUpdate(ctx, buf.ctypes.data, ctypes.byref(n), buf.ctypes.data, buf.size) == 1
    dt = time.perf_counter() - t0
    c.EVP_CIPHER_CTX_free(ctx)
    return dt


def host_leg(procs, mib):
    if not ctypes.util.find_library("crypto"):
        return None
    with multiprocessing.get_context("spawn").Pool(procs) as pool:
        t0 = time.perf_counter()
        pool.map(_evp_worker, [mib] * procs)
        wall = time.perf_counter() - t0
    return dict(leg="libcrypto EVP aes-128-ctr on %d processes, %d MiB each (wall time of the pool's map)" % (procs, mib),
                gbs=round(procs * max(mib // 16, 1) * (16 << 20) / wall / 1e9, 2))


def gpu_step(name, args):
    """One input on the GPU (this process opens it).  Prints one JSON row."""
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    c = s3shuffle.Codec(0)
    key = bytes(range(16))
    outs = [make(name, args.mib, m) for m in range(args.maps)]
    d_src = [torch.from_numpy(d.copy()).to(dev) for d, _ in outs]
    raw = sum(d.size for d, _ in outs)
    n_parts = sum(len(o) - 1 for _, o in outs)
    ivs = np.random.default_rng(1).integers(0, 256, 16 * n_parts, dtype=np.uint8)
    row = dict(input=name, maps=args.maps, mib=args.mib)
    for mode in ("off", "on"):
        c.set_io_encryption(key if mode == "on" else None)
        caps = [c.max_compressed_size(s3shuffle.CODEC_LZ4, o) for _, o in outs]
        d_dst = [torch.empty(cap + 64, dtype=torch.uint8, device=dev) for cap in caps]
        tasks = [(d_src[i].data_ptr(), outs[i][1], d_dst[i].data_ptr(), caps[i]) for i in range(args.maps)]

        def compress():
            if mode == "on":
                c.set_stream_ivs(ivs)
            return c.compress_map_outputs_batch_device(s3shuffle.CODEC_LZ4, s3shuffle.CHECKSUM_ADLER32, tasks)

        for _ in range(2):
            res = compress()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = compress()
        dt = (time.perf_counter() - t0) / args.steps
        stored = sum(r[0] for r in res)
        d_back = [torch.empty(d.size + 64, dtype=torch.uint8, device=dev) for d, _ in outs]
        ranges = [(d_dst[i].data_ptr(), res[i][0], res[i][1], res[i][2], d_back[i].data_ptr(), outs[i][0].size) for i in range(args.maps)]
        for _ in range(2):
            dres = c.decompress_ranges_batch_device(s3shuffle.CODEC_LZ4, s3shuffle.CHECKSUM_ADLER32, ranges)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            dres = c.decompress_ranges_batch_device(s3shuffle.CODEC_LZ4, s3shuffle.CHECKSUM_ADLER32, ranges)
        ddt = (time.perf_counter() - t0) / args.steps
        assert all(st == 0 and nb == outs[i][0].size for i, (st, nb, _) in enumerate(dres))
        assert bool(torch.equal(d_back[0][: outs[0][0].size].cpu(), torch.from_numpy(outs[0][0])))
        # one profiled call of one map task alone: the stages (with the layer on the AES-CTR pass is inside "assemble")
        c.set_option(OPT_PROFILE, 1)
        if mode == "on":
            c.set_stream_ivs(ivs[: 16 * (len(outs[0][1]) - 1)])
        c.compress_map_output_device(s3shuffle.CODEC_LZ4, s3shuffle.CHECKSUM_ADLER32, d_src[0].data_ptr(), outs[0][1], d_dst[0].data_ptr(), caps[0])
        stages = {k: round(c.stage_ms(v), 3) for k, v in STAGES}
        c.set_option(OPT_PROFILE, 0)
        row[mode] = dict(compress_gbs=round(raw / dt / 1e9, 2), compress_ms=round(dt * 1e3, 2), decompress_gbs=round(raw / ddt / 1e9, 2),
                         decompress_ms=round(ddt * 1e3, 2), stored_over_src=round(stored / raw, 5), one_task_stages_ms=stages)
        del d_dst, d_back
    # the kernel's own rate: 1 GiB (8 partitions of 128 MiB) through codec NONE with the layer on, checksums off
    big = torch.randint(0, 256, (1 << 30,), dtype=torch.uint8, device=dev)
    offs = np.arange(9, dtype=np.int64) * (128 << 20)
    out = torch.empty((1 << 30) + 16 * 8 + 64, dtype=torch.uint8, device=dev)
    c.set_option(OPT_PROFILE, 1)
    ms = []
    for _ in range(4):
        c.set_stream_ivs(ivs[: 16 * 8])
        c.compress_map_output_device(s3shuffle.CODEC_NONE, s3shuffle.CHECKSUM_NONE, big.data_ptr(), offs, out.data_ptr(), out.numel())
        ms.append(c.stage_ms(2))
    row["kernel_1gib_ms"] = [round(x, 3) for x in ms]
    row["kernel_1gib_gbs"] = round((1 << 30) / (min(ms[1:]) * 1e-3) / 1e9, 1)
    c.set_option(OPT_PROFILE, 0)
    c.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--inputs", default="terasort,wide")
    ap.add_argument("--cpu-procs", type=int, default=16, help="0: no host leg")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    ap.add_argument("--gpu-step", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpu_step:
        gpu_step(args.gpu_step, args)
        return 0
    lines, rows = [], []
    host = host_leg(args.cpu_procs, 256) if args.cpu_procs > 0 else None
    if host:
        lines.append("host: %s: %.2f GB/s" % (host["leg"], host["gbs"]))
        print(lines[-1], flush=True)
    for name in args.inputs.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--gpu-step", name, "--maps", str(args.maps),
               "--steps", str(args.steps), "--mib", str(args.mib)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print("GPU step %s ended with status %d; nothing more is started\n%s" % (name, r.returncode, r.stderr[-3000:]), flush=True)
            return 1
        for ln in r.stdout.splitlines():
            if not ln.startswith("ROW "):
                continue
            row = json.loads(ln[4:])
            row["host"] = host
            for mode in ("off", "on"):
                m = row[mode]
                lines.append(f"{name:9s} layer {mode:3s}: compress + Adler32 {m['compress_gbs']:6.2f} GB/s ({m['compress_ms']:.1f} ms), verify + decompress "
                             f"{m['decompress_gbs']:6.2f} GB/s ({m['decompress_ms']:.1f} ms) of source bytes, {row['maps']} x {row['mib']} MiB; stored / source "
                             f"{m['stored_over_src']:.4f}; one task alone, ms: {m['one_task_stages_ms']}")
                print(lines[-1], flush=True)
            lines.append(f"{name:9s} AES-CTR kernel alone over 1 GiB (codec NONE, HIP events on s3s_stream): {row['kernel_1gib_gbs']:.1f} GB/s, ms per call {row['kernel_1gib_ms']}")
            print(lines[-1], flush=True)
            rows.append(row)
    if args.out:
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
