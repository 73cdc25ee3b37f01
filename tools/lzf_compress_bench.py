"""(GPU) map-side LZF compress + Adler32 (S3S_OPT_LZF_COMPRESS = 1, key 10) next to the LZ4 line of the same run: TeraSort map
outputs of 200 partitions and wide rows resident in HBM, the batched device entry point with 2 map tasks per call and 4 calls
in flight like bench.py's headline.  Reports GB/s of SOURCE bytes, output / source, and - from one profiled call on one context
(S3S_OPT_PROFILE) - the stage times.

This process never opens the GPU: every input is one GPU step, a child process of its own under `timeout`, one after the other
(at most one GPU process at a time); the first step that fails ends the run.  The host leg runs before them: liblzf 3.6 through
tests/golden/make_lzf_golden.py --streams on 16 interpreter processes where /opt/conda/bin/python3.9 has imagecodecs (the time
of the same processes over empty input is taken off), otherwise the oracle's greedy encoder on 16 threads, named as such.

usage: python tools/lzf_compress_bench.py [--maps 8] [--steps 5] [--mib 128] [--inputs terasort,wide] [--cpu-threads 16]
                                          [--step-timeout 240] [--out profiles/lzf_compress_tool]"""
import argparse
import json
import os
import struct
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
import numpy as np  # noqa: E402

OPT_PROFILE, OPT_LZF_COMPRESS = 3, 10
CODEC_LZF = 4
LIBLZF_PYTHON = "/opt/conda/bin/python3.9"
LIBLZF_FILTER = os.path.join(ROOT, "tests", "golden", "make_lzf_golden.py")


def make(name, mib, m):
    from s3shuffle import datagen

    return (datagen.terasort_map_output(mib << 20, 200, seed=2, map_id=m) if name == "terasort"
            else datagen.tpcds_wide_map_output(mib << 20, 64, seed=3, map_id=m))


def liblzf_available():
    return os.path.exists(LIBLZF_PYTHON) and subprocess.run([LIBLZF_PYTHON, "-c", "import imagecodecs"], capture_output=True).returncode == 0


def _filter_run(payloads):
    """Wall time of one make_lzf_golden.py --streams process per payload, all started together; -> (seconds, output bytes)."""
    t0 = time.perf_counter()
    procs = [subprocess.Popen([LIBLZF_PYTHON, LIBLZF_FILTER, "--streams"], stdin=subprocess.PIPE, stdout=subprocess.PIPE) for _ in payloads]
    outs = [None] * len(procs)

    def feed(i):
        outs[i] = procs[i].communicate(payloads[i])[0]

    th = [threading.Thread(target=feed, args=(i,)) for i in range(len(procs))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    assert all(p.returncode == 0 for p in procs)
    size = 0
    for o in outs:
        pos = 0
        while pos < len(o):
            (n,) = struct.unpack_from("<Q", o, pos)
            size += n
            pos += 8 + n
    return dt, size


def host_leg(name, mib, workers):
    """-> (label, GB/s of source bytes, output bytes) for one map task on `workers` host processes / threads."""
    data, offs = make(name, mib, 0)
    if liblzf_available():
        parts = [data[offs[p]:offs[p + 1]] for p in range(len(offs) - 1) if offs[p + 1] > offs[p]]
        per = (len(parts) + workers - 1) // workers
        payloads = [b"".join(struct.pack("<Q", q.size) + q.tobytes() for q in parts[i:i + per]) for i in range(0, len(parts), per)]
        idle, _ = _filter_run([b""] * len(payloads))
        dt, size = _filter_run(payloads)
        return "liblzf 3.6 (make_lzf_golden.py --streams) on %d processes, interpreter start taken off" % len(payloads), data.size / max(dt - idle, 1e-6) / 1e9, size
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "lzf_cpu_leg.py"), "--input", name, "--mib", str(mib), "--threads",
                        str(workers)], check=True, capture_output=True, text=True)  # (the oracle is test infrastructure and stays under tests/)
    row = json.loads(r.stdout.strip().splitlines()[-1])
    return "the oracle's greedy encoder (NOT liblzf; tests/tools/lzf_cpu_leg.py) on %d threads" % workers, row["gbs"], row["out_bytes"]


def gpu_step(name, args):
    """One input on the GPU (this process opens it): LZF, then LZ4.  Prints one JSON row per codec."""
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    n_threads = 4
    codecs = [s3shuffle.Codec(0) for _ in range(n_threads)]
    for c in codecs:
        c.set_option(OPT_LZF_COMPRESS, 1)
    outs = [make(name, args.mib, m) for m in range(args.maps)]
    d_src = [torch.from_numpy(d.copy()).to(dev) for d, _ in outs]
    per = args.maps // n_threads
    raw = sum(d.size for d, _ in outs[: per * n_threads])
    for codec_id, label in ((CODEC_LZF, "lzf"), (s3shuffle.CODEC_LZ4, "lz4 32k")):
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
        # stage times: one profiled call of one map task on one context, nothing else in flight
        codecs[0].set_option(OPT_PROFILE, 1)
        codecs[0].compress_map_output_device(codec_id, s3shuffle.CHECKSUM_ADLER32, d_src[0].data_ptr(), outs[0][1], d_dst[0].data_ptr(), caps[0])
        stages = {k: round(codecs[0].stage_ms(v), 3) for k, v in (("total", 0), ("codec", 1), ("assemble", 2), ("checksum", 3), ("hash", 5))}
        codecs[0].set_option(OPT_PROFILE, 0)
        print("ROW " + json.dumps(dict(input=name, codec=label, gbs=round(raw / dt / 1e9, 3), ms=round(dt * 1e3, 2), tasks=per * n_threads, mib=args.mib,
                                       out_over_src=round(sum(totals) / raw, 5), stages_ms=stages)), flush=True)
        del d_dst
    for c in codecs:
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--inputs", default="terasort,wide")
    ap.add_argument("--cpu-threads", type=int, default=16, help="0: no host leg")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    ap.add_argument("--gpu-step", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.gpu_step:
        gpu_step(args.gpu_step, args)
        return 0
    lines, rows = [], []
    host = {}
    if args.cpu_threads > 0:
        for name in args.inputs.split(","):
            label, gbs, size = host_leg(name, args.mib, args.cpu_threads)
            host[name] = dict(leg=label, gbs=round(gbs, 3), out_over_src=round(size / make(name, args.mib, 0)[0].size, 5))
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
            line = (f"{row['input']:9s} {row['codec']:8s}: {row['gbs']:6.2f} GB/s compress + Adler32 of source bytes ({row['ms']:.1f} ms per {row['tasks']} x "
                    f"{row['mib']} MiB), output / source {row['out_over_src']:.4f}; one {row['mib']} MiB task alone, ms: {row['stages_ms']}")
            if row["codec"] == "lzf" and name in host:
                h = host[name]
                row["host"] = h
                line += f"; host: {h['leg']}: {h['gbs']:.2f} GB/s, output / source {h['out_over_src']:.4f}, GPU / host {row['gbs'] / max(h['gbs'], 1e-9):.2f}"
            print(line, flush=True)
            lines.append(line)
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
