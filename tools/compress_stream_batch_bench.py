"""(GPU) what the batched feed of the streaming map side (s3s_cstream_feed_batch_device) saves: S streams with one window each
per round, the shape of an executor whose map tasks each write through a buffer of spark.shuffle.s3.bufferSize.  Inputs: one
map output of --mib + 1 MiB resident in HBM (TeraSort rows in 200 partitions as LZ4 + Adler32, wide rows in 64 partitions as Snappy + Adler32).
Window g of a row is the source bytes [g W, g W + W) of that map output, presented as the first window of a fresh stream with
the partition ends that lie in it; every window has a destination of its own of s3s_cstream_feed_bound bytes.  Neither the
windows nor the destinations overlap.

  rows       S = 8 x 4 MiB, S = 16 x 8 MiB, S = 16 x 1 MiB
  (a) single   the S windows fed one after another through s3s_cstream_feed_device on one context
  (b) batch    ONE s3s_cstream_feed_batch_device per round (it must report S entries under option key 18)
  (c) tasks    s3s_compress_map_outputs_batch_device over the same bytes as S map tasks: the ceiling the batch cannot beat

Times are a host clock around calls that end in a stream synchronise.  The legs of a row alternate inside ONE process: every
step runs each leg once, in order; every figure is the median of --steps such steps after --warmup, with the fastest and
slowest beside it.  The streams of a step are opened before the clock starts (host-only work, the same for (a) and (b)).
Before anything is timed the batched call's bytes, lengths and checksums are compared with the single feeds'.

With --parent-lib the run alternates between this library and the parent's, --rounds times each: the parent's process runs
(a) and (c) (it has no batched feed), and the table's (a) is the parent's, with the spread of all its medians beside it.

This process never opens the GPU: every (library, input) pair is one GPU step, a child process of its own under `timeout`,
one after the other; the first step that fails ends the run.

usage: python tools/compress_stream_batch_bench.py [--parent-lib PATH] [--steps 10] [--warmup 3] [--mib 128] [--rounds 2]
                                                   [--inputs terasort,wide] [--step-timeout 240] [--out profiles/compress_stream_batch.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))

LZ4, SNAPPY, ADLER = 1, 2, 1
OPT_BATCH_ENTRIES = 18
ROWS = ((8, 4 << 20), (16, 8 << 20), (16, 1 << 20))


def make(name, mib):
    from s3shuffle import datagen

    if name == "terasort":
        data, offs = datagen.terasort_map_output((mib + 1) << 20, 200, seed=2, map_id=0)  # (a MiB more: 16 windows of 8 MiB fit)
        return LZ4, data, offs
    data, offs = datagen.tpcds_wide_map_output((mib + 1) << 20, 64, seed=3)
    return SNAPPY, data, offs


def gpu_step(name, args):
    """One input on the library S3S_CODEC_LIB names (this process opens the GPU).  Prints one JSON row per row and leg."""
    import numpy as np
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    c = s3shuffle.Codec(0)
    codec, data, offs = make(name, args.mib)
    offs = [int(x) for x in offs]
    total = int(data.size)
    d_src = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    has_batch = hasattr(c._lib, "s3s_cstream_feed_batch_device")
    probe = c.compress_stream(codec, ADLER)
    for S, W in ROWS:
        if S * W > total:
            continue
        ends = [[e - g * W for e in offs[1:] if g * W < e <= g * W + W] for g in range(S)]
        caps = [probe.feed_bound(W, len(e)) for e in ends]
        at = [0]
        for cap in caps:
            at.append(at[-1] + ((cap + 255) & ~255))
        d_dst = torch.empty(at[-1] + 4096, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        src_of = [d_src.data_ptr() + g * W for g in range(S)]
        dst_of = [d_dst.data_ptr() + at[g] for g in range(S)]

        def open_all():
            return [c.compress_stream(codec, ADLER) for _ in range(S)]

        def close_all(streams):
            for s in streams:
                s.close(check=False)  # (a window's last partition stays open)

        def single(streams):
            out = [s.feed_device(src_of[g], W, ends[g], dst_of[g], caps[g]) for g, s in enumerate(streams)]
            close_all(streams)
            return out

        def batch(streams):
            out = c.compress_stream_feed_batch([(s, src_of[g], W, ends[g], dst_of[g], caps[g]) for g, s in enumerate(streams)])
            assert c.last_compress_batch_code == 0 and c.get_option(OPT_BATCH_ENTRIES) == S
            close_all(streams)
            return out

        tasks = [(src_of[g], [0] + ends[g] + ([W] if not ends[g] or ends[g][-1] < W else []), dst_of[g], ((caps[g] + 255) & ~255)) for g in range(S)]

        def ceiling(_):
            return c.compress_map_outputs_batch_device(codec, ADLER, tasks)

        def snapshot(results):
            img = d_dst[:at[-1]].cpu().numpy()
            rows = [(r.code, r.consumed, r.out_len, r.parts_closed, [int(x) for x in r.lengths], [int(x) for x in r.checksums],
                     img[at[g]:at[g] + r.out_len].copy()) for g, r in enumerate(results)]
            d_dst.zero_()
            torch.cuda.synchronize()
            return rows

        want = snapshot(single(open_all()))
        assert all(r[0] == 0 and r[1] > 0 for r in want)
        legs = [("single", single, open_all)]
        if has_batch:
            got = snapshot(batch(open_all()))
            for g, (a, b) in enumerate(zip(want, got)):
                assert a[:6] == b[:6] and np.array_equal(a[6], b[6]), "window %d: the batched feed differs from the single feed" % g
            legs.append(("batch", batch, open_all))
        legs.append(("tasks", ceiling, lambda: None))
        times = {mode: [] for mode, _, _ in legs}
        for step in range(args.warmup + args.steps):
            for mode, fn, prepare in legs:
                state = prepare()
                t0 = time.perf_counter()
                fn(state)
                dt = time.perf_counter() - t0
                if step >= args.warmup:
                    times[mode].append(dt)
        for mode, _, _ in legs:
            ts = times[mode]
            med = statistics.median(ts)
            print(json.dumps(dict(input=name, lib=args.label, mode=mode, streams=S, window=W, src_bytes=sum(r[1] for r in want),
                                  image_bytes=sum(r[2] for r in want), steps=len(ts), median_ms=round(med * 1e3, 4),
                                  min_ms=round(min(ts) * 1e3, 4), max_ms=round(max(ts) * 1e3, 4))), flush=True)
    probe.close()
    c.close()


def table(rows, inputs, with_parent):
    """-> the markdown of profiles/compress_stream_batch.md"""
    def pick(name, mode, lib, S, W):
        return [r for r in rows if r["input"] == name and r["mode"] == mode and r["lib"].startswith(lib) and (r["streams"], r["window"]) == (S, W)]

    def cell(rs):
        return " / ".join("%.4f (%.3f – %.3f)" % (r["median_ms"], r["min_ms"], r["max_ms"]) for r in rs) or "not measured"

    mean = lambda rs: sum(r["median_ms"] for r in rs) / len(rs)  # noqa: E731
    base = "parent" if with_parent else "this"
    out = ["# The batched feed of the map side: S streams, one window each per call", "",
           "Written by `tools/compress_stream_batch_bench.py` (its docstring says what a row is).  Milliseconds per round of S windows: median",
           "(fastest – slowest) of the recorded steps, one cell per process of the run (the libraries alternate).  (a) is %s library's;" % ("the parent commit's" if with_parent else "this"),
           "ratios and GB/s (source bytes consumed per second) use the mean of the cells' medians; the spread of (a) is the largest minus the",
           "smallest of ALL medians of S single feeds in the run, on either library.", ""]
    for name in inputs:
        out += ["## %s" % name, "", "| S x window | source MiB consumed | (a) S single feeds | (b) one batched feed | (c) one-shot batch of S tasks | spread of (a) ms | (a) - (b) ms | (b)/(a) | (b)/(c) | (b) GB/s |",
                "|---|---|---|---|---|---|---|---|---|---|"]
        for S, W in ROWS:
            a, b, c = pick(name, "single", base, S, W), pick(name, "batch", "this", S, W), pick(name, "tasks", "this", S, W)
            if not (a and b and c):
                continue
            every_a = [r["median_ms"] for r in pick(name, "single", "", S, W)]
            out.append("| %d x %d MiB | %.1f | %s | %s | %s | %.4f | %.4f | %.3f | %.3f | %.1f |" % (
                S, W >> 20, b[0]["src_bytes"] / 2**20, cell(a), cell(b), cell(c), max(every_a) - min(every_a), mean(a) - mean(b), mean(b) / mean(a),
                mean(b) / mean(c), b[0]["src_bytes"] / mean(b) / 1e6))
        if with_parent:
            out += ["", "| paths this change shares with the parent | this commit | parent commit |", "|---|---|---|"]
            for S, W in ROWS:
                for mode, what in (("single", "S single feeds"), ("tasks", "one-shot batch of S tasks")):
                    out.append("| %s, %d x %d MiB | %s | %s |" % (what, S, W >> 20, cell(pick(name, mode, "this", S, W)), cell(pick(name, mode, "parent", S, W))))
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--inputs", default="terasort,wide")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    if args.child:
        gpu_step(args.child, args)
        return 0
    rows = []
    libs = [("this", None)] + ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    inputs = args.inputs.split(",")
    for name in inputs:
        for rnd in range(args.rounds):
            for label, path in libs:
                env = dict(os.environ)
                if path:
                    env["S3S_CODEC_LIB"] = path
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--label",
                       "%s#%d" % (label, rnd), "--steps", str(args.steps), "--warmup", str(args.warmup), "--mib", str(args.mib)]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if r.returncode != 0:  # a failed step ends the run: nothing more is started on the GPU
                    sys.stderr.write(r.stderr[-4000:])
                    print(json.dumps(dict(failed="%s %s" % (label, name), returncode=r.returncode)))
                    return 1
                rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(table(rows, inputs, bool(args.parent_lib)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
