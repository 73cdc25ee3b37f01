"""(GPU) what ONE encrypt pass for all windows of a batched feed saves under Spark IO encryption: S streams of
s3s_cstream_open_encrypted with one window each per round, AES-128.  Inputs, windows and destinations are those of
tools/compress_stream_batch_bench.py (TeraSort rows in 200 partitions as LZ4 + Adler32, wide rows in 64 partitions as Snappy +
Adler32; window g of a row is the source bytes [g W, g W + W) of the map output, the first window of a fresh stream); every
window's destination has s3s_cstream_feed_bound bytes of the keyed stream.

  rows       S = 8 x 4 MiB, S = 16 x 8 MiB, S = 16 x 1 MiB
  (a) parent   ONE s3s_cstream_feed_batch_device over the S keyed streams on the parent commit's library, which feeds them one by
               one inside the call (key 19 is unknown there)
  (b) batch    the same call on this library (it must report S entries under option key 19, and 0 under key 18)
  (c) plain    the batched feed of S plain streams over the same windows on a context without a key
  (d) tasks    s3s_compress_map_outputs_batch_device over the same bytes as S keyed map tasks

Times are a host clock around calls that end in a stream synchronise.  The legs of a row alternate inside ONE process: every
step runs each leg once, in order; every figure is the median of --steps such steps after --warmup, with the fastest and
slowest beside it.  Streams are opened and the call's IVs are set before the clock starts (host-only work, the same for every
leg).  Before anything is timed the batched call's bytes, lengths and checksums are compared with single keyed feeds'.

With --parent-lib the run alternates between this library and the parent's, --rounds times each; every process runs the keyed
call, (c) and (d).  (b) - (c) is the cost of the pass (and of the IV records in the plan); its GB/s counts the stored bytes.

This process never opens the GPU: every (library, input) pair is one GPU step, a child process of its own under `timeout`,
one after the other; the first step that fails ends the run.

usage: python tools/compress_stream_batch_encrypted_bench.py [--parent-lib PATH] [--steps 10] [--warmup 3] [--mib 128] [--rounds 2]
                                                   [--inputs terasort,wide] [--step-timeout 240] [--out profiles/compress_stream_batch_encrypted.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from compress_stream_batch_bench import ADLER, OPT_BATCH_ENTRIES, ROWS, make  # noqa: E402

OPT_BATCH_ENC_ENTRIES = 19
KEY = bytes(range(16))


def gpu_step(name, args):
    """One input on the library S3S_CODEC_LIB names (this process opens the GPU).  Prints one JSON row per row and leg."""
    import numpy as np
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    ck, cp = s3shuffle.Codec(0), s3shuffle.Codec(0)
    ck.set_io_encryption(KEY)
    codec, data, offs = make(name, args.mib)
    offs = [int(x) for x in offs]
    total = int(data.size)
    d_src = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    has_key19 = ck.get_option(OPT_BATCH_ENC_ENTRIES) >= 0
    probe = ck.compress_stream(codec, ADLER, encrypted=True)
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
        rng = np.random.default_rng(S)
        feed_ivs = [rng.integers(0, 256, (len(e) + 1, 16), dtype=np.uint8) for e in ends]
        all_ivs = np.concatenate(feed_ivs).reshape(-1)
        tasks = [(src_of[g], [0] + ends[g] + ([W] if not ends[g] or ends[g][-1] < W else []), dst_of[g], ((caps[g] + 255) & ~255)) for g in range(S)]
        task_ivs = np.concatenate([feed_ivs[g][:len(tasks[g][1]) - 1] for g in range(S)]).reshape(-1)

        def open_keyed():
            ck.set_stream_ivs(all_ivs)
            return [ck.compress_stream(codec, ADLER, encrypted=True) for _ in range(S)]

        def open_plain():
            return [cp.compress_stream(codec, ADLER) for _ in range(S)]

        def close_all(streams):
            for s in streams:
                s.close(check=False)  # (a window's last partition stays open)

        def single(_):
            out = []
            for g in range(S):
                s = ck.compress_stream(codec, ADLER, encrypted=True)
                ck.set_stream_ivs(feed_ivs[g].reshape(-1))
                out.append(s.feed_device(src_of[g], W, ends[g], dst_of[g], caps[g]))
                s.close(check=False)
            return out

        def keyed(streams):
            out = ck.compress_stream_feed_batch([(s, src_of[g], W, ends[g], dst_of[g], caps[g]) for g, s in enumerate(streams)])
            assert ck.last_compress_batch_code == 0 and ck.get_option(OPT_BATCH_ENTRIES) == 0
            assert not has_key19 or ck.get_option(OPT_BATCH_ENC_ENTRIES) == S
            close_all(streams)
            return out

        def plain(streams):
            out = cp.compress_stream_feed_batch([(s, src_of[g], W, ends[g], dst_of[g], caps[g]) for g, s in enumerate(streams)])
            assert cp.last_compress_batch_code == 0 and cp.get_option(OPT_BATCH_ENTRIES) == S
            close_all(streams)
            return out

        def set_task_ivs():
            ck.set_stream_ivs(task_ivs)

        def ceiling(_):
            return ck.compress_map_outputs_batch_device(codec, ADLER, tasks)

        def snapshot(results):
            img = d_dst[:at[-1]].cpu().numpy()
            rows = [(r.code, r.consumed, r.out_len, r.parts_closed, [int(x) for x in r.lengths], [int(x) for x in r.checksums],
                     img[at[g]:at[g] + r.out_len].copy()) for g, r in enumerate(results)]
            d_dst.zero_()
            torch.cuda.synchronize()
            return rows

        want = snapshot(single(None))
        assert all(r[0] == 0 and r[1] > 0 for r in want)
        got = snapshot(keyed(open_keyed()))
        for g, (a, b) in enumerate(zip(want, got)):
            assert a[:6] == b[:6] and np.array_equal(a[6], b[6]), "window %d: the batched keyed feed differs from the single keyed feed" % g
        legs = [("keyed", keyed, open_keyed), ("plain", plain, open_plain), ("tasks", ceiling, set_task_ivs)]
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
            print(json.dumps(dict(input=name, lib=args.label, mode=mode, streams=S, window=W, key19=bool(has_key19), src_bytes=sum(r[1] for r in want),
                                  image_bytes=sum(r[2] for r in want), steps=len(ts), median_ms=round(med * 1e3, 4),
                                  min_ms=round(min(ts) * 1e3, 4), max_ms=round(max(ts) * 1e3, 4))), flush=True)
    probe.close()
    ck.close()
    cp.close()


def table(rows, inputs, with_parent):
    """-> the markdown of profiles/compress_stream_batch_encrypted.md"""
    def pick(name, mode, lib, S, W):
        return [r for r in rows if r["input"] == name and r["mode"] == mode and r["lib"].startswith(lib) and (r["streams"], r["window"]) == (S, W)]

    def cell(rs):
        return " / ".join("%.4f (%.3f – %.3f)" % (r["median_ms"], r["min_ms"], r["max_ms"]) for r in rs) or "not measured"

    mean = lambda rs: sum(r["median_ms"] for r in rs) / len(rs)  # noqa: E731
    out = ["# The batched feed of the map side under IO encryption: S keyed streams, one window each per call", "",
           "Written by `tools/compress_stream_batch_encrypted_bench.py` (its docstring says what a row is).  AES-128.  Milliseconds per round of S",
           "windows: median (fastest – slowest) of the recorded steps, one cell per process of the run (the libraries alternate).  (a) is the",
           "parent commit's library, which feeds the keyed streams one by one inside the call; differences, ratios and GB/s use the mean of the",
           "cells' medians; the spread of (a) is the largest minus the smallest of its medians across its processes.  (b) - (c) is the cost",
           "of the pass with the IV records; its GB/s counts stored bytes.  No kernel trace was taken: the pass is not separated from the",
           "other launches of the call.", ""]
    for name in inputs:
        out += ["## %s" % name, "",
                "| S x window | stored MiB | (a) parent: one by one inside the call | (b) this: one batched feed | (c) plain batched feed | (d) one-shot keyed batch of S tasks | spread of (a) ms | (a) - (b) ms | (b)/(a) | (b) - (c) ms | pass GB/s |",
                "|---|---|---|---|---|---|---|---|---|---|---|"]
        for S, W in ROWS:
            a, b = pick(name, "keyed", "parent", S, W), pick(name, "keyed", "this", S, W)
            c, d = pick(name, "plain", "this", S, W), pick(name, "tasks", "this", S, W)
            if not (b and c and d):
                continue
            if a:
                meds = [r["median_ms"] for r in a]
                head = "%s | %s | %s | %s | %.4f | %.4f | %.3f" % (cell(a), cell(b), cell(c), cell(d), max(meds) - min(meds), mean(a) - mean(b), mean(b) / mean(a))
            else:
                head = "not measured | %s | %s | %s | - | - | -" % (cell(b), cell(c), cell(d))
            cost = mean(b) - mean(c)
            out.append("| %d x %d MiB | %.1f | %s | %.4f | %s |" % (S, W >> 20, b[0]["image_bytes"] / 2**20, head, cost,
                                                                 "%.1f" % (b[0]["image_bytes"] / cost / 1e6) if cost > 0 else "-"))
        if with_parent:
            out += ["", "| paths this change shares with the parent | this commit | parent commit |", "|---|---|---|"]
            for S, W in ROWS:
                for mode, what in (("plain", "plain batched feed"), ("tasks", "one-shot keyed batch of S tasks")):
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
