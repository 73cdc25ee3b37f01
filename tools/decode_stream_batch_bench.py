"""(GPU) what the batched feed (s3s_dstream_feed_batch_device) saves: S streams with one window each per round, the shape of
the reference's reduce task (S3BufferedPrefetchIterator: up to 10 fetches open, 8 MiB buffers, 128 MiB in all).  Inputs are
those of tools/decode_stream_bench.py: one 128 MiB map output resident in HBM (TeraSort rows in 200 partitions as LZ4 + CRC32,
wide rows in 64 partitions as Snappy + CRC32).  A stream's range is a run of whole partitions of the image of at most W
compressed bytes (the runs start at evenly spaced partitions and may share source bytes - they are only read - each has a
destination of its own), and its one window is that whole range, so every feed takes everything and ends at_end.

  rows       S = 8 x 4 MiB, S = 16 x 8 MiB (the reference's budget), S = 16 x 1 MiB
  (a) single   the S windows fed one by one through s3s_dstream_feed_device, in the same process: unchanged code, the parent's
  (b) batch    ONE s3s_dstream_feed_batch_device per round
  (c) ranges   s3s_decompress_ranges_batch_device over the same S ranges (they are cut at partition boundaries): the ceiling
  defaults   rows (1) and (3) of profiles/decode_stream.md - the one-shot call and one stream feed over the whole range - on this
             library and on --parent-lib, in alternation: the default paths did not move
  encrypted  (--enc-rows, on by default) the same rows over the same partitions written under IO encryption (AES-128, the
             library's own map side): S streams of s3s_dstream_open_encrypted.
             (a) enc-call on --parent-lib: ONE s3s_dstream_feed_batch_device, which that library answers with S single feeds
             (b) enc-call on this library: the same call, batched (it must report S entries under option key 17)
             (c) the plain batched row above, on the same partitions unencrypted: (b) - (c) is what the layer costs, held
                 against one decrypt pass over the stored bytes
             enc-single on either library: S s3s_dstream_feed_device calls; one of them, and the plain batched row, on both
             libraries in alternation: the paths this change does not touch did not move

Times are a host clock around calls that end in a stream synchronise; every figure is the median of --steps calls after
--warmup with the fastest and slowest beside it.  The streams of a call are opened before the clock starts (host-only work,
the same for (a) and (b)).

This process never opens the GPU: every (library, input) pair is one GPU step, a child process of its own under `timeout`,
one after the other; the first step that fails ends the run.

usage: python tools/decode_stream_batch_bench.py [--parent-lib PATH] [--steps 10] [--warmup 3] [--mib 128] [--rounds 2] [--enc-rows 1]
                                                 [--inputs terasort,wide] [--step-timeout 240] [--out profiles/decode_stream_batch.md]"""
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

CRC = 2
OPT_BATCH_ENTRIES = 17
ENC_KEY = bytes(range(16))
ROWS = ((8, 4 << 20), (16, 8 << 20), (16, 1 << 20))


def gpu_step(name, args):
    """One input on the library S3S_CODEC_LIB names (this process opens the GPU).  Prints one JSON row per mode."""
    import numpy as np
    import torch

    import s3shuffle
    from decode_stream_bench import make

    dev = torch.device("cuda", 0)
    c = s3shuffle.Codec(0)
    codec, data, offs = make(name, args.mib)
    img, index, sums = c.compress_map_output(codec, CRC, data, offs)
    index, sums, offs = np.asarray(index, np.int64), np.asarray(sums, np.int64), np.asarray(offs, np.int64)
    total, decoded, nparts = int(index[-1]), int(data.size), len(index) - 1
    d_img = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    d_out = torch.empty(decoded + 4096, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def row(mode, ts, **more):
        med = statistics.median(ts)
        print(json.dumps(dict(input=name, lib=args.label, mode=mode, steps=len(ts), median_ms=round(med * 1e3, 4), min_ms=round(min(ts) * 1e3, 4),
                              max_ms=round(max(ts) * 1e3, 4), **more)), flush=True)

    def clock(fn, prepare=lambda: None):
        ts = []
        for k in range(args.warmup + args.steps):
            state = prepare()
            t0 = time.perf_counter()
            fn(state)
            if k >= args.warmup:
                ts.append(time.perf_counter() - t0)
        return ts

    # ---- rows (1) and (3) of profiles/decode_stream.md
    def one_shot(_):
        assert c.decompress_range_device(codec, CRC, d_img.data_ptr(), total, index, sums, d_out.data_ptr(), decoded) == decoded

    one_shot(None)
    assert np.array_equal(d_out[:decoded].cpu().numpy(), data), "one-shot decode differs from the source"
    row("one-shot", clock(one_shot), decoded_bytes=decoded)

    def whole(s):
        r = s.feed_device(d_img.data_ptr(), total, d_out.data_ptr(), decoded)
        assert r.code == 0 and r.at_end == 1 and r.out_len == decoded
        s.close()

    row("stream-whole", clock(whole, lambda: s3shuffle.DecodeStream(c, codec, CRC, index, sums)), decoded_bytes=decoded)
    if not (args.batch_rows or args.enc_rows) or not hasattr(c._lib, "s3s_dstream_feed_batch_device"):
        return
    if args.enc_rows:  # the same partitions under the layer: IV | cipher text per non-empty partition
        c.set_io_encryption(ENC_KEY)
        c.set_stream_ivs(np.random.default_rng(17).integers(0, 256, 16 * nparts, dtype=np.uint8))
        eimg, eindex, esums = c.compress_map_output(codec, CRC, data, offs)
        c.set_io_encryption(None)
        eindex, esums = np.asarray(eindex, np.int64), np.asarray(esums, np.int64)
        d_eimg = torch.from_numpy(np.ascontiguousarray(eimg)).to(dev)
        has_key = c._lib.s3s_get_option(c._h, OPT_BATCH_ENTRIES) >= 0

    # ---- the batched rows
    for S, W in ROWS:
        # run g: whole partitions from a[g] on while they stay inside W compressed bytes
        last = max(p for p in range(nparts) if total - int(index[p]) >= min(W, total))
        runs = []
        for g in range(S):
            a = (g * last) // max(S - 1, 1)
            b = a + 1
            while b < nparts and int(index[b + 1] - index[a]) <= W:
                b += 1
            runs.append((a, b))
        comp_bytes = sum(int(index[b] - index[a]) for a, b in runs)
        out_bytes = sum(int(offs[b] - offs[a]) for a, b in runs)
        d_dst = torch.empty(out_bytes + 4096, dtype=torch.uint8, device=dev)
        dst_at, at = [], 0
        for a, b in runs:
            dst_at.append(d_dst.data_ptr() + at)
            at += int(offs[b] - offs[a])

        def open_all():
            return [s3shuffle.DecodeStream(c, codec, CRC, index[a:b + 1] - index[a], sums[a:b]) for a, b in runs]

        def entries(streams):
            return [(s, d_img.data_ptr() + int(index[a]), int(index[b] - index[a]), dst_at[g], int(offs[b] - offs[a]))
                    for g, (s, (a, b)) in enumerate(zip(streams, runs))]

        def close_all(streams):
            for s in streams:
                s.close()

        def single(streams):
            for s, d_comp, n, d, cap in entries(streams):
                r = s.feed_device(d_comp, n, d, cap)
                assert r.code == 0 and r.at_end == 1 and r.out_len == cap
            close_all(streams)

        def batch(streams):
            got = c.feed_streams_device(entries(streams))
            assert all(code == 0 and r.at_end == 1 for code, r in got), [code for code, _ in got]
            close_all(streams)

        ranges = [(d_img.data_ptr() + int(index[a]), int(index[b] - index[a]), index[a:b + 1] - index[a], sums[a:b], dst_at[g], int(offs[b] - offs[a]))
                  for g, (a, b) in enumerate(runs)]

        def ceiling(_):
            got = c.decompress_ranges_batch_device(codec, CRC, ranges)
            assert all(st == 0 for st, _, _ in got)

        def check(what):
            got = d_dst[:out_bytes].cpu().numpy()
            at = 0
            for a, b in runs:
                n = int(offs[b] - offs[a])
                assert np.array_equal(got[at:at + n], data[int(offs[a]):int(offs[b])]), "%s: output differs from the source" % what
                at += n
            d_dst.zero_()
            torch.cuda.synchronize()

        more = dict(streams=S, window=W, comp_bytes=comp_bytes, decoded_bytes=out_bytes)
        plain_modes = (("single", single, open_all), ("batch", batch, open_all), ("ranges", ceiling, lambda: None))
        for mode, fn, prep in plain_modes if args.batch_rows else plain_modes[1:2]:  # (the plain batched row is a default path of the encrypted rows)
            fn(prep())
            check(mode)
            row(mode, clock(fn, prep), **more)
        if not args.enc_rows:
            continue

        # ---- the same partitions, encrypted
        def enc_open_all():
            return [s3shuffle.DecodeStream(c, codec, CRC, eindex[a:b + 1] - eindex[a], esums[a:b], encrypted=True) for a, b in runs]

        def enc_entries(streams):
            return [(s, d_eimg.data_ptr() + int(eindex[a]), int(eindex[b] - eindex[a]), dst_at[g], int(offs[b] - offs[a]))
                    for g, (s, (a, b)) in enumerate(zip(streams, runs))]

        def enc_single(streams):
            for s, d_comp, n, d, cap in enc_entries(streams):
                r = s.feed_device(d_comp, n, d, cap)
                assert r.code == 0 and r.at_end == 1 and r.out_len == cap
            close_all(streams)

        def enc_call(streams):
            got = c.feed_streams_device(enc_entries(streams))
            assert all(code == 0 and r.at_end == 1 for code, r in got), [code for code, _ in got]
            if has_key:  # this library: the call must have been batched
                assert c._lib.s3s_get_option(c._h, OPT_BATCH_ENTRIES) == S
            close_all(streams)

        emore = dict(more, comp_bytes=sum(int(eindex[b] - eindex[a]) for a, b in runs), batched=bool(has_key))
        c.set_io_encryption(ENC_KEY)
        try:
            for mode, fn in (("enc-single", enc_single), ("enc-call", enc_call)):
                fn(enc_open_all())
                check(mode)
                row(mode, clock(fn, enc_open_all), **emore)
        finally:
            c.set_io_encryption(None)


def table(rows, inputs):
    """-> the markdown of profiles/decode_stream_batch.md"""
    def pick(name, mode, lib, S=None, W=None):
        return [r for r in rows if r["input"] == name and r["mode"] == mode and r["lib"].startswith(lib) and (S is None or (r["streams"], r["window"]) == (S, W))]

    def cell(r):
        return "%.4f (%.3f – %.3f)" % (r["median_ms"], r["min_ms"], r["max_ms"])

    out = ["# The batched feed: S streams, one window each per call", "",
           "Written by `tools/decode_stream_batch_bench.py` (its docstring says what a row is).  Milliseconds per round of S windows, median",
           "(fastest – slowest) of the recorded calls; GB/s are decoded bytes per second of the median.", ""]
    for name in inputs:
        out += ["## %s" % name, "", "| S x window | compressed / decoded MiB | (a) S single feeds | (b) one batched feed | (c) one-shot ranges batch | (b)/(a) | (b)/(c) | (b) GB/s |",
                "|---|---|---|---|---|---|---|---|"]
        for S, W in ROWS:
            a, b, c = (pick(name, m, "this#0", S, W) for m in ("single", "batch", "ranges"))
            if not (a and b and c):
                continue
            a, b, c = a[0], b[0], c[0]
            out.append("| %d x %d MiB | %.1f / %.1f | %s | %s | %s | %.2f | %.2f | %.0f |" % (
                S, W >> 20, a["comp_bytes"] / 2**20, a["decoded_bytes"] / 2**20, cell(a), cell(b), cell(c), b["median_ms"] / a["median_ms"],
                b["median_ms"] / c["median_ms"], b["decoded_bytes"] / b["median_ms"] / 1e6))
        enc = [(S, W, pick(name, "enc-call", "parent", S, W), pick(name, "enc-call", "this", S, W), pick(name, "batch", "this", S, W)) for S, W in ROWS]
        if any(b for _, _, _, b, _ in enc):
            out += ["", "Encrypted (AES-128), the same partitions: (a) one call on the parent's library = S single encrypted feeds, (b) one batched call on this",
                    "commit, (c) the plain batched feed over the same partitions unencrypted.  One cell per round of the run (the libraries alternate);",
                    "the ratios use the mean of the rounds' medians.  The last column is the stored bytes over (b) - (c): what one decrypt pass would have to run at.", "",
                    "| S x window | stored MiB | (a) parent: S single feeds | (b) this: one batched feed | (c) plain batched feed | (b)/(a) | (b) - (c) ms | stored bytes / ((b) - (c)) GB/s |",
                    "|---|---|---|---|---|---|---|---|"]
            for S, W, a, b, c in enc:
                if not (b and c):
                    continue
                mean = lambda rs: sum(r["median_ms"] for r in rs) / len(rs)  # noqa: E731
                d = mean(b) - mean(c)
                out.append("| %d x %d MiB | %.1f | %s | %s | %s | %s | %.4f | %s |" % (
                    S, W >> 20, b[0]["comp_bytes"] / 2**20, " / ".join(cell(r) for r in a) or "not measured", " / ".join(cell(r) for r in b),
                    " / ".join(cell(r) for r in c), "%.2f" % (mean(b) / mean(a)) if a else "-", d, "%.0f" % (b[0]["comp_bytes"] / d / 1e6) if d > 0 else "-"))
            out += ["", "| paths this change does not touch | this commit, per round | parent commit |", "|---|---|---|"]
            for S, W in ROWS:
                for mode, what in (("batch", "plain batched feed"), ("enc-single", "S single encrypted feeds")):
                    out.append("| %s, %d x %d MiB | %s | %s |" % (what, S, W >> 20, " / ".join(cell(r) for r in pick(name, mode, "this", S, W)) or "-",
                                                              " / ".join(cell(r) for r in pick(name, mode, "parent", S, W)) or "not measured"))
        out += ["", "| default path (rows (1) and (3) of `profiles/decode_stream.md`) | this commit, per round of the run | parent commit |", "|---|---|---|"]
        for mode, what in (("one-shot", "one-shot `s3s_decompress_range_device`"), ("stream-whole", "ONE stream feed over the whole range")):
            out.append("| %s | %s | %s |" % (what, " / ".join(cell(r) for r in pick(name, mode, "this")) or "-",
                                            " / ".join(cell(r) for r in pick(name, mode, "parent")) or "not measured"))
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
    ap.add_argument("--batch-rows", type=int, default=0)
    ap.add_argument("--enc-rows", type=int, default=1)
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
                       "%s#%d" % (label, rnd), "--steps", str(args.steps), "--warmup", str(args.warmup), "--mib", str(args.mib),
                       "--batch-rows", "1" if label == "this" and rnd == 0 else "0", "--enc-rows", str(args.enc_rows)]
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
            f.write(table(rows, inputs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
