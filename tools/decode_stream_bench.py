"""(GPU) what the streaming reduce side (s3s_dstream_*) costs next to the one-shot call: one 128 MiB map output resident in
HBM (TeraSort rows in 200 partitions as LZ4 + CRC32, wide rows in 64 partitions as Snappy + CRC32), verify + decompress of
the whole range

  one-shot      s3s_decompress_range_device, this library
  parent        the same call on another build of the library (--parent-lib: the parent commit's), in alternation with this
                one in the same run - the default path did not move, so the two must agree within the run-to-run spread
  stream-whole  ONE feed over the whole range (what the stream-mode discovery, the capacity cut and the seeded checksum add)
  stream-64m / -16m / -4m   feeds of at most that many compressed bytes; the destination holds 8 x the window (the images
                compress 4 - 5 x, so the window ends a feed, not the capacity) and is reused
  one-shot-4m   the floor of a CALL, for the row above it: one-shot calls over sub-ranges of whole partitions of at most
                4 MiB compressed each (what a caller can do today where the partitions are small)
  host-64m / -16m   s3s_dstream_feed on page-locked host buffers, the shape of the Scala stream: ONE compressed and ONE
                decoded buffer of that size, so the capacity ends most feeds; upload, decode and download of a feed do not overlap
  enc-one-shot / enc-stream-whole / enc-stream-16m / -4m / enc-host-64m   the same range stored under IO encryption (AES-128,
                written by this library's map side): the one-shot encrypted call and s3s_dstream_open_encrypted with the inputs
                and windows of the rows above, in the same process - against the plain rows, the layer's cost per feed

Times are a host clock around calls that end in a stream synchronise; every figure is the median of --steps calls after
--warmup, with the fastest and slowest beside it.  The comparison is between the rows, never against a target.

This process never opens the GPU: every (library, input) pair is one GPU step, a child process of its own under `timeout`,
one after the other, this library and the parent's alternating (--rounds times); the first step that fails ends the run.

usage: python tools/decode_stream_bench.py [--parent-lib PATH] [--steps 20] [--warmup 3] [--mib 128] [--rounds 2]
                                           [--inputs terasort,wide] [--step-timeout 240] [--out profiles/decode_stream_tool.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))

LZ4, SNAPPY, CRC = 1, 2, 2
WINDOWS = (("stream-64m", 64 << 20), ("stream-16m", 16 << 20), ("stream-4m", 4 << 20))


def make(name, mib):
    from s3shuffle import datagen

    return ((LZ4,) + datagen.terasort_map_output(mib << 20, 200, seed=2, map_id=0) if name == "terasort"
            else (SNAPPY,) + datagen.tpcds_wide_map_output(mib << 20, 64, seed=3, map_id=0))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def gpu_step(name, args):
    """One input on the library S3S_CODEC_LIB names (this process opens the GPU).  Prints one JSON row per mode."""
    import numpy as np
    import torch

    import s3shuffle

    dev = torch.device("cuda", 0)
    c = s3shuffle.Codec(0)
    codec, data, offs = make(name, args.mib)
    img, index, sums = c.compress_map_output(codec, CRC, data, offs)
    total, decoded = int(index[-1]), int(data.size)
    d_img = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    d_out = torch.empty(decoded + 4096, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    streams = hasattr(c._lib, "s3s_dstream_open")

    def row(mode, ts, feeds=1):
        med = statistics.median(ts)
        print(json.dumps(dict(input=name, lib=args.label, mode=mode, comp_bytes=total, decoded_bytes=decoded, feeds=feeds, steps=len(ts),
                              median_ms=round(med * 1e3, 4), min_ms=round(min(ts) * 1e3, 4), max_ms=round(max(ts) * 1e3, 4),
                              decoded_gbs=round(decoded / med / 1e9, 2))), flush=True)

    def one_shot():
        assert c.decompress_range_device(codec, CRC, d_img.data_ptr(), total, index, sums, d_out.data_ptr(), decoded) == decoded

    one_shot()
    want = d_out[:decoded].cpu().numpy().copy()
    assert np.array_equal(want, data), "one-shot decode differs from the source"
    row("one-shot", timed(one_shot, args.steps, args.warmup))
    if not streams:
        return

    def stream(window, cap, check=False):
        feeds, n_out = 0, 0
        with s3shuffle.DecodeStream(c, codec, CRC, index, sums) as s:
            while True:
                pos = s.position
                r = s.feed_device(d_img.data_ptr() + pos, min(window, total - pos), d_out.data_ptr(), cap)
                assert r.code == 0 and (r.consumed > 0 or r.at_end), (r.code, pos, r.need_comp, r.need_dst)
                if check and r.out_len:
                    assert np.array_equal(d_out[:r.out_len].cpu().numpy(), want[n_out:n_out + r.out_len]), "stream output differs"
                feeds, n_out = feeds + 1, n_out + r.out_len
                if r.at_end:
                    break
        assert n_out == decoded
        return feeds

    feeds = stream(total, decoded, check=True)
    row("stream-whole", timed(lambda: stream(total, decoded), args.steps, args.warmup), feeds)
    for mode, window in WINDOWS:
        cap = min(8 * window, decoded)
        feeds = stream(window, cap, check=True)
        row(mode, timed(lambda: stream(window, cap), args.steps, args.warmup), feeds)

    # the same range stored under IO encryption (AES-128): the one-shot encrypted call, then s3s_dstream_open_encrypted with the
    # windows above, in the same process as the plain legs - the difference is the layer's cost per feed
    if hasattr(c._lib, "s3s_dstream_open_encrypted"):
        c.set_io_encryption(bytes(range(16)))
        try:
            c.set_stream_ivs(np.random.default_rng(11).integers(0, 256, 16 * (len(offs) - 1), dtype=np.uint8))
            e_img, e_index, e_sums = c.compress_map_output(codec, CRC, data, offs)
            e_total = int(e_index[-1])
            d_enc = torch.from_numpy(np.ascontiguousarray(e_img)).to(dev)
            torch.cuda.synchronize()

            def enc_one_shot():
                assert c.decompress_range_device(codec, CRC, d_enc.data_ptr(), e_total, e_index, e_sums, d_out.data_ptr(), decoded) == decoded

            def enc_stream(window, cap, check=False):
                feeds, n_out = 0, 0
                with s3shuffle.DecodeStream(c, codec, CRC, e_index, e_sums, encrypted=True) as s:
                    while True:
                        pos = s.position
                        r = s.feed_device(d_enc.data_ptr() + pos, min(window, e_total - pos), d_out.data_ptr(), cap)
                        assert r.code == 0 and (r.consumed > 0 or r.at_end), (r.code, pos, r.need_comp, r.need_dst)
                        if check and r.out_len:
                            assert np.array_equal(d_out[:r.out_len].cpu().numpy(), want[n_out:n_out + r.out_len]), "encrypted stream output differs"
                        feeds, n_out = feeds + 1, n_out + r.out_len
                        if r.at_end:
                            break
                assert n_out == decoded
                return feeds

            enc_one_shot()
            assert np.array_equal(d_out[:decoded].cpu().numpy(), want), "one-shot encrypted decode differs from the source"
            row("enc-one-shot", timed(enc_one_shot, args.steps, args.warmup))
            feeds = enc_stream(e_total, decoded, check=True)
            row("enc-stream-whole", timed(lambda: enc_stream(e_total, decoded), args.steps, args.warmup), feeds)
            for mode, window in WINDOWS[1:]:
                cap = min(8 * window, decoded)
                feeds = enc_stream(window, cap, check=True)
                row("enc-" + mode, timed(lambda: enc_stream(window, cap), args.steps, args.warmup), feeds)
            h_comp, h_out = s3shuffle.PinnedBuffer(e_total), s3shuffle.PinnedBuffer(64 << 20)
            h_comp.array[:e_total] = e_img

            def enc_host_stream():
                feeds, n_out = 0, 0
                with s3shuffle.DecodeStream(c, codec, CRC, e_index, e_sums, encrypted=True) as s:
                    while True:
                        pos = s.position
                        r = s.feed(h_comp.array[pos:min(pos + (64 << 20), e_total)], h_out.array)
                        assert r.code == 0 and (r.consumed > 0 or r.at_end), (r.code, pos, r.need_comp, r.need_dst)
                        feeds, n_out = feeds + 1, n_out + r.out_len
                        if r.at_end:
                            break
                assert n_out == decoded
                return feeds

            feeds = enc_host_stream()
            row("enc-host-64m", timed(enc_host_stream, max(args.steps // 2, 1), 1), feeds)
            h_comp.free()
            h_out.free()
        finally:
            c.set_io_encryption(None)

    # sub-ranges of whole partitions, at most 4 MiB compressed each, one one-shot call per sub-range
    subs, r0 = [], 0
    for p in range(1, len(index)):
        if p == len(index) - 1 or int(index[p + 1] - index[r0]) > (4 << 20):
            subs.append((r0, p))
            r0 = p

    def sub_ranges():
        for a, b in subs:
            n = c.decompress_range_device(codec, CRC, d_img.data_ptr() + int(index[a]), int(index[b] - index[a]), index[a:b + 1] - index[a],
                                          sums[a:b], d_out.data_ptr(), decoded)
            assert n == int(offs[b] - offs[a])

    row("one-shot-4m", timed(sub_ranges, args.steps, args.warmup), len(subs))

    for mode, window in (("host-64m", 64 << 20), ("host-16m", 16 << 20)):
        h_comp, h_out = s3shuffle.PinnedBuffer(max(total, 1)), s3shuffle.PinnedBuffer(window)
        h_comp.array[:total] = img

        def host_stream(check=False):
            feeds, n_out = 0, 0
            with s3shuffle.DecodeStream(c, codec, CRC, index, sums) as s:
                while True:
                    pos = s.position
                    r = s.feed(h_comp.array[pos:min(pos + window, total)], h_out.array)
                    assert r.code == 0 and (r.consumed > 0 or r.at_end), (r.code, pos, r.need_comp, r.need_dst)
                    if check and r.out_len:
                        assert np.array_equal(h_out.array[:r.out_len], want[n_out:n_out + r.out_len]), "host stream output differs"
                    feeds, n_out = feeds + 1, n_out + r.out_len
                    if r.at_end:
                        break
            assert n_out == decoded
            return feeds

        feeds = host_stream(check=True)
        row(mode, timed(host_stream, max(args.steps // 2, 1), 1), feeds)
        h_comp.free()
        h_out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=20)
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
    for name in args.inputs.split(","):
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
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
