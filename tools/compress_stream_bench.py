"""(GPU) what the streaming map side (s3s_cstream_*) costs next to the one-shot call: one 128 MiB TeraSort map output of 200
partitions resident in HBM, compress + checksum of the whole output, LZ4 + Adler32 and Snappy + Adler32

  one-shot      s3s_compress_map_output_device
  stream-whole  ONE feed over the whole output with every end (what the plan's marks, the cut kernel, the gather's read of
                the cut and the seeded checksum add)
  stream-64m / -16m / -4m   feeds of at most that many source bytes, dst_capacity = s3s_cstream_feed_bound of the window;
                the destination is reused
  host-64m      s3s_cstream_feed on page-locked host buffers: ONE source window and ONE image buffer; upload, codec and
                download of a feed do not overlap

Times are a host clock around calls that end in a stream synchronise.  All legs run in ONE process and alternate: every
step runs each leg once, in order; every figure is the median of --steps such steps after --warmup, with the fastest and
slowest beside it.  The comparison is between the rows, never against a target.  The streamed image, lengths and checksums
are compared with the one-shot call's before anything is timed.

usage: python tools/compress_stream_bench.py [--steps 15] [--warmup 3] [--mib 128] [--codecs lz4,snappy] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))

LZ4, SNAPPY, ADLER = 1, 2, 1
WINDOWS = (("stream-64m", 64 << 20), ("stream-16m", 16 << 20), ("stream-4m", 4 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--codecs", default="lz4,snappy")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import s3shuffle
    from s3shuffle import datagen

    dev = torch.device("cuda", 0)
    data, offs = datagen.terasort_map_output(args.mib << 20, 200, seed=2, map_id=0)
    offs = np.asarray(offs, np.int64)
    total, nparts = int(data.size), len(offs) - 1
    d_src = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    rows = []
    for name in args.codecs.split(","):
        codec = {"lz4": LZ4, "snappy": SNAPPY}[name]
        c = s3shuffle.Codec(0)
        cap_all = c.max_compressed_size(codec, offs)
        d_dst = torch.empty(cap_all + 4096, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ref = {}

        def one_shot():
            n, index, sums = c.compress_map_output_device(codec, ADLER, d_src.data_ptr(), offs, d_dst.data_ptr(), cap_all)
            return n, index, sums

        n, index, sums = one_shot()
        ref["img"] = d_dst[:n].cpu().numpy().copy()
        ref["lengths"], ref["sums"] = [int(x) for x in np.diff(index)], [int(x) for x in sums]

        def stream(window, check=False, host=None):
            feeds = closed = 0
            lengths, checks, out = [], [], []
            with c.compress_stream(codec, ADLER) as s:
                pos = 0
                while pos < total or closed < nparts:
                    w = min(window, total - pos)
                    ends = [int(offs[p + 1]) - pos for p in range(closed, nparts) if int(offs[p + 1]) <= pos + w]
                    cap = s.feed_bound(w, len(ends))
                    if host is None:
                        r = s.feed_device(d_src.data_ptr() + pos, w, ends, d_dst.data_ptr(), cap)
                    else:
                        host[0].array[:w] = data[pos:pos + w]  # (the serializer filling the window)
                        r = s.feed(host[0].array[:w], ends, host[1].array, cap)
                    assert r.code == 0 and (r.consumed > 0 or r.parts_closed > 0), (r.code, pos, r.need_src, r.need_dst)
                    if check:
                        out.append(d_dst[:r.out_len].cpu().numpy().copy() if host is None else host[1].array[:r.out_len].copy())
                        lengths += [int(x) for x in r.lengths]
                        checks += [int(x) for x in r.checksums]
                    pos, closed, feeds = pos + r.consumed, closed + r.parts_closed, feeds + 1
            if check:
                assert np.array_equal(np.concatenate(out), ref["img"]), "the streamed image differs from the one-shot call's"
                assert lengths == ref["lengths"] and checks == ref["sums"]
            return feeds

        legs = [("one-shot", lambda: one_shot() and 1), ("stream-whole", lambda: stream(total))]
        for mode, window in WINDOWS:
            if window < total:
                legs.append((mode, lambda window=window: stream(window)))
        hw = min(64 << 20, total)
        host = (s3shuffle.PinnedBuffer(hw), s3shuffle.PinnedBuffer(c.compress_stream(codec, ADLER).feed_bound(hw, nparts) + 64))
        legs.append(("host-64m", lambda: stream(hw, host=host)))
        # every leg's output is the one-shot call's, before anything is timed
        stream(total, check=True)
        for mode, window in WINDOWS:
            if window < total:
                stream(window, check=True)
        stream(hw, check=True, host=host)
        times = {mode: [] for mode, _ in legs}
        feeds = {}
        for step in range(args.warmup + args.steps):
            for mode, fn in legs:
                t0 = time.perf_counter()
                feeds[mode] = fn()
                dt = time.perf_counter() - t0
                if step >= args.warmup:
                    times[mode].append(dt)
        base = statistics.median(times["one-shot"])
        for mode, _ in legs:
            ts = times[mode]
            med = statistics.median(ts)
            row = dict(codec=name, mode=mode, src_bytes=total, image_bytes=int(ref["img"].size), feeds=feeds[mode], steps=len(ts),
                       median_ms=round(med * 1e3, 4), min_ms=round(min(ts) * 1e3, 4), max_ms=round(max(ts) * 1e3, 4),
                       src_gbs=round(total / med / 1e9, 2), vs_one_shot=round(med / base, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
        host[0].free()
        host[1].free()
        c.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
