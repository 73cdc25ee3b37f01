"""(GPU) a resumable Zstandard stream (s3s_dstream_open_zstd) against the one-shot call on the same ranges: the
inputs of tools/zstd_decode_staged_bench.py - one libzstd level-1 frame of --mib MiB, and TeraSort --maps x --mib MiB at 25
and 200 partitions per map output, every partition a streamed libzstd frame (no content size, history across the blocks).
One process, one context, compressed ranges and destinations resident in HBM.  Per range the stream is fed in one feed, in
16 MiB windows and in 4 MiB windows (the window grows to need_comp when a feed asks; dst holds every feed's output); the
one-shot call is s3s_decompress_range_device on the same range.  Schedules alternate repeat by repeat; per schedule the
median of the timed passes and their range are reported.

usage: python tools/decode_stream_zstd_bench.py [--legs frame1,terasort25,terasort200] [--mib 128] [--maps 8] [--repeats 3]
                                                [--out PREFIX]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from zstd_decode_blocks_bench import libzstd_image  # noqa: E402

ZSTD, ADLER = 3, 1
SCHEDULES = [("one-shot", None), ("stream, one feed", 0), ("stream, 16 MiB windows", 16 << 20), ("stream, 4 MiB windows", 4 << 20)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="frame1,terasort25,terasort200")
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window-log-max", type=int, default=19)
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    args = ap.parse_args()
    import torch

    import s3shuffle
    from s3shuffle import datagen

    dev = torch.device("cuda", 0)
    codec = s3shuffle.Codec(0)
    lines, rows = [], []

    def stream_pass(d_img, total, index, sums, d_dst, cap, window):
        out = feeds = 0
        with s3shuffle.DecodeStream(codec, ZSTD, ADLER, index, sums, window_log_max=args.window_log_max) as s:
            need = 0
            while True:
                pos = s.position
                w = min(max(window or total, need), total - pos)
                r = s.feed_device(d_img + pos, w, d_dst + out, cap - out)
                assert r.code == 0, (r.code, pos, w)
                feeds += 1
                out += r.out_len
                if r.at_end:
                    break
                need = r.need_comp if r.consumed == 0 else 0
                assert r.consumed > 0 or r.need_comp > w
        return out, feeds

    def timed(label, outs):
        ranges = []
        for data, offs in outs:
            img, index, sums = libzstd_image(data, offs)
            ranges.append((torch.from_numpy(img).to(dev), int(img.size), index, sums, int(data.size)))
        raw = sum(r[4] for r in ranges)
        frames = sum(int(np.count_nonzero(np.diff(o))) for _, o in outs)
        dsts = [torch.empty(n + 64, dtype=torch.uint8, device=dev) for *_, n in ranges]
        times = {name: [] for name, _ in SCHEDULES}
        feeds = {}
        for rep in range(args.repeats + 1):  # (pass 0 warms every schedule up: the workspace has grown)
            for name, window in SCHEDULES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nf = 0
                for (c, ln, idx, sums, n), d in zip(ranges, dsts):
                    if window is None:
                        got = codec.decompress_range_device(ZSTD, ADLER, c.data_ptr(), ln, idx, sums, d.data_ptr(), n)
                    else:
                        got, k = stream_pass(c.data_ptr(), ln, idx, sums, d.data_ptr(), n, window)
                        nf += k
                    assert got == n
                if rep:
                    times[name].append(time.perf_counter() - t0)
                feeds[name] = nf
        row = dict(leg=label, frames=frames, raw_bytes=raw)
        text = f"{label:30s} {frames:5d} frames"
        for name, _ in SCHEDULES:
            t = sorted(times[name])
            med = t[len(t) // 2]
            text += f"\n    {name:24s} {med * 1e3:10.2f} ms median of {len(t)} ({t[0] * 1e3:.2f} - {t[-1] * 1e3:.2f}), {raw / med / 1e9:7.3f} GB/s decoded, {feeds[name]} feeds"
            row[name] = dict(ms_median=round(med * 1e3, 3), ms_min=round(t[0] * 1e3, 3), ms_max=round(t[-1] * 1e3, 3), passes=len(t),
                             gbs=round(raw / med / 1e9, 4), feeds=feeds[name])
        print(text, flush=True)
        lines.append(text)
        rows.append(row)

    for leg in args.legs.split(","):
        if leg == "frame1":
            data = datagen.terasort_map_output(args.mib << 20, 1, seed=2)[0]
            timed(f"libzstd 1 frame {args.mib}MiB", [(data, np.array([0, data.size], np.int64))])
        elif leg in ("terasort25", "terasort200"):
            parts = int(leg[8:])
            outs = [datagen.terasort_map_output(args.mib << 20, parts, seed=2, map_id=m) for m in range(args.maps)]
            timed(f"terasort {args.maps}x{args.mib}MiB at {parts}", outs)
        else:
            raise SystemExit("unknown leg " + leg)
    codec.close()
    if args.out:
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
