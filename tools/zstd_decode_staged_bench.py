"""(GPU) reduce-side Zstandard decode of frames WITH history, staged path against one frame per wavefront
(S3S_OPT_ZSTD_DECODE_STAGED 1 / 0).  One process, one context, compressed ranges and destinations resident in
HBM, the batched device entry point; every timed call ends in the library's own stream synchronisation.  The two settings
ALTERNATE call by call on the same context; per setting the median of the timed calls and their range (the spread) are
reported, and S3S_OPT_ZSTD_DECODE_STAGED_BLOCKS of the last call with 1.  All frames are libzstd's, written the way Spark writes
them (streaming API, level 1, 32 KiB at a time: no content size, history across the blocks).

legs:  frame1      one frame of --mib MiB (TeraSort)
       wide        wide rows, --wide-maps x --lz-mib MiB at 64 partitions (512 frames at 8 maps)
       terasort    TeraSort, --lz-maps x --lz-mib MiB at 200 partitions (3 200 frames at 16 maps)
       cuts        --cut-maps x --mib MiB TeraSort (1 GiB at 8 x 128) cut into 100, 25 and 12 partitions per map output

A build of the library without key 15 (S3S_CODEC_LIB = an older build) is timed as it is: the no-harm comparison.

usage: python tools/zstd_decode_staged_bench.py [--legs frame1,wide,terasort,cuts] [--repeats 5] [--mib 128] [--lz-maps 16]
                                                [--lz-mib 32] [--wide-maps 8] [--cut-maps 8] [--out PREFIX]"""
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

OPT_STAGED, OPT_STAGED_BLOCKS = 15, 16
ZSTD, ADLER = 3, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="frame1,wide,terasort,cuts")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--lz-maps", type=int, default=16)
    ap.add_argument("--lz-mib", type=int, default=32)
    ap.add_argument("--wide-maps", type=int, default=8)
    ap.add_argument("--cut-maps", type=int, default=8)
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    args = ap.parse_args()
    import torch

    import s3shuffle
    from s3shuffle import datagen

    dev = torch.device("cuda", 0)
    codec = s3shuffle.Codec(0)
    has_key = codec._lib.s3s_set_option(codec._h, OPT_STAGED, 0) == 0  # (a build from before the staged path: one setting)
    settings = (0, 1) if has_key else (None,)
    lines, rows = [], []

    def timed(label, outs, repeats):
        """outs: [(data, offsets)] map outputs -> libzstd images in HBM, alternating timed calls"""
        ranges = []
        for data, offs in outs:
            img, index, sums = libzstd_image(data, offs)
            ranges.append((torch.from_numpy(img).to(dev), int(img.size), index, sums, int(data.size)))
        raw = sum(int(d.size) for d, _ in outs)
        comp = sum(r[1] for r in ranges)
        frames = sum(int(np.count_nonzero(np.diff(o))) for _, o in outs)
        dsts = [torch.empty(n + 16, dtype=torch.uint8, device=dev) for *_, n in ranges]
        call = [(c.data_ptr(), ln, idx, sums, d.data_ptr(), n) for (c, ln, idx, sums, n), d in zip(ranges, dsts)]
        times = {v: [] for v in settings}
        blocks = 0
        for v in settings:  # warm-up of both, buffers grown
            if v is not None:
                codec.set_option(OPT_STAGED, v)
            codec.decompress_ranges_batch_device(ZSTD, ADLER, call)
        for r in range(repeats):
            for v in settings:
                if v is not None:
                    codec.set_option(OPT_STAGED, v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = codec.decompress_ranges_batch_device(ZSTD, ADLER, call)
                times[v].append(time.perf_counter() - t0)
                assert all(st == 0 and m == n for (st, m, _), (*_, n) in zip(res, ranges))
                if v == 1:
                    blocks = codec.get_option(OPT_STAGED_BLOCKS)
        row = dict(leg=label, frames=frames, raw_bytes=raw, comp_bytes=comp, library=os.environ.get("S3S_CODEC_LIB", "this build"))
        text = f"{label:34s} {frames:5d} frames"
        for v in settings:
            t = sorted(times[v])
            med = t[len(t) // 2]
            name = "staged %s" % v if v is not None else "(no key 15)"
            text += f" | {name}: {med * 1e3:9.2f} ms median of {len(t)} ({t[0] * 1e3:.2f} - {t[-1] * 1e3:.2f}), {raw / med / 1e9:7.2f} GB/s decoded"
            row[name] = dict(ms_median=round(med * 1e3, 3), ms_min=round(t[0] * 1e3, 3), ms_max=round(t[-1] * 1e3, 3), calls=len(t),
                             gbs=round(raw / med / 1e9, 3))
        if has_key:
            text += f" | blocks on the staged path: {blocks}"
            row["blocks"] = blocks
        print(text, flush=True)
        lines.append(text)
        rows.append(row)
        del dsts, ranges

    for leg in args.legs.split(","):
        if leg == "frame1":
            data = datagen.terasort_map_output(args.mib << 20, 1, seed=2)[0]
            timed(f"libzstd 1 frame {args.mib}MiB", [(data, np.array([0, data.size], np.int64))], args.repeats)
        elif leg == "wide":
            outs = [datagen.tpcds_wide_map_output(args.lz_mib << 20, 64, seed=3, map_id=m) for m in range(args.wide_maps)]
            timed(f"libzstd wide {args.wide_maps}x{args.lz_mib}MiB", outs, 2 * args.repeats)
        elif leg == "terasort":
            outs = [datagen.terasort_map_output(args.lz_mib << 20, 200, seed=2, map_id=m) for m in range(args.lz_maps)]
            timed(f"libzstd terasort {args.lz_maps}x{args.lz_mib}MiB", outs, 2 * args.repeats)
        elif leg == "cuts":
            for parts in (100, 25, 12):
                outs = [datagen.terasort_map_output(args.mib << 20, parts, seed=2, map_id=m) for m in range(args.cut_maps)]
                timed(f"libzstd terasort {args.cut_maps}x{args.mib}MiB at {parts}", outs, args.repeats)
        else:
            raise SystemExit("unknown leg " + leg)
    codec.close()
    if args.out:
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
