"""(GPU) what IO encryption adds to the streaming map side (s3s_cstream_open_encrypted): one 128 MiB TeraSort map output of 200
partitions resident in HBM, compress + checksum of the whole output, LZ4 + Adler32 and Snappy + Adler32, AES-128

  one-shot-enc                  s3s_compress_map_output_device on the keyed context
  plain-whole / enc-whole       ONE feed over the whole output with every end: the plain stream (a second, unkeyed context of
                                the same library) and the encrypted stream
  plain-64m / enc-64m, -16m, -4m   feeds of at most that many source bytes, dst_capacity = s3s_cstream_feed_bound of the
                                window; the destination is reused

Times are a host clock around calls that end in a stream synchronise.  All legs run in ONE process and alternate: every step
runs each leg once, in order; every figure is the median of --steps such steps after --warmup, with the fastest and slowest
beside it.  `over_plain_ms` is the encrypted leg's median minus its plain twin's, `pass_gbs` the stored bytes over that
difference: the rate of the encrypt pass as the feed sees it, IV upload and seed launch included.  The comparison is between
the rows, never against a target.  The encrypted stream's image, lengths and checksums are compared with the one-shot
encrypted call's before anything is timed.

usage: python tools/compress_stream_encrypted_bench.py [--steps 15] [--warmup 3] [--mib 128] [--codecs lz4,snappy] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))

LZ4, SNAPPY, ADLER = 1, 2, 1
WINDOWS = (("whole", None), ("64m", 64 << 20), ("16m", 16 << 20), ("4m", 4 << 20))


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
    ivs = np.random.default_rng(1).integers(0, 256, (nparts + 1, 16), dtype=np.uint8)  # (one spare for the piece behind the last end)
    rows = []
    for name in args.codecs.split(","):
        codec = {"lz4": LZ4, "snappy": SNAPPY}[name]
        plain, keyed = s3shuffle.Codec(0), s3shuffle.Codec(0)
        keyed.set_io_encryption(bytes(range(16)))
        cap_all = keyed.max_compressed_size(codec, offs)
        d_dst = torch.empty(cap_all + 4096, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def one_shot():
            keyed.set_stream_ivs(ivs[:nparts].reshape(-1))
            return keyed.compress_map_output_device(codec, ADLER, d_src.data_ptr(), offs, d_dst.data_ptr(), cap_all)

        n, index, sums = one_shot()
        ref_img = d_dst[:n].cpu().numpy().copy()
        ref_lengths, ref_sums = [int(x) for x in np.diff(index)], [int(x) for x in sums]

        def stream(window, enc, check=False):
            c = keyed if enc else plain
            feeds = closed = 0
            lengths, checks, out = [], [], []
            with c.compress_stream(codec, ADLER, encrypted=enc) as s:
                pos = 0
                while pos < total or closed < nparts:
                    w = min(window or total, total - pos)
                    ends = [int(offs[p + 1]) - pos for p in range(closed, nparts) if int(offs[p + 1]) <= pos + w]
                    cap = s.feed_bound(w, len(ends))
                    if enc:
                        c.set_stream_ivs(ivs[closed:closed + len(ends) + 1].reshape(-1))
                    r = s.feed_device(d_src.data_ptr() + pos, w, ends, d_dst.data_ptr(), cap)
                    assert r.code == 0 and (r.consumed > 0 or r.parts_closed > 0), (r.code, pos, r.need_src, r.need_dst)
                    if check:
                        out.append(d_dst[:r.out_len].cpu().numpy().copy())
                        lengths += [int(x) for x in r.lengths]
                        checks += [int(x) for x in r.checksums]
                    pos, closed, feeds = pos + r.consumed, closed + r.parts_closed, feeds + 1
            if check:
                assert np.array_equal(np.concatenate(out), ref_img), "the streamed image differs from the one-shot encrypted call's"
                assert lengths == ref_lengths and checks == ref_sums
            return feeds

        legs = [("one-shot-enc", lambda: one_shot() and 1)]
        for tag, window in WINDOWS:
            if window is None or window < total:
                legs.append(("plain-" + tag, lambda window=window: stream(window, False)))
                legs.append(("enc-" + tag, lambda window=window: stream(window, True)))
                stream(window, True, check=True)  # the one-shot encrypted call's bytes, before anything is timed
        times = {mode: [] for mode, _ in legs}
        feeds = {}
        for step in range(args.warmup + args.steps):
            for mode, fn in legs:
                t0 = time.perf_counter()
                feeds[mode] = fn()
                dt = time.perf_counter() - t0
                if step >= args.warmup:
                    times[mode].append(dt)
        med = {mode: statistics.median(ts) for mode, ts in times.items()}
        for mode, _ in legs:
            ts = times[mode]
            row = dict(codec=name, mode=mode, src_bytes=total, stored_bytes=int(ref_img.size), feeds=feeds[mode], steps=len(ts),
                       median_ms=round(med[mode] * 1e3, 4), min_ms=round(min(ts) * 1e3, 4), max_ms=round(max(ts) * 1e3, 4),
                       vs_one_shot_enc=round(med[mode] / med["one-shot-enc"], 3))
            if mode.startswith("enc-"):
                over = med[mode] - med["plain-" + mode[4:]]
                row.update(over_plain_ms=round(over * 1e3, 4), pass_gbs=round(ref_img.size / over / 1e9, 1) if over > 0 else None)
            rows.append(row)
            print(json.dumps(row), flush=True)
        plain.close()
        keyed.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
