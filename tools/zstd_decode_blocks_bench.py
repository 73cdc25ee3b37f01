"""(GPU) reduce-side Zstandard decode, block path against one frame per wavefront (S3S_OPT_ZSTD_DECODE_VARIANT 1 / 0).
One process, one context, compressed ranges and destinations resident in HBM, the batched device entry point; every timed call
ends in the library's own stream synchronisation.  The two variants ALTERNATE call by call on the same context; per variant the
median of the timed calls and their range (the spread) are reported, and S3S_OPT_ZSTD_DECODE_BLOCKS of the last variant-1 call.

legs:  writer200   frames of the library's writer (S3S_OPT_ZSTD_COMPRESS = 1): TeraSort at 200 partitions and wide rows at 64,
                   --maps x --mib MiB in one call
       writer1     one partition per task: one frame of --mib MiB (TeraSort)
       frame1g     one frame of 1 GiB (TeraSort); variant 0 is timed once (it takes half a minute)
       sweep       the TeraSort bytes of writer200 at 200, 100, 50, 25 and 12 partitions per map output (frames of ~5 to ~86 blocks)
       libzstd     frames libzstd writes the way Spark does (streaming, level 1): --lz-maps x --lz-mib MiB TeraSort at 200
                   partitions (3 200 frames at 16 maps) and the wide-rows set - the no-harm leg; run the tool again with
                   S3S_CODEC_LIB = another build of the library to compare (a build without key 13 is timed as it is)

usage: python tools/zstd_decode_blocks_bench.py [--legs writer200,writer1,frame1g,libzstd] [--repeats 5] [--maps 8] [--mib 128]
                                                [--lz-maps 16] [--lz-mib 32] [--out PREFIX]"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))
import numpy as np  # noqa: E402

OPT_ZSTD_COMPRESS, OPT_VARIANT, OPT_BLOCKS = 9, 13, 14
ZSTD, ADLER = 3, 1


class _Buf(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


def libzstd_stream(z, data, chunk=32768):
    """One frame the way zstd-jni's ZstdOutputStream writes it for Spark: level 1, the bytes 32 KiB at a time, no content size."""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    cctx = z.ZSTD_createCCtx()
    z.ZSTD_CCtx_setParameter(cctx, 100, 1)  # ZSTD_c_compressionLevel
    cap = int(z.ZSTD_compressBound(d.size)) + 1024
    out = np.empty(cap, dtype=np.uint8)
    ob = _Buf(out.ctypes.data, cap, 0)
    for pos in range(0, d.size, chunk):
        ib = _Buf(d.ctypes.data + pos, min(chunk, d.size - pos), 0)
        while ib.pos < ib.size:
            assert not z.ZSTD_isError(z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), 0))  # ZSTD_e_continue
    ib = _Buf(d.ctypes.data, 0, 0)
    while True:
        r = z.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(ib), 2)  # ZSTD_e_end
        assert not z.ZSTD_isError(r)
        if r == 0:
            break
    z.ZSTD_freeCCtx(cctx)
    return out[:ob.pos].copy()


def libzstd_image(data, offs):
    """image, index, Adler32 per partition: one streamed frame per non-empty partition"""
    z = ctypes.CDLL("libzstd.so.1")
    z.ZSTD_compressBound.restype = ctypes.c_size_t
    z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
    z.ZSTD_isError.restype = ctypes.c_uint
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]
    z.ZSTD_createCCtx.restype = ctypes.c_void_p
    z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
    z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
    z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    z.ZSTD_compressStream2.restype = ctypes.c_size_t
    z.ZSTD_compressStream2.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Buf), ctypes.POINTER(_Buf), ctypes.c_int]
    n = len(offs) - 1
    parts = [libzstd_stream(z, data[offs[p]:offs[p + 1]]) if offs[p + 1] > offs[p] else np.zeros(0, np.uint8) for p in range(n)]
    index = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([q.size for q in parts], out=index[1:])
    sums = np.array([zlib.adler32(q.tobytes()) for q in parts], dtype=np.int64)
    return np.concatenate(parts), index, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="writer200,writer1,frame1g,libzstd")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--mib", type=int, default=128)
    ap.add_argument("--lz-maps", type=int, default=16)
    ap.add_argument("--lz-mib", type=int, default=32)
    ap.add_argument("--out", default="", help="write PREFIX.txt / PREFIX.json")
    args = ap.parse_args()
    import torch

    import s3shuffle
    from s3shuffle import datagen

    dev = torch.device("cuda", 0)
    codec = s3shuffle.Codec(0)
    has_key = codec._lib.s3s_set_option(codec._h, OPT_VARIANT, 1) == 0  # (a build from before the block path: one variant)
    variants = (0, 1) if has_key else (None,)
    lines, rows = [], []

    def timed(label, ranges, raw, repeats, repeats_v0=None):
        """ranges: [(d_comp tensor, comp_len, index, sums, n)] -> alternating timed calls"""
        dsts = [torch.empty(n + 16, dtype=torch.uint8, device=dev) for *_, n in ranges]
        call = [(c.data_ptr(), ln, idx, sums, d.data_ptr(), n) for (c, ln, idx, sums, n), d in zip(ranges, dsts)]
        times = {v: [] for v in variants}
        blocks = 0
        for v in variants:  # warm-up of both, buffers grown
            if v is not None:
                codec.set_option(OPT_VARIANT, v)
            if not (v == 0 and repeats_v0 == 1):
                codec.decompress_ranges_batch_device(ZSTD, ADLER, call)
        for r in range(repeats):
            for v in variants:
                if v == 0 and repeats_v0 is not None and r >= repeats_v0:
                    continue
                if v is not None:
                    codec.set_option(OPT_VARIANT, v)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = codec.decompress_ranges_batch_device(ZSTD, ADLER, call)
                times[v].append(time.perf_counter() - t0)
                assert all(st == 0 and m == n for (st, m, _), (*_, n) in zip(res, ranges))
                if v == 1:
                    blocks = codec.get_option(OPT_BLOCKS)
        row = dict(leg=label, raw_bytes=raw, library=os.environ.get("S3S_CODEC_LIB", "this build"))
        text = f"{label:28s}"
        for v in variants:
            t = sorted(times[v])
            med = t[len(t) // 2]
            name = "variant %s" % v if v is not None else "(no key 13)"
            text += f" | {name}: {med * 1e3:9.2f} ms median of {len(t)} ({t[0] * 1e3:.2f} - {t[-1] * 1e3:.2f}), {raw / med / 1e9:7.2f} GB/s decoded"
            row[name] = dict(ms_median=round(med * 1e3, 3), ms_min=round(t[0] * 1e3, 3), ms_max=round(t[-1] * 1e3, 3), calls=len(t),
                             gbs=round(raw / med / 1e9, 3))
        if has_key:
            text += f" | blocks on the block path: {blocks}"
            row["blocks"] = blocks
        print(text, flush=True)
        lines.append(text)
        rows.append(row)
        del dsts

    def writer_ranges(outs):
        """map outputs -> ranges of the library's own frames, compressed here, resident in HBM"""
        codec.set_option(OPT_ZSTD_COMPRESS, 1)
        ranges = []
        for data, offs in outs:
            cap = codec.max_compressed_size(ZSTD, offs)
            d_src = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
            d_img = torch.empty(cap + 16, dtype=torch.uint8, device=dev)
            total, index, sums = codec.compress_map_output_device(ZSTD, ADLER, d_src.data_ptr(), offs, d_img.data_ptr(), cap)
            ranges.append((d_img[:total].clone(), total, index, sums, int(data.size)))
            del d_src, d_img
        codec.set_option(OPT_ZSTD_COMPRESS, 0)
        return ranges

    for leg in args.legs.split(","):
        if leg == "writer200":
            for name in ("terasort", "wide"):
                outs = [(datagen.terasort_map_output(args.mib << 20, 200, seed=2, map_id=m) if name == "terasort"
                         else datagen.tpcds_wide_map_output(args.mib << 20, 64, seed=3, map_id=m)) for m in range(args.maps)]
                timed(f"writer {name} {args.maps}x{args.mib}MiB", writer_ranges(outs), sum(d.size for d, _ in outs), args.repeats)
        elif leg == "sweep":  # the crossover: the same bytes cut into fewer, longer frames
            for parts in (200, 100, 50, 25, 12):
                outs = [datagen.terasort_map_output(args.mib << 20, parts, seed=2, map_id=m) for m in range(args.maps)]
                blocks = -(-(args.mib << 20) // parts // (1 << 17))
                timed(f"writer terasort {args.maps * parts} frames of ~{blocks} blocks", writer_ranges(outs), sum(d.size for d, _ in outs), args.repeats)
        elif leg == "writer1":
            data = datagen.terasort_map_output(args.mib << 20, 1, seed=2)[0]
            timed(f"writer 1 frame {args.mib}MiB", writer_ranges([(data, np.array([0, data.size], np.int64))]), int(data.size), max(3, args.repeats // 2 + 1))
        elif leg == "frame1g":
            piece = datagen.terasort_map_output(128 << 20, 1, seed=2)[0]
            data = np.resize(piece, 1 << 30)
            timed("writer 1 frame 1GiB", writer_ranges([(data, np.array([0, data.size], np.int64))]), int(data.size), args.repeats, repeats_v0=1)
        elif leg == "libzstd":
            for name in ("terasort", "wide"):
                maps = args.lz_maps if name == "terasort" else max(1, args.lz_maps // 2)
                outs = [(datagen.terasort_map_output(args.lz_mib << 20, 200, seed=2, map_id=m) if name == "terasort"
                         else datagen.tpcds_wide_map_output(args.lz_mib << 20, 64, seed=3, map_id=m)) for m in range(maps)]
                ranges = []
                for data, offs in outs:
                    img, index, sums = libzstd_image(data, offs)
                    ranges.append((torch.from_numpy(img).to(dev), int(img.size), index, sums, int(data.size)))
                frames = sum(int(np.count_nonzero(np.diff(o))) for _, o in outs)
                timed(f"libzstd {name} {frames} frames", ranges, sum(d.size for d, _ in outs), 2 * args.repeats)
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
