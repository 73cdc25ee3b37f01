"""Contexts are spread over the runtime's hardware-queue pools by creation slot (csrc/stream_placement.h, S3S_OPT_STREAM_CLASS),
and a context computes the same bytes in whichever pool its stream lives.  The placement itself is checked in a fresh process:
the slots of a device are shared by every context alive in the process, the session's own included."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LZ4, ADLER = 1, 1
OPT_STREAM_CLASS = 12
SIZES = [0, 1, 32767, 32768, 32769, 70000]


def map_outputs():
    """the two map tasks of every call of this file: the same partition sizes, other bytes"""
    import corpus

    out = []
    for t in range(2):
        rng = np.random.default_rng(40 + t)
        parts = []
        for i, n in enumerate(SIZES):
            kind = (3 + 2 * i + t) % corpus.N_KINDS
            parts.append(corpus.chunk_corpus(7 if kind == 6 and n > 5000 else kind, n, rng))  # (kind 6 is a Python loop per byte)
        offs = np.zeros(len(SIZES) + 1, np.int64)
        np.cumsum([p.size for p in parts], out=offs[1:])
        out.append((np.concatenate(parts).astype(np.uint8), offs))
    return out


def expected_class(slot, cap, levels=3):
    """the policy as the issue states it: the first `cap` contexts in the lowest pool, the next cap-1 in the normal one (one
    queue stays the application's), the next cap-2 in the highest (two stay the copy lanes'), the rest share normal queues"""
    pools = ([(0, cap)] if levels >= 3 else []) + [(1, cap - 1)] + ([(2, max(cap - 2, 0))] if levels >= 2 else [])
    for cls, n in pools:
        if slot < n:
            return cls
        slot -= n
    return 3


def _child(mode, out_path):
    """runs in a fresh process (see the bottom of the file)"""
    import ctypes

    sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "spark-s3-shuffle_amd")]
    import s3shuffle
    from hipdev import Dev

    s3shuffle.load_library()
    if mode == "placement":
        cap = min(max(int(os.environ["GPU_MAX_HW_QUEUES"]), 1), 32)  # (load_library sets the variable where the caller has not)
        ctxs = [s3shuffle.Codec(0) for _ in range(3 * cap)]
        classes = [c.get_option(OPT_STREAM_CLASS) for c in ctxs]
        ctxs[1].close()
        again = s3shuffle.Codec(0)
        hip = ctypes.CDLL("libamdhip64.so")
        least, greatest = ctypes.c_int(0), ctypes.c_int(0)
        assert hip.hipDeviceGetStreamPriorityRange(ctypes.byref(least), ctypes.byref(greatest)) == 0
        res = {"cap": cap, "classes": classes, "second_again": again.get_option(OPT_STREAM_CLASS), "levels": least.value - greatest.value + 1,
               "read_only": again._lib.s3s_set_option(again._h, OPT_STREAM_CLASS, 0)}
        json.dump(res, open(out_path, "w"))
        for c in ctxs + [again]:
            c.close()
    else:  # "one": one context, the two map tasks in one batched call
        dev = Dev()
        with s3shuffle.Codec(0) as c:
            tasks = []
            for data, offs in map_outputs():
                cap = c.max_compressed_size(LZ4, offs)
                tasks.append((dev.upload(data), offs, dev.alloc(cap), cap))
            res = c.compress_map_outputs_batch_device(LZ4, ADLER, tasks)
            np.savez(out_path, stream_class=c.get_option(OPT_STREAM_CLASS),
                     **{f"{k}{t}": v for t, (total, index, sums) in enumerate(res)
                        for k, v in (("index", index), ("sums", sums), ("image", dev.download(tasks[t][2], total)))})
        dev.free()


def _run_child(mode, out_path, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, str(out_path)], env={**os.environ, **env}, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def reference(oracle):
    return [oracle.compress_map_output(LZ4, ADLER, d, o) for d, o in map_outputs()]


def test_classes_follow_creation_order(tmp_path):
    _run_child("placement", tmp_path / "placement.json")
    res = json.load(open(tmp_path / "placement.json"))
    cap, levels = res["cap"], res["levels"]
    assert len(res["classes"]) == 3 * cap
    assert res["classes"] == [expected_class(slot, cap, levels) for slot in range(3 * cap)]
    assert res["second_again"] == expected_class(1, cap, levels)  # the slot the second context gave back
    assert res["read_only"] == -1  # S3S_E_INVALID


def test_nine_contexts_in_nine_threads(gpu_codec, oracle, reference):
    """nine contexts (at the default cap: every pool, and one context beyond them) compress the same two map tasks at the same
    time, then decode them on the same contexts"""
    import s3shuffle
    from hipdev import Dev

    host = map_outputs()
    dev = Dev()
    ctxs = [s3shuffle.Codec(0) for _ in range(9)]
    try:
        jobs = []
        for c in ctxs:
            tasks = []
            for data, offs in host:
                cap = c.max_compressed_size(LZ4, offs)
                tasks.append((dev.upload(data), offs, dev.alloc(cap), cap))
            jobs.append({"tasks": tasks, "outs": [dev.alloc(d.size) for d, _ in host]})
        go = threading.Barrier(len(ctxs))

        def work(c, job):
            try:
                go.wait(timeout=60)
                job["res"] = c.compress_map_outputs_batch_device(LZ4, ADLER, job["tasks"])
                ranges = [(job["tasks"][t][2], total, index, sums, job["outs"][t], host[t][0].size)
                          for t, (total, index, sums) in enumerate(job["res"])]
                job["dec"] = c.decompress_ranges_batch_device(LZ4, ADLER, ranges)
            except Exception as e:  # reported by the main thread
                job["error"] = e

        threads = [threading.Thread(target=work, args=(c, j)) for c, j in zip(ctxs, jobs)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for k, job in enumerate(jobs):
            assert "error" not in job, (k, job.get("error"))
            for t, ((total, index, sums), (r_img, r_index, r_sums)) in enumerate(zip(job["res"], reference)):
                assert np.array_equal(index, r_index), (k, t)
                assert np.array_equal(sums, r_sums), (k, t)
                assert total == r_img.size and np.array_equal(dev.download(job["tasks"][t][2], total), r_img), (k, t)
                st, n, bad = job["dec"][t]
                assert (st, n) == (0, host[t][0].size), (k, t, st, bad)
                assert np.array_equal(dev.download(job["outs"][t], n), host[t][0]), (k, t)
    finally:
        for c in ctxs:
            c.close()
        dev.free()


def test_without_pools_the_same_bytes(tmp_path, reference):
    """S3S_STREAM_POOLS=0: every stream at normal priority, as before the pools"""
    _run_child("one", tmp_path / "one.npz", S3S_STREAM_POOLS="0")
    got = np.load(tmp_path / "one.npz")
    assert int(got["stream_class"]) == 1
    for t, (r_img, r_index, r_sums) in enumerate(reference):
        assert np.array_equal(got[f"index{t}"], r_index)
        assert np.array_equal(got[f"sums{t}"], r_sums)
        assert np.array_equal(got[f"image{t}"], r_img)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
