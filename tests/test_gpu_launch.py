"""The N-GPU launch line, on one GPU: bench.py under `python -m torch.distributed.run
--nproc-per-node 1` creates the RCCL process group (backend "nccl"), runs the barrier + MAX / SUM all_reduce the
scaling runs use, and prints the contract's JSON line; --dry-run validates rank <-> device <-> mapId."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(extra, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_dry_run_over_rccl():
    d = _launch(["--dry-run", "--maps-per-gpu", "4"], 29551)
    assert d["ok"] and d["backend"] == "nccl" and d["world"] == 1
    assert d["ranks"][0]["map_ids"] == [0, 1, 2, 3] and d["ranks"][0]["device"] == "cuda:0"


def test_timed_run_through_the_process_group():
    d = _launch(["--steps", "2", "--warmup", "1", "--maps-per-gpu", "2", "--map-mib", "16", "--no-cpu-baseline", "--full"], 29552)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["metric"] == "shuffle_block_compress_checksum_throughput" and d["unit"] == "GB/s" and d["value"] > 0
    assert d["config"]["workload"] == "terasort-10g-200p-lz4" and "roofline" in d
    assert d["image_verified"] is True and d["rccl_ranks"] == 1


def test_plain_command_last_line_is_the_compact_headline():
    """The driver's N=1 form (`python bench.py --gpus 1 ...`, no launcher): the LAST stdout line alone must round-trip as the
    contract's JSON object, under 4 KB, with roofline + cpu_baseline + image_verified."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--maps-per-gpu", "2",
           "--map-mib", "16", "--cpu-seconds", "1", "--full-line", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    last = lines[-1]
    assert len(last) < 4096
    d = json.loads(last)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["image_verified"] is True and d["cpu_baseline"]["cores"] >= 1 and d["roofline"]["bound"] == "hbm"
    assert d["roofline"]["achieved"] > 0 and d["rccl_ranks"] == 0
    full = json.loads(lines[-2])["full_record"]
    assert full["value"] == d["value"] and len(full["cpu_baseline"]["sample"]) > len(d["cpu_baseline"]["sample"])


def test_plain_run_is_lean_and_dumps_what_its_last_step_returned(tmp_path, oracle):
    """Without --full the run times the steps and prints the line, nothing else (no CPU leg, no oracle check); --dump-outputs
    holds what the last timed step returned: index and checksums equal to the oracle's for the same map outputs, the CRC32 of
    the .data image in HBM equal to that of the oracle's image."""
    import zlib

    import numpy as np

    import bench
    from s3shuffle import datagen

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--maps-per-gpu", "2",
           "--map-mib", "16", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["cpu_baseline"] is None
    assert "image_verified" not in d and "secondary_file" not in d
    got = {f.stem: np.load(f) for f in tmp_path.iterdir()}
    assert got["map_ids"].tolist() == [0, 1]
    for i in range(2):
        data, offs = datagen.terasort_map_output(16 << 20, 200, seed=2, map_id=i)
        img, index, sums = oracle.compress_map_output(oracle.CODEC_LZ4, oracle.CHECKSUM_ADLER32, data, offs)
        assert np.array_equal(got["index"][i], index) and np.array_equal(got["checksums"][i], sums)
        assert got["data_image_bytes"][i] == img.size and got["data_image_crc32"][i] == zlib.crc32(img)
        pos = bench.dump_sample_positions(i, img.size, got["data_image_sample"].shape[1])
        assert np.array_equal(got["data_image_sample"][i], img[pos].astype(np.float32))


def test_plain_decode_run_is_lean_and_dumps_the_decoded_bytes(tmp_path):
    """The reduce side without --full: no bytes_verified in the line (no check ran), and the dump holds the decoded bytes of
    the last timed step — equal to the source map outputs"""
    import zlib

    import numpy as np

    import bench
    from s3shuffle import datagen

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--direction", "decompress", "--steps", "2", "--warmup", "1",
           "--maps-per-gpu", "2", "--map-mib", "16", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "shuffle_block_verify_decompress_throughput" and d["steps"] == 2 and d["ms_per_step"] > 0
    assert "bytes_verified" not in d and "image_verified" not in d and d["cpu_baseline"] is None
    got = {f.stem: np.load(f) for f in tmp_path.iterdir()}
    assert sorted(got) == ["decoded_bytes", "decoded_crc32", "decoded_sample", "map_ids"] and got["map_ids"].tolist() == [0, 1]
    for i in range(2):
        data, _ = datagen.terasort_map_output(16 << 20, 200, seed=2, map_id=i)
        assert got["decoded_bytes"][i] == data.size and got["decoded_crc32"][i] == zlib.crc32(data)
        pos = bench.dump_sample_positions(i, data.size, got["decoded_sample"].shape[1])
        assert np.array_equal(got["decoded_sample"][i], data[pos].astype(np.float32))
