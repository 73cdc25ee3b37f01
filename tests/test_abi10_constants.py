"""ABI 10: S3S_OPT_LZ4_BLOCK_SIZE_LARGE is the same number in the header, the Scala shim and the Python binding, and the Scala shim
expects the header's ABI version.  CPU only: what the option DOES needs a context, i.e. a GPU (tests/test_gpu_lz4_big_blocks.py,
which also covers the host mirror's choice of the key and the routing of chunks by their length)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-s3-shuffle_amd"))


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_large_block_size_key_is_8_everywhere():
    from s3shuffle import codec

    header = _read("include", "s3shuffle_codec.h")
    scala = _read("scala", "org", "apache", "spark", "shuffle", "gpu", "S3SCodec.scala")
    assert int(re.search(r"S3S_OPT_LZ4_BLOCK_SIZE_LARGE\s*=\s*(\d+)", header).group(1)) == 8
    assert int(re.search(r"val OPT_LZ4_BLOCK_SIZE_LARGE = (\d+)", scala).group(1)) == 8
    assert codec.OPT_LZ4_BLOCK_SIZE_LARGE == 8 and codec.OPT_LZ4_BLOCK_SIZE == 1
    abi = int(re.search(r"#define\s+S3S_ABI_VERSION\s+(\d+)", header).group(1))
    assert abi >= 10 and int(re.search(r"val ABI_VERSION = (\d+)", scala).group(1)) == abi
    keys = [int(m) for m in re.findall(r"^\s+S3S_OPT_\w+ = (\d+)", header, re.M)]
    assert 8 in keys and len(keys) == len(set(keys)), "two options share a key"
