"""The two pure functions of spark-s3-shuffle_amd/csrc/stream_placement.h on the CPU: which hardware-queue pool a context's
creation slot goes to, and how a batched map-side call packs its small arrays into one arena.  The header is compiled into a
stand-alone program with -fsanitize=address,undefined and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spark-s3-shuffle_amd", "csrc")
LOWEST, NORMAL, HIGHEST, OVERFLOW = 0, 1, 2, 3
TAIL_BYTES, ITEM_BYTES = 64, 24  # sizeof(TaskTail), sizeof(Item) (s3s_internal.h)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("placement") / "stream_placement")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "model", "stream_placement_main.cpp"), "-o", exe],
                   check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


def _shares(cap, levels):
    """queues of each pool that contexts may take: the whole lowest pool, the normal one less the application's stream, the
    highest one less the two copy lanes; a device with fewer levels has no lowest (then no highest) pool"""
    return {LOWEST: cap if levels >= 3 else 0, NORMAL: cap - 1, HIGHEST: max(cap - 2, 0) if levels >= 2 else 0}


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("cap", [1, 2, 4, 16, 32])
def test_stream_class(program, cap, levels):
    got = _run(program, "class", cap, levels, 1)
    share = _shares(cap, levels)
    assert len(got) == 128
    assert all(a <= b for a, b in zip(got, got[1:])), "not monotone in slot"
    for cls in (LOWEST, NORMAL, HIGHEST):
        assert got.count(cls) == share[cls], (cls, got.count(cls))      # class sizes as specified ...
        assert got.count(cls) <= (cap, cap - 1, cap - 2)[cls] or share[cls] == 0  # ... and none beyond its pool's share
    own = sum(share.values())
    assert got[own:] == [OVERFLOW] * (128 - own) and OVERFLOW not in got[:own]
    if levels == 3 and cap == 4:
        assert got[:12] == [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3]


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("cap", [1, 2, 4, 16, 32])
def test_stream_class_other_orders(program, cap, levels):
    """S3S_STREAM_POOLS=2 fills normal, highest, lowest in that order with the same shares; =0 knows no pools"""
    share = _shares(cap, levels)
    got = _run(program, "class", cap, levels, 2)
    want = [NORMAL] * share[NORMAL] + [HIGHEST] * share[HIGHEST] + [LOWEST] * share[LOWEST]
    assert got == want + [OVERFLOW] * (128 - len(want))
    assert _run(program, "class", cap, levels, 0) == [NORMAL] * 128


def test_cap_is_clamped(program):
    assert _run(program, "class", 0, 3, 1) == _run(program, "class", 1, 3, 1)
    assert _run(program, "class", 1000, 3, 1) == _run(program, "class", 32, 3, 1)


@pytest.mark.parametrize("tasks,parts,items", [(1, 0, 0), (1, 1, 0), (3, 5, 9), (2, 2000, 4000)])
def test_packed_plan(program, tasks, parts, items):
    work, tails, item_off, pf, seg, status, up_end, index, sums, total = _run(program, "plan", tasks, parts, items, TAIL_BYTES, ITEM_BYTES)
    np1 = parts + tasks
    regions = [(work, 4), (tails, TAIL_BYTES * tasks), (item_off, ITEM_BYTES * items), (pf, 4 * np1), (seg, 4 * np1),
               (status, 4 * tasks), (index, 8 * np1), (sums, 8 * parts)]
    assert all(off % 16 == 0 for off, _ in regions) and up_end % 16 == 0 and total % 16 == 0
    assert work == 0
    for (a, na), (b, _) in zip(regions, regions[1:]):
        assert a + na <= b, "regions overlap or are out of order"
    assert sums + 8 * parts <= total
    # the upload ends behind the status words and in front of what only the device writes; the download starts at them
    assert status + 4 * tasks <= up_end <= index

    def al(x):
        return (x + 15) // 16 * 16

    want = 16  # the block counter's slot
    for n in (TAIL_BYTES * tasks, ITEM_BYTES * items, 4 * np1, 4 * np1, 4 * tasks, 8 * np1, 8 * parts):
        want = al(want + n)
    assert total == want
