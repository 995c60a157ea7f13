"""The parts of the streaming map pass with no device in them (csrc/ps_map_plan.h): which devices and how many workers, the
piece-size rule, and the hand-over queue's bound, close and abort.  tests/map_plan_check.cpp includes that header alone, is built by
the host compiler with AddressSanitizer and UBSan and runs as a plain executable."""
import itertools
import os
import subprocess

import pytest

from test_capi_cpu import ROOT

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "map_plan_check")
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread",
           "-I", os.path.join(ROOT, "para-suite_amd", "csrc"), os.path.join(ROOT, "tests", "map_plan_check.cpp"), "-o", out]
    subprocess.check_call(cmd[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + cmd[1:])
    return out


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, timeout=120, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def test_the_header_needs_no_hip():
    text = open(os.path.join(ROOT, "para-suite_amd", "csrc", "ps_map_plan.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_plan_devices(exe):
    """values worked by hand from the rule: distinct devices in the order named, a worker per mention, at least per_dev, at most max_lanes"""
    cases = [  # ids, gpus, per_dev, present, max_lanes -> devices, workers (None: not looked at)
        (("0,0", 1, 1, 1, 4), [0], [2]),
        (("1,0,1", 1, 1, 1, 4), [1, 0], [2, 1]),
        (("0", 1, 2, 1, 4), [0], [2]),
        (("2,2,2,2,2,2", 1, 1, 1, 4), [2], [4]),
        (("-", 3, 1, 2, 4), [0, 1], [1, 1]),
        (("-", 1, 1, 1, 4), [0], [1]),
        (("-", 0, 0, 1, 4), [0], [1]),                # nothing stated, and nothing sensible stated
        (("0,1", 1, 9, 1, 4), [0, 1], [4, 4]),        # the floor itself is capped
        (("3", 8, 1, 8, 4), [3], [1]),                # a list overrides the count
    ]
    lines = _run(exe, "devices", *[a for c in cases for a in c[0]])
    assert len(lines) == len(cases)
    for (args, devs, workers), line in zip(cases, lines):
        d, w = ([int(x) for x in part.split(",")] for part in line.split())
        assert (d, w) == (devs, workers), (args, line)


def plan_pieces(size, n_workers, bam, chunk_mb, hungry_mb, first_mb):
    """the piece-size rule, restated: 1 GB pieces, handed over early from 128 MB or a fifth of the input on; with several workers
    at most 1/(2 x workers) of the input (+ 64 KiB, at least 16 MB); BAM out: at most a quarter (+ 64 KiB, at least 64 MB) and early
    from half a piece on; a stated piece size is taken as it is; stated hungry and first sizes come last"""
    chunk, hungry, first = 1 * GiB, 128 * MiB, 0
    if chunk_mb:
        chunk = hungry = chunk_mb * MiB
    elif size > 0:
        if n_workers > 1:
            chunk = min(chunk, max(16 * MiB, -(-size // (2 * n_workers)) + 64 * KiB))
        hungry = min(chunk, max(hungry, size // 5))
        if bam:
            chunk = min(chunk, max(64 * MiB, size // 4 + 64 * KiB))
            hungry = min(hungry, chunk // 2)
    if hungry_mb:
        hungry = hungry_mb * MiB
    if first_mb:
        first = first_mb * MiB
    return chunk, hungry, first


def test_plan_pieces(exe):
    grid = list(itertools.product((0, 1 * MiB, 10 * MiB, 400 * MiB, 1000 * MiB, 40 * GiB), (1, 2, 4), (0, 1), (0, 48), (0, 7), (0, 3)))
    lines = _run(exe, "pieces", *[a for c in grid for a in c])
    got = {c: tuple(int(x) for x in l.split()) for c, l in zip(grid, lines)}
    assert len(lines) == len(grid) == 6 * 3 * 2 * 2 * 2 * 2
    for c in grid:
        assert got[c] == plan_pieces(*c), c
    # worked by hand
    assert got[(10 * MiB, 1, 0, 0, 0, 0)] == (1 * GiB, 128 * MiB, 0)
    assert got[(400 * MiB, 2, 0, 0, 0, 0)] == (100 * MiB + 64 * KiB, 100 * MiB + 64 * KiB, 0)
    assert got[(1000 * MiB, 1, 1, 0, 0, 0)] == (250 * MiB + 64 * KiB, 125 * MiB + 32 * KiB, 0)
    assert got[(40 * GiB, 4, 1, 48, 7, 3)] == (48 * MiB, 7 * MiB, 3 * MiB)       # everything stated: the input's size plays no part
    assert got[(0, 4, 1, 0, 0, 0)] == (1 * GiB, 128 * MiB, 0)                    # size unknown: the defaults


def test_chan(exe):
    assert _run(exe, "chan") == ["chan ok"]
