"""The parts of a search launch with no device in them (csrc/ps_search_plan.h): the knobs the search stage reads from the
environment, the launch geometry that run_search and reserve_search_workspace share, and the budget-by-length table of a ragged
launch.  tests/search_plan_check.cpp includes that header with ps_core.h and ps_model.h, is built by the host compiler with
AddressSanitizer and UBSan and runs as a plain executable.  The expected geometry is worked by hand from the rule."""
import math
import os
import re
import subprocess

import pytest

from test_capi_cpu import ROOT

CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
GiB = 1 << 30
LM = 156                  # lm_bytes(50, 32, 25, narrow): 163,840 / (256 x 156) = 4 workgroups per CU
CUS = 256
BIG = 65535 * 16          # bytes of a large slot: 1,048,560
LDS_ERROR = "error: read length / score range too large for the per-lane LDS state"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "search_plan_check")
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
           "-I", CSRC, os.path.join(ROOT, "tests", "search_plan_check.cpp"), "-o", out]
    subprocess.check_call(cmd[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + cmd[1:])
    return out


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], check=True, timeout=120, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def _geometry(exe, cases):
    """cases: (reads, lm, pool_cap, wide, cus, bt_blocks, max_per_cu, n_big) -> dicts (or the error line)"""
    lines = _run(exe, "geometry", *[a for c in cases for a in c])
    assert len(lines) == len(cases)
    keys = ["blocks", "lanes", "pool_bytes", "head_words", "n_big", "big_bytes"]
    return [l if l.startswith("error") else dict(zip(keys, map(int, l.split()))) for l in lines]


def test_the_header_needs_no_hip():
    """every header reachable from ps_search_plan.h is a system header without `hip` in its name or a project header of which the same holds"""
    seen, todo = set(), ["ps_search_plan.h"]
    while todo:
        h = todo.pop()
        if h in seen:
            continue
        seen.add(h)
        for inc in re.findall(r"^\s*#\s*include\s+(\S+)", open(os.path.join(CSRC, h)).read(), re.M):
            assert "hip" not in inc.lower(), (h, inc)
            if inc.startswith('"'):
                todo.append(inc.strip('"'))
    assert {"ps_search_plan.h", "ps_core.h", "ps_model.h"} <= seen


def test_geometry_worked_by_hand(exe):
    assert _run(exe, "lm", 50, 32, 25, 0) == [str(LM)]
    narrow = lambda reads, pool_cap=16384, bt=0, per_cu=4, n_big=4096: (reads, LM, pool_cap, 0, CUS, bt, per_cu, n_big)
    wide = lambda reads: (reads, LM, 2000064, 1, CUS, 0, 4, 4096)
    g = _geometry(exe, [narrow(10_000_000), narrow(156_250), narrow(100), narrow(10_000_000, per_cu=2), narrow(10_000_000, bt=2),
                        narrow(5_000, pool_cap=65535), narrow(10_000_000, pool_cap=65535), wide(87), wide(100_000), narrow(10)])
    # every CU full: 256 CUs x 4 workgroups, 64 GiB of stack exactly (16 B x 16384 entries x 262,144 lanes)
    assert (g[0]["blocks"], g[0]["lanes"], g[0]["pool_bytes"], g[0]["head_words"]) == (1024, 262_144, 68_719_476_736, 0)
    assert (g[1]["blocks"], g[1]["lanes"], g[1]["pool_bytes"]) == (611, 156_416, 41_003_515_904)      # no more workgroups than the reads fill
    assert g[2]["blocks"] == 1
    assert g[3]["blocks"] == 512
    assert g[4]["blocks"] == 2
    # 65,535-entry stacks: 1,048,560 B per lane, 64 GiB hold 65,537 lanes = 256 whole workgroups; no large slots (the stack is as large as one)
    assert (g[5]["blocks"], g[5]["pool_bytes"], g[5]["n_big"], g[5]["big_bytes"]) == (20, 20 * 256 * BIG, 0, 0)
    assert (g[6]["blocks"], g[6]["lanes"], g[6]["n_big"], g[6]["big_bytes"]) == (256, 65_536, 0, 0)
    assert (64 * GiB) // BIG == 65_537
    # wide: 32 B x 2,000,064 + 512 B of heads per lane, 32 GiB / 64,002,560 = 536 lanes = 2 whole workgroups
    assert (g[7]["blocks"], g[7]["lanes"], g[7]["pool_bytes"], g[7]["head_words"], g[7]["n_big"]) == (1, 256, 16_384_524_288, 32_768, 0)
    assert (g[8]["blocks"], g[8]["lanes"]) == (2, 512)
    assert (32 * GiB) // (32 * 2_000_064 + 512) == 536
    # large slots: min(n_big, max(64, reads)), 1,048,560 B each
    assert (g[9]["n_big"], g[9]["big_bytes"]) == (64, 64 * BIG)
    assert (g[0]["n_big"], g[0]["big_bytes"]) == (4096, 4096 * BIG)
    assert _geometry(exe, [narrow(10, n_big=0), narrow(10, n_big=10)])[0]["n_big"] == 0
    assert _geometry(exe, [narrow(1000, n_big=100)])[0]["n_big"] == 100


def test_geometry_errors(exe):
    ok, at, over, wide_over = _geometry(exe, [(1000, 636, 16384, 0, CUS, 0, 4, 4096), (1000, 640, 16384, 0, CUS, 0, 4, 4096),
                                              (1000, 644, 16384, 0, CUS, 0, 4, 4096), (1000, 1000, 2000064, 1, CUS, 8, 4, 4096)])
    assert ok["blocks"] == at["blocks"] == 4                 # one workgroup per CU still fits at 640 B per lane; 1000 reads fill 4
    assert over == LDS_ERROR and wide_over == LDS_ERROR      # also with a stated grid, as before
    # fewer than one workgroup per CU: refused (it used to launch an empty grid); a stated grid does not ask
    zero, neg, stated = _geometry(exe, [(1000, LM, 16384, 0, CUS, 0, 0, 4096), (1000, LM, 16384, 0, CUS, 0, -1, 4096), (1000, LM, 16384, 0, CUS, 3, 0, 4096)])
    assert zero.startswith("error: PS_MAX_PER_CU") and neg.startswith("error: PS_MAX_PER_CU")
    assert stated["blocks"] == 3
    # the LDS lets fewer in than the knob: lm 300 -> 163,840 / 76,800 = 2 per CU
    assert _geometry(exe, [(10_000_000, 300, 64, 0, CUS, 0, 4, 0)])[0]["blocks"] == 512


@pytest.mark.parametrize("cus,bt_blocks,n_big", [(256, 0, 4096), (256, 0, 0), (304, 0, 4096), (256, 7, 100), (8, 0, 4096)])
def test_reservation_equals_first_tier_launch(exe, cus, bt_blocks, n_big):
    caps = [48, 64, 16384, 65535]
    res = [dict(zip(["blocks", "lanes", "pool_bytes", "head_words", "n_big", "big_bytes"], map(int, l.split())))
           for l in _run(exe, "reserve", *[a for c in caps for a in (c, cus, bt_blocks, n_big)])]
    for pool_cap, r in zip(caps, res):
        # reads at or above the lane count (and above n_big), the flagship's LDS state, 4 workgroups per CU
        for reads in (max(r["lanes"], n_big, 64), 10_000_000, 2**31 - 1):
            launch = _geometry(exe, [(reads, LM, pool_cap, 0, cus, bt_blocks, 4, n_big)])[0]
            assert (r["pool_bytes"], r["big_bytes"], r["n_big"], r["lanes"]) == (launch["pool_bytes"], launch["big_bytes"], launch["n_big"], launch["lanes"]), (pool_cap, reads)
        # and they are what the reservation asked for before: 4 workgroups per CU (or the stated grid), bounded by 64 GiB alone
        blocks = bt_blocks or cus * 4
        if blocks * 256 > (64 * GiB) // (pool_cap * 16):
            blocks = max(1, (64 * GiB) // (pool_cap * 16) // 256)
        assert r["pool_bytes"] == blocks * 256 * pool_cap * 16
        assert (r["n_big"], r["big_bytes"]) == ((n_big, n_big * BIG) if pool_cap < 65535 and n_big > 0 else (0, 0))
    # a first tier above 65535 is the wide one: nothing is reserved
    for r in _run(exe, "reserve", 65536, cus, bt_blocks, n_big, 2000064, cus, bt_blocks, n_big):
        assert r.split() == ["0"] * 6


def test_knobs(exe):
    assert _run(exe, "knobs") == ["knobs ok"]


def _cal_maxdiff(l, err, thres):
    """ps_model.h cal_maxdiff (BWA's rule), restated: the same double operations in the same order"""
    elambda = math.exp(-l * err)
    s, y, x = elambda, 1.0, 1
    for k in range(1, 1000):
        y *= l * err
        x = (x * k) & 0xFFFFFFFF
        s += elambda * y / (x - (1 << 32) if x >= 1 << 31 else x)
        if 1.0 - s < thres:
            return k
    return 2


def test_budget_table(exe):
    tabs = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in _run(exe, "table")}     # the driver holds every entry against budget_diffs() itself
    assert sorted(tabs) == ["profile", "profile_X40", "stock_0.04", "stock_2", "stock_300"] and all(len(t) == 256 for t in tabs.values())
    assert tabs["stock_0.04"] == [_cal_maxdiff(l, 0.02, 0.04) for l in range(256)]
    assert tabs["stock_2"] == [2] * 256
    assert tabs["profile"] == [8 * _cal_maxdiff(l, 0.02, 0.04) for l in range(256)]         # 8 units per difference
    assert tabs["profile_X40"] == [255] * 256 and tabs["stock_300"] == [255] * 256           # capped
    # the lengths at which bwa aln's start-up text states a new budget for -n 0.04
    t = tabs["stock_0.04"]
    for length, diffs in ((17, 2), (38, 3), (64, 4), (93, 5), (124, 6), (157, 7), (190, 8), (225, 9)):
        assert (t[length - 1], t[length]) == (diffs - 1 if length > 17 else t[16], diffs), length
