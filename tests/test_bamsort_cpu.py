"""The coordinate sort of BAM records as csrc/ps_bamsort.h states it for host and device, without a device.  tests/bamsort_check.cpp
is the header (with csrc/ps_bam.cpp, which links alone with zlib) under the host compiler, built with AddressSanitizer and UBSan as
a plain executable: the key's order against the library's comparator, the gather's 64 lanes run one after the other on exact-size
heap buffers, a swapped pair as the negative control, and the host functions of the device route's staging (the piece knob, the column
layout, the upload's cut).  The library's host route behind ps_bam_sort_records (no sanitizer: it is
loaded into Python) is held to Python's own sorted()."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bamsort_inputs as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bamsort") / "bamsort_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "bamsort_check.cpp"), os.path.join(CSRC, "ps_bam.cpp"), "-o", exe, "-lz", "-lpthread"])
    r = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def test_key_order_is_the_comparator_of_sort_records(check_output):
    line = [l for l in check_output if l.startswith("keys ok")]
    assert line and "20000 records" in line[0] and "end bit 64" in line[0], check_output


def test_gather_lane_by_lane(check_output):
    line = [l for l in check_output if l.startswith("gather ok")]
    assert line and "all 256 pairs" in line[0], check_output
    assert int(line[0].split()[4]) >= 16 * 1065


def test_a_swapped_pair_fails_the_comparison(check_output):
    assert any(l.startswith("swap ok") for l in check_output) and check_output[-1] == "all ok"


def test_the_piece_knob_clamps_as_documented(check_output):
    """PS_BAM_SORT_PIECE: unset, empty, not a number, <= 0, below 256, not a multiple of 64, the default and above"""
    assert "piece knob ok: 16 values" in check_output, check_output


def test_the_column_sub_arrays_fit_their_half(check_output):
    """every piece size from 256 to 8192 in steps of 64, and the default: four arrays, disjoint, inside the half, aligned"""
    assert "column layout ok: %d piece sizes and the default" % len(range(256, 8193, 64)) in check_output, check_output


def test_the_upload_cut_tiles_the_parts(check_output):
    """run_route's upload loop replayed over the header's cut: empty parts, parts that end on a piece boundary, parts of many pieces"""
    line = [l for l in check_output if l.startswith("upload cut ok")]
    assert line and int(line[0].split()[3]) >= 3 * 13 + 200, check_output


@pytest.mark.parametrize("n", [0, 1, 65, 3000])
def test_host_route_equals_python_sorted(n):
    import capi
    rng = np.random.default_rng(0xB50 + n)
    recs = B.random_records(n, rng, big_at=n // 2 if n > 100 else None)
    recs += [B.record(0, 0x7fffffff, 40, rng), B.record(70000, 0, 41, rng), B.record(0, 0, 36, rng)] if n else []
    data = b"".join(recs)
    got, st, guard = capi.ps_bam_sort_records(data, device=-1, threads=3, guard=64)
    assert got == B.python_sorted(recs) and guard == b"\xee" * 64
    assert (st["n_records"], st["bytes"], st["n_calls_host"], st["n_calls_device"], st["on_device"]) == ((len(recs), len(data), 1, 0, 0) if n else (0, 0, 0, 0, 0))


def test_bad_records_are_refused_with_their_number():
    import capi
    rng = np.random.default_rng(7)
    recs = B.random_records(10, rng)
    data = b"".join(recs)
    n = len(data)
    L = capi.lib()

    def refused(buf, cap=None):
        dst = C.create_string_buffer(b"\xee" * n, n)
        assert L.ps_bam_sort_records(buf, len(buf), -1, 2, dst, n if cap is None else cap, None) == -1 and dst.raw == b"\xee" * n
        return L.ps_last_error().decode()

    assert "record 10 runs past" in refused(data[:-1])
    assert "record 10 runs past" in refused(data[:-len(recs[9]) + 2])          # not even a whole block_size
    at = sum(len(r) for r in recs[:4])
    err = refused(data[:at] + struct.pack("<i", 8) + data[at + 4:])
    assert "record 5 " in err and "block_size of 8" in err
    err = refused(data, cap=n - 1)
    assert str(n) in err and str(n - 1) in err
    st = capi.BamSortStats(struct_size=8)
    assert L.ps_bam_sort_records(data, n, -1, 2, C.create_string_buffer(n), n, C.byref(st)) == -1 and b"struct_size" in L.ps_last_error()
