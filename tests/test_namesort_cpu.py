"""The name order of BAM records as csrc/ps_namesort.h states it for host and device, without a device.  tests/namesort_check.cpp is
the header (with csrc/ps_bam.cpp, which links alone with zlib) under the host compiler, built with AddressSanitizer and UBSan as a
plain executable: the rows' order against the library's comparator -- every pair of short names, a million random pairs --, the
key's length, the column passes against the host route, and a swapped pair as the negative control.  The library's host route behind
ps_bam_name_sort_records (no sanitizer: it is loaded into Python) is held to Python's sorted() under a restatement of the rule."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bamsort_inputs as B
import namesort_inputs as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("namesort") / "namesort_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "namesort_check.cpp"), os.path.join(CSRC, "ps_bam.cpp"), "-o", exe, "-lz", "-lpthread"])
    r = subprocess.run([exe], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def test_every_pair_of_short_names(check_output):
    line = [l for l in check_output if l.startswith("exhaustive ok")]
    assert line and "1555 names" in line[0] and "%d ordered pairs" % (1555 * 1555) in line[0], check_output


def test_a_million_random_pairs(check_output):
    line = [l for l in check_output if l.startswith("random ok")]
    assert line and "1000000 pairs" in line[0], check_output


def test_key_length(check_output):
    line = [l for l in check_output if l.startswith("length ok")]
    assert line and "reached by 127 names" in line[0], check_output          # the odd lengths from 1 to 253


def test_column_passes_and_a_swapped_pair(check_output):
    assert any(l.startswith("order ok: 3000 records") for l in check_output)
    assert any(l.startswith("swap ok") for l in check_output) and check_output[-1] == "all ok"


def test_the_python_row_orders_as_the_python_rule():
    """the two restatements of tests/namesort_inputs.py against each other: the GPU tests take their expected pass count from one and
    their expected order from the other"""
    rng = np.random.default_rng(0x4E53)
    names = [N.random_name(rng) for _ in range(400)] + [b"", b"a0", b"a00", b"a", b"a0b", b"ab", b"a1b", b"r9", b"r10", b"r099"]
    W = N.key_words(max(len(x) for x in names))
    rows = [N.row(x, 0, W) for x in names]
    sign = lambda v: (v > 0) - (v < 0)
    for i in range(0, len(names), 3):
        for j in range(len(names)):
            assert sign(N.name_cmp(names[i], names[j])) == sign((rows[i] > rows[j]) - (rows[i] < rows[j])), (names[i], names[j])
    assert N.key_words(3) == 3 and N.row(b"1a1", 0xC0, 3) == (0x30013161, 0x30013100, 3) and N.key_words(254) == 128 and N.key_words(0) == 1


@pytest.mark.parametrize("n", [0, 1, 65, 3000])
def test_host_route_equals_python_sorted(n):
    import capi
    rng = np.random.default_rng(0x4A50 + n)
    recs = N.random_records(n, rng, lengths=B.mixed_lengths(n, rng))
    recs += [N.record(b"1a" * 126 + b"1", 0x40, 300, rng), N.record(b"", 0x80, 37, rng), N.record(b"x" * 254, 0, 36 + 255, rng)] if n else []
    data = b"".join(recs)
    got, st, guard = capi.ps_bam_name_sort_records(data, device=-1, threads=3, guard=64)
    assert got == N.python_sorted(recs) and guard == b"\xee" * 64
    assert (st["n_records"], st["bytes"], st["n_calls_host"], st["n_calls_device"], st["on_device"]) == ((len(recs), len(data), 1, 0, 0) if n else (0, 0, 0, 0, 0))


def test_bad_records_are_refused_with_their_number():
    import capi
    rng = np.random.default_rng(7)
    recs = N.random_records(10, rng)
    data = b"".join(recs)
    n = len(data)
    L = capi.lib()

    def refused(buf, cap=None):
        dst = C.create_string_buffer(b"\xee" * n, n)
        assert L.ps_bam_name_sort_records(buf, len(buf), -1, 2, dst, n if cap is None else cap, None) == -1 and dst.raw == b"\xee" * n
        return L.ps_last_error().decode()

    assert "record 10 runs past" in refused(data[:-1])
    assert "record 10 runs past" in refused(data[:-len(recs[9]) + 2])          # not even a whole block_size
    at = sum(len(r) for r in recs[:4])
    err = refused(data[:at] + struct.pack("<i", 8) + data[at + 4:])
    assert "record 5 " in err and "block_size of 8" in err
    # a name that does not end inside its record: no NUL where byte 12 says, no name at all, a length that reaches past the record
    l_name = recs[4][12]
    for bad in (recs[4][:36 + l_name - 1] + b"x" + recs[4][36 + l_name:], recs[4][:12] + b"\0" + recs[4][13:], N.record(b"", 0, 37, rng)[:12] + b"\x09" + N.record(b"", 0, 37, rng)[13:]):
        err = refused(data[:at] + bad + data[at + len(recs[4]):])
        assert "record 5 " in err and "name" in err, err
    err = refused(data, cap=n - 1)
    assert str(n) in err and str(n - 1) in err
    st = capi.BamNameSortStats(struct_size=8)
    assert L.ps_bam_name_sort_records(data, n, -1, 2, C.create_string_buffer(n), n, C.byref(st)) == -1 and b"struct_size" in L.ps_last_error()
