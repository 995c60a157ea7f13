"""The coordinate sort of BAM records on the device (csrc/ps_bamsort.hip: ps_bam_sort_device, PS_BAM_SORT_GPU, ps_bam_sort_records).
The staged call is held to Python's own sorted() (tests/bamsort_inputs.py); every file-writing call is made with the switch off and
on under the same compressor, and the .bam and the .bai must be the same files, byte for byte."""
import os
import signal
import struct
import subprocess
import sys

import numpy as np
import pytest

import bamsort_inputs as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after two minutes at the latest (none takes more than a few seconds)"""
    def over(signum, frame):
        raise TimeoutError("test_gpu_bam_sort: a test ran into its time limit")
    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _sorts_as_python(recs, **kw):
    import capi
    data = b"".join(recs)
    got, st, guard = capi.ps_bam_sort_records(data, device=0, threads=4, guard=64, **kw)
    want = B.python_sorted(recs)
    bad = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
    assert got == want, (len(recs), len(got), len(want), bad)
    assert guard == b"\xee" * 64
    if recs:
        assert (st["on_device"], st["n_calls_device"], st["n_calls_host"], st["n_records"], st["bytes"]) == (1, 1, 0, len(recs), len(data))
    return st


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_records_around_one_wave(n):
    """mixed lengths, ties, unplaced records scattered: the sizes around the 64 records of one wave of the gather, and many groups"""
    rng = np.random.default_rng(0x50F7 + n)
    _sorts_as_python(B.random_records(n, rng))


def _keyed(keys, rng, big_at=None):
    lens = B.mixed_lengths(len(keys), rng)
    return [B.record(ref, pos, 70000 if i == big_at else lens[i], rng) for i, (ref, pos) in enumerate(keys)]


@pytest.mark.parametrize("order", ["equal", "descending", "sorted", "unplaced_interleaved", "all_placed"])
def test_orderings(order):
    rng = np.random.default_rng(0xABC)
    n = 1500
    keys = {"equal": [(3, 77)] * n,                                                    # stability: the input order is the answer
            "descending": [(4 - i * 5 // n, 100000 - i) for i in range(n)],
            "sorted": [(i * 5 // n, i) for i in range(n)],
            "unplaced_interleaved": [(-1, -1) if i & 1 else (i % 3, (i * 7919) % 500) for i in range(n)],
            "all_placed": [(i % 6, (i * 104729) % 0x7fffffff) for i in range(n)]}[order]   # no key has bit 63: the sort stops below 64 bits
    recs = _keyed(keys, rng)
    if order == "equal":
        assert B.python_sorted(recs) == b"".join(recs)
    _sorts_as_python(recs)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_record_larger_than_the_staging(where):
    """a record of 70,000 bytes goes straight through its wave, whatever lies around it"""
    rng = np.random.default_rng(0xB16)
    n = 300
    keys = [(int(rng.integers(0, 3)), int(rng.integers(0, 1000))) for _ in range(n)]
    at = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    keys[at] = {"first": (0, -1), "middle": (1, 500), "last": (-1, -1)}[where]         # where it lands in the output too
    recs = _keyed(keys, rng, big_at=at)
    want = B.python_sorted(recs)
    assert {"first": want[:70000] == recs[at], "middle": True, "last": want[-70000:] == recs[at]}[where]
    _sorts_as_python(recs)


def test_capacity():
    """one byte short fails the call and leaves dst untouched, guard bytes included"""
    import capi
    import ctypes as C
    rng = np.random.default_rng(5)
    recs = B.random_records(65, rng)
    data = b"".join(recs)
    n = len(data)
    dst = C.create_string_buffer(b"\xee" * (n + 64), n + 64)
    assert capi.lib().ps_bam_sort_records(data, n, 0, 4, dst, n - 1, None) == -1
    err = capi.lib().ps_last_error().decode()
    assert str(n) in err and str(n - 1) in err and dst.raw == b"\xee" * (n + 64)
    assert capi.lib().ps_bam_sort_records(data, n, 0, 4, dst, n, None) == n and dst.raw == B.python_sorted(recs) + b"\xee" * 64


@pytest.fixture(scope="module")
def mapped(example, workdir):
    """the 2,000 reads the other GPU tests map, as SAM text and as an unsorted BAM (switches off)"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "bamsort")
    os.makedirs(d)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], 2000, 50, seed=21, indel_scale=30))
    if not os.path.exists(example["fa"] + ".bwt"):
        capi.ps_index(example["fa"])
    capi.ps_bam_sort_device(-1)
    sam, bam = os.path.join(d, "r.sam"), os.path.join(d, "unsorted.bam")
    capi.ps_map(4, "2", None, None, example["fa"], fq, sam)
    capi.ps_map_to_bam(4, "2", None, None, example["fa"], fq, bam)
    return dict(dir=d, fq=fq, fa=example["fa"], sam=sam, bam=bam)


def _off_and_on(write, tag, d):
    """write(path) with the switch off, then on -> the number of device calls of the second; the files must be the same"""
    import capi
    off, on = os.path.join(d, tag + ".off.bam"), os.path.join(d, tag + ".on.bam")
    capi.ps_bam_sort_device(-1)
    write(off)
    assert capi.ps_bam_sort_info()["n_calls_device"] == 0
    capi.ps_bam_sort_device(0)
    try:
        write(on)
        info = capi.ps_bam_sort_info()
    finally:
        capi.ps_bam_sort_device(-1)
    assert open(off, "rb").read() == open(on, "rb").read(), tag
    assert os.path.exists(off + ".bai") == os.path.exists(on + ".bai")
    if os.path.exists(off + ".bai"):
        assert open(off + ".bai", "rb").read() == open(on + ".bai", "rb").read(), tag
    assert info["on_device"] == 1
    return info


def test_the_sorted_stream_stays_on_the_device_for_the_compressor(mapped):
    """both switches on device 0: the stream never comes down (n_resident counts the calls), and every file is the one that the
    device compressor alone writes -- its bytes are a pure function of its input"""
    import capi
    writers = dict(sam=lambda p: capi.ps_sam_to_bam(mapped["sam"], p, sort_by_coordinate=True, write_index=True, threads=4),
                   sort=lambda p: capi.ps_bam_sort(mapped["bam"], p, by_name=False, threads=4),
                   map=lambda p: capi.ps_map_to_bam(4, "2", None, None, mapped["fa"], mapped["fq"], p, sort_by_coordinate=True, write_index=True))
    capi.ps_bgzf_device(0)
    try:
        for k, (tag, write) in enumerate(sorted(writers.items())):
            info = _off_and_on(write, "resident_" + tag, mapped["dir"])
            assert (info["n_calls_device"], info["n_resident"], info["n_calls_host"]) == (1, 1, 0), tag
    finally:
        capi.ps_bgzf_device(-1)
    # the compressor on another device than the sort's (here: off) leaves the stream to come down
    info = _off_and_on(writers["sort"], "not_resident", mapped["dir"])
    assert (info["n_calls_device"], info["n_resident"]) == (1, 0)


def test_sam_to_bam_and_bam_sort_write_the_same_files(mapped):
    import capi
    info = _off_and_on(lambda p: capi.ps_sam_to_bam(mapped["sam"], p, sort_by_coordinate=True, write_index=True, threads=4), "sam", mapped["dir"])
    assert info["n_calls_device"] == 1 and info["n_records"] == 2000 and info["n_calls_host"] == 0 and info["bytes"] > 2000 * 36
    assert os.path.exists(os.path.join(mapped["dir"], "sam.on.bam.bai"))
    info = _off_and_on(lambda p: capi.ps_bam_sort(mapped["bam"], p, by_name=False, threads=4), "sort", mapped["dir"])
    assert info["n_calls_device"] == 1 and info["n_records"] == 2000
    # the records really are in coordinate order, unplaced last (not only equal to the host's)
    import gzip
    stream = gzip.decompress(open(os.path.join(mapped["dir"], "sort.on.bam"), "rb").read())
    l_text = struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, 8 + l_text)[0]
    at = 12 + l_text
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    keys = []
    while at < len(stream):
        bs, ref, pos = struct.unpack_from("<iii", stream, at)
        keys.append((ref & 0xffffffff, pos))
        at += 4 + bs
    assert len(keys) == 2000 and keys == sorted(keys)


@pytest.mark.parametrize("records_on_device", [False, True])
def test_map_to_bam_sorted_and_indexed(mapped, records_on_device):
    import capi
    capi.ps_bam_records_device(records_on_device)
    try:
        info = _off_and_on(lambda p: capi.ps_map_to_bam(4, "2", None, None, mapped["fa"], mapped["fq"], p, sort_by_coordinate=True, write_index=True),
                           "map%d" % records_on_device, mapped["dir"])
    finally:
        capi.ps_bam_records_device(0)
    assert info["n_calls_device"] == 1 and info["n_records"] == 2000


_CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import capi
kind, args = sys.argv[2], sys.argv[3:]
if kind == "route":
    capi.ps_map_route(args[0], args[1], args[2], transcripts_fa=args[3], threads=4)
else:
    capi.ps_bam_sort(args[0], args[1], by_name=False, threads=4)
info = capi.ps_bam_sort_info()
print("INFO", info["on_device"], info["n_calls_device"], info["n_calls_host"], info["n_records"])
"""


def _child(env, *args):
    e = dict(os.environ)
    for k in ("PS_BAM_SORT_GPU", "PS_BAM_SORT_MAX_MB"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "para-suite_amd")] + list(args), env=e, timeout=100, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("INFO")][0].split()[1:]]


def test_map_route_under_the_environment_switch(workdir):
    """the route test's input with transcripts (sorted + indexed passes whose records are kept for the next step, a name-sorted pass):
    every file of a call made in a fresh process with PS_BAM_SORT_GPU=0 is the file of the same call without it"""
    import capi
    import map_route as M
    d = os.path.join(workdir, "bamsort_route")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    for where in ("host", "dev"):
        os.makedirs(os.path.join(d, where))
    capi.ps_bam_sort_device(-1)
    capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "host", "o"), transcripts_fa=data["transcripts_fa"], threads=4)
    assert capi.ps_bam_sort_info()["n_calls_device"] == 0
    on, n_device, n_host, n_records = _child(dict(PS_BAM_SORT_GPU="0"), "route", data["route_fastq"], data["genome_fa"], os.path.join(d, "dev", "o"), data["transcripts_fa"])
    assert on == 1 and n_device >= 1 and n_host == 0 and n_records > 0
    files = sorted(os.listdir(os.path.join(d, "host")))
    assert len([f for f in files if f.endswith(".bam")]) >= 3 and any(f.endswith(".bai") for f in files) and files == sorted(os.listdir(os.path.join(d, "dev")))
    for f in files:
        assert open(os.path.join(d, "host", f), "rb").read() == open(os.path.join(d, "dev", f), "rb").read(), f


def test_name_sort_and_the_memory_bound_stay_on_the_host(mapped):
    import capi
    d = mapped["dir"]
    capi.ps_bam_sort_device(-1)
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "name.off.bam"), by_name=True, threads=4)
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "coord.off.bam"), by_name=False, threads=4)
    capi.ps_bam_sort_device(0)
    try:
        capi.ps_bam_sort(mapped["bam"], os.path.join(d, "name.on.bam"), by_name=True, threads=4)
        info = capi.ps_bam_sort_info()
    finally:
        capi.ps_bam_sort_device(-1)
    assert (info["n_calls_device"], info["n_calls_host"]) == (0, 0)              # the name sort never asks
    assert open(os.path.join(d, "name.off.bam"), "rb").read() == open(os.path.join(d, "name.on.bam"), "rb").read()
    # PS_BAM_SORT_MAX_MB=0: nothing fits, the call goes to the host route and is counted there
    on, n_device, n_host, n_records = _child(dict(PS_BAM_SORT_GPU="0", PS_BAM_SORT_MAX_MB="0"), "sort", mapped["bam"], os.path.join(d, "coord.bound.bam"))
    assert (on, n_device, n_host, n_records) == (1, 0, 1, 0)
    assert open(os.path.join(d, "coord.off.bam"), "rb").read() == open(os.path.join(d, "coord.bound.bam"), "rb").read()


def test_the_switch_refuses_a_missing_device_and_goes_back(mapped):
    import capi
    d = mapped["dir"]
    capi.ps_bam_sort_device(-1)
    assert capi.lib().ps_bam_sort_device(99) != 0 and b"no HIP device 99" in capi.lib().ps_last_error()
    assert capi.ps_bam_sort_info()["on_device"] == 0
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "refused.bam"), by_name=False, threads=4)
    assert capi.ps_bam_sort_info()["n_calls_device"] == 0                         # the failed call changed nothing
    capi.ps_bam_sort_device(0)
    capi.ps_bam_sort_device(-1)
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "back.bam"), by_name=False, threads=4)
    info = capi.ps_bam_sort_info()
    assert (info["on_device"], info["n_calls_device"], info["n_calls_host"]) == (0, 0, 0)
    assert open(os.path.join(d, "back.bam"), "rb").read() == open(os.path.join(d, "refused.bam"), "rb").read()
