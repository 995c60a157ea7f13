"""The name sort of BAM records on the device (csrc/ps_bamsort.hip, csrc/ps_namesort.h: ps_bam_name_sort_device, PS_BAM_NAME_SORT_GPU,
ps_bam_name_sort_records).  The staged call is held to Python's sorted() under a restatement of the samtools rule
(tests/namesort_inputs.py); every file-writing call is made with the switch off and on under the same compressor, and the files must
be the same, byte for byte."""
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import bamsort_inputs as B
import namesort_inputs as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after two minutes at the latest (none takes more than a few seconds)"""
    def over(signum, frame):
        raise TimeoutError("test_gpu_bam_name_sort: a test ran into its time limit")
    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _sorts_as_python(recs, **kw):
    import capi
    data = b"".join(recs)
    got, st, guard = capi.ps_bam_name_sort_records(data, device=0, threads=4, guard=64, **kw)
    want = N.python_sorted(recs)
    bad = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
    assert got == want, (len(recs), len(got), len(want), bad)
    assert guard == b"\xee" * 64
    if recs:
        assert (st["on_device"], st["n_calls_device"], st["n_calls_host"], st["n_records"], st["bytes"]) == (1, 1, 0, len(recs), len(data))
        assert st["key_words"] == N.key_words(max(len(N.name_of(r)) for r in recs)) and st["n_passes"] <= st["key_words"]
    return st


def _named(names, flags, rng, big_at=None):
    lens = B.mixed_lengths(len(names), rng)
    return [N.record(name, flag, 70000 if i == big_at else max(lens[i], 37 + len(name)), rng) for i, (name, flag) in enumerate(zip(names, flags))]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_records_around_one_wave(n):
    """mixed lengths, names of every class, many ties: the sizes around the 64 records of one wave, and many groups"""
    rng = np.random.default_rng(0x4E00 + n)
    _sorts_as_python(N.random_records(n, rng, lengths=B.mixed_lengths(n, rng)))


def _class(order, n, rng):
    """(names, flags) of one class of names; flags None: drawn"""
    pick = lambda pool: [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    forty = b"1234567890" * 4
    if order == "equal":
        return [b"read7/1"] * n, [0x41] * n                                           # stability: the input order is the answer
    if order == "leading_zeros":
        return [(b"r1", b"r01", b"r001")[i % 3] for i in range(n)], [(0x40, 0x80, 0, 0xC0)[i % 4] for i in range(n)]   # ties on the name: the pair bits, then the input order
    if order == "zero_runs":
        return pick([b"a", b"a0", b"a00", b"a0b", b"ab", b"a1b", b"a00b", b"a000"]), None
    if order == "number_lengths":
        return pick([b"r9", b"r10", b"r099", b"r100", b"r0"] + [b"r" + forty[:39] + bytes([0x30 + d]) for d in range(10)] + [b"r" + forty[:38] + b"99"]), None
    if order == "separators":
        seps = b"/.-#+:_AZaz"
        return pick([b"x" + bytes([s]) + b"7" for s in seps] + [b"x7" + bytes([s]) for s in seps] + [b"x7", b"x12", b"x", b"x07/1", b"x7/2", b"x7:1"]), None
    if order == "prefixes":
        return pick([b"ab", b"abc", b"a1", b"a1b", b"a", b"a12", b"abc1"]), None
    if order == "length_extremes":
        return pick([b"a", b"1", b"0", b"/", b"1a" * 127, b"1a" * 126 + b"1", b"1a" * 126 + b"2", b"9" * 254, b"0" * 254, b"x" * 254, b"x" * 253 + b"y"]), None
    if order == "high_bytes":
        return pick([b"r\xc3\xa9" + b"%d" % k for k in (1, 2, 10)] + [b"\xff1", b"\x80", b"\x801", b"r\x7f2", b"r\x802", b"r2", b"r:2", b"\xfe\xff", b"r\xc3"]), None
    ids = [b"read%d" % i for i in range(n)]
    return {"descending": ids[::-1], "sorted": ids}[order], None


@pytest.mark.parametrize("order", ["equal", "leading_zeros", "zero_runs", "number_lengths", "separators", "prefixes", "length_extremes", "high_bytes",
                                   "descending", "sorted"])
def test_name_classes(order):
    rng = np.random.default_rng(0xABC)
    n = 1500
    names, flags = _class(order, n, rng)
    recs = _named(names, [int(f) for f in rng.integers(0, 4096, n)] if flags is None else flags, rng)
    if order in ("equal", "sorted"):
        assert N.python_sorted(recs) == b"".join(recs)
    st = _sorts_as_python(recs)
    if order == "length_extremes":
        assert st["key_words"] == 128                                                  # "1a1a..." fills the row
    if order == "equal":
        assert st["n_passes"] == 0                                                     # no two rows differ anywhere


def test_common_long_prefix_sorts_only_the_columns_that_differ():
    """60 equal bytes, then a number: the fifteen words of the prefix are never sorted.  The expected count comes from the row's
    layout (tests/namesort_inputs.py: row), not from the library"""
    rng = np.random.default_rng(0xC0)
    n = 1500
    names = [b"P" * 60 + b"%d" % ((i * 7919) % 100000) for i in range(n)]
    recs = _named(names, [int(f) for f in rng.integers(0, 4096, n)], rng)
    W, differ = N.columns_that_differ(recs)
    assert W == N.key_words(65) == 34 and 2 <= differ <= W - 15
    st = _sorts_as_python(recs)
    assert (st["key_words"], st["n_passes"]) == (W, differ)


def test_one_record_larger_than_the_staging():
    """one record of 70,000 bytes among 300: the shared gather's straight-through path, reached from this order"""
    rng = np.random.default_rng(0xB16)
    n = 300
    names = [N.random_name(rng) for _ in range(n)]
    recs = _named(names, [int(f) for f in rng.integers(0, 4096, n)], rng, big_at=n // 2)
    assert len(recs[n // 2]) == 70000
    _sorts_as_python(recs)


def test_capacity():
    """one byte short fails the call and leaves dst untouched, guard bytes included"""
    import capi
    import ctypes as C
    rng = np.random.default_rng(5)
    recs = N.random_records(65, rng)
    data = b"".join(recs)
    n = len(data)
    dst = C.create_string_buffer(b"\xee" * (n + 64), n + 64)
    assert capi.lib().ps_bam_name_sort_records(data, n, 0, 4, dst, n - 1, None) == -1
    err = capi.lib().ps_last_error().decode()
    assert str(n) in err and str(n - 1) in err and dst.raw == b"\xee" * (n + 64)
    assert capi.lib().ps_bam_name_sort_records(data, n, 0, 4, dst, n, None) == n and dst.raw == N.python_sorted(recs) + b"\xee" * 64


@pytest.fixture(scope="module")
def mapped(example, workdir):
    """the 2,000 reads the other GPU tests map, as an unsorted BAM (switches off), and its name-sorted form by the host route"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "bamnamesort")
    os.makedirs(d)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], 2000, 50, seed=21, indel_scale=30))
    if not os.path.exists(example["fa"] + ".bwt"):
        capi.ps_index(example["fa"])
    capi.ps_bam_sort_device(-1)
    capi.ps_bam_name_sort_device(-1)
    bam, off = os.path.join(d, "unsorted.bam"), os.path.join(d, "name.off.bam")
    capi.ps_map_to_bam(4, "2", None, None, example["fa"], fq, bam)
    capi.ps_bam_sort(bam, off, by_name=True, threads=4)
    assert capi.ps_bam_name_sort_info()["n_calls_device"] == 0
    return dict(dir=d, fq=fq, fa=example["fa"], bam=bam, off=off)


def _same(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def test_bam_sort_by_name_writes_the_same_file(mapped):
    import capi
    on = os.path.join(mapped["dir"], "name.on.bam")
    capi.ps_bam_name_sort_device(0)
    try:
        capi.ps_bam_sort(mapped["bam"], on, by_name=True, threads=4)
        info, coord = capi.ps_bam_name_sort_info(), capi.ps_bam_sort_info()
    finally:
        capi.ps_bam_name_sort_device(-1)
    assert _same(mapped["off"], on)
    assert (info["on_device"], info["n_calls_device"], info["n_calls_host"], info["n_records"], info["n_resident"]) == (1, 1, 0, 2000, 0)
    assert info["key_words"] >= 2 and 1 <= info["n_passes"] <= info["key_words"] and info["bytes"] > 2000 * 36
    assert (coord["on_device"], coord["n_calls_device"], coord["n_calls_host"]) == (0, 0, 0)    # the coordinate switch saw nothing of it
    assert capi.ps_bam_name_sort_info()["n_calls_device"] == 0                                  # switching off started the counters again
    # the names really are in order (not only equal to the host's)
    import gzip
    import struct
    stream = gzip.decompress(open(on, "rb").read())
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 12 + l_text
    for _ in range(struct.unpack_from("<i", stream, 8 + l_text)[0]):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    recs = []
    while at < len(stream):
        bs = struct.unpack_from("<i", stream, at)[0]
        recs.append(stream[at:at + 4 + bs])
        at += 4 + bs
    assert len(recs) == 2000 and all(N.record_cmp(recs[i], recs[i + 1]) <= 0 for i in range(1999))


_CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import capi
kind, args = sys.argv[2], sys.argv[3:]
if kind == "route":
    capi.ps_map_route(args[0], args[1], args[2], transcripts_fa=args[3], threads=4)
else:
    capi.ps_bam_sort(args[0], args[1], by_name=True, threads=4)
info = capi.ps_bam_name_sort_info()
print("INFO", info["on_device"], info["n_calls_device"], info["n_calls_host"], info["n_records"], capi.ps_bam_sort_info()["n_calls_device"])
"""


def _env(env):
    e = dict(os.environ)
    for k in ("PS_BAM_SORT_GPU", "PS_BAM_NAME_SORT_GPU", "PS_BAM_SORT_MAX_MB", "PS_BGZF_GPU", "PS_VERBOSE"):
        e.pop(k, None)
    e.update(env)
    return e


def _child(env, *args):
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "para-suite_amd")] + list(args), env=_env(env), timeout=100, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("INFO")][0].split()[1:]]


def test_samtools_sort_n_under_the_environment_switch(mapped):
    """the shim takes the switch from the environment: the same file, and the stage line names the route"""
    exe = os.path.join(ROOT, "para-suite_amd", "bin", "samtools")
    out = os.path.join(mapped["dir"], "name.shim.bam")
    r = subprocess.run([exe, "sort", "-n", "-@", "4", "-o", out, mapped["bam"]], env=_env(dict(PS_BAM_NAME_SORT_GPU="0", PS_VERBOSE="1")), timeout=100,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _same(mapped["off"], out)
    assert "bam name sort: 2000 records" in r.stderr and "ms (device)" in r.stderr, r.stderr[-2000:]


def test_map_route_under_the_environment_switch(workdir):
    """the input of test_gpu_bam_sort's route test, with transcripts (its transcript pass is name-sorted): every file of a call made
    in a fresh process with PS_BAM_NAME_SORT_GPU=0 is the file of the same call without it"""
    import capi
    import map_route as M
    d = os.path.join(workdir, "bamnamesort_route")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    for where in ("host", "dev"):
        os.makedirs(os.path.join(d, where))
    capi.ps_bam_name_sort_device(-1)
    capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "host", "o"), transcripts_fa=data["transcripts_fa"], threads=4)
    assert capi.ps_bam_name_sort_info()["n_calls_device"] == 0
    on, n_device, n_host, n_records, n_coordinate = _child(dict(PS_BAM_NAME_SORT_GPU="0"), "route", data["route_fastq"], data["genome_fa"], os.path.join(d, "dev", "o"), data["transcripts_fa"])
    assert on == 1 and n_device >= 1 and n_host == 0 and n_records > 0 and n_coordinate == 0
    files = sorted(os.listdir(os.path.join(d, "host")))
    assert len([f for f in files if f.endswith(".bam")]) >= 3 and files == sorted(os.listdir(os.path.join(d, "dev")))
    for f in files:
        assert _same(os.path.join(d, "host", f), os.path.join(d, "dev", f)), f


def test_the_sorted_stream_stays_on_the_device_for_the_compressor(mapped):
    """both switches on device 0: the stream never comes down, and the file is the one that the BGZF switch alone writes"""
    import capi
    d = mapped["dir"]
    alone, both = os.path.join(d, "name.bgzf.bam"), os.path.join(d, "name.resident.bam")
    capi.ps_bgzf_device(0)
    try:
        capi.ps_bam_sort(mapped["bam"], alone, by_name=True, threads=4)
        capi.ps_bam_name_sort_device(0)
        try:
            capi.ps_bam_sort(mapped["bam"], both, by_name=True, threads=4)
            info = capi.ps_bam_name_sort_info()
        finally:
            capi.ps_bam_name_sort_device(-1)
    finally:
        capi.ps_bgzf_device(-1)
    assert (info["n_calls_device"], info["n_resident"], info["n_calls_host"]) == (1, 1, 0)
    assert _same(alone, both)


def test_the_memory_bound_sends_the_call_to_the_host(mapped):
    """PS_BAM_SORT_MAX_MB=1: the call does not fit, goes to the host route and is counted there; the file is the same"""
    out = os.path.join(mapped["dir"], "name.bound.bam")
    on, n_device, n_host, n_records, _ = _child(dict(PS_BAM_NAME_SORT_GPU="0", PS_BAM_SORT_MAX_MB="1"), "sort", mapped["bam"], out)
    assert (on, n_device, n_host, n_records) == (1, 0, 1, 0)
    assert _same(mapped["off"], out)


def test_the_switch_refuses_a_missing_device_and_goes_back(mapped):
    import capi
    d = mapped["dir"]
    capi.ps_bam_name_sort_device(-1)
    assert capi.lib().ps_bam_name_sort_device(99) != 0 and b"no HIP device 99" in capi.lib().ps_last_error()
    assert capi.ps_bam_name_sort_info()["on_device"] == 0
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "refused.bam"), by_name=True, threads=4)
    assert capi.ps_bam_name_sort_info()["n_calls_device"] == 0                    # the failed call changed nothing
    capi.ps_bam_name_sort_device(0)
    capi.ps_bam_name_sort_device(-1)
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "back.bam"), by_name=True, threads=4)
    info = capi.ps_bam_name_sort_info()
    assert (info["on_device"], info["n_calls_device"], info["n_calls_host"]) == (0, 0, 0)
    assert _same(mapped["off"], os.path.join(d, "back.bam")) and _same(mapped["off"], os.path.join(d, "refused.bam"))


def test_each_sort_asks_its_own_switch_only(mapped):
    """the coordinate switch alone: a name sort leaves both infos at zero device calls; the name switch alone: so does a coordinate sort"""
    import capi
    d = mapped["dir"]
    capi.ps_bam_sort_device(0)
    try:
        capi.ps_bam_sort(mapped["bam"], os.path.join(d, "name.coord_switch.bam"), by_name=True, threads=4)
        coord, name = capi.ps_bam_sort_info(), capi.ps_bam_name_sort_info()
    finally:
        capi.ps_bam_sort_device(-1)
    assert (coord["n_calls_device"], coord["n_calls_host"]) == (0, 0) and (name["on_device"], name["n_calls_device"], name["n_calls_host"]) == (0, 0, 0)
    assert _same(mapped["off"], os.path.join(d, "name.coord_switch.bam"))
    capi.ps_bam_sort(mapped["bam"], os.path.join(d, "coord.off.bam"), by_name=False, threads=4)
    capi.ps_bam_name_sort_device(0)
    try:
        capi.ps_bam_sort(mapped["bam"], os.path.join(d, "coord.name_switch.bam"), by_name=False, threads=4)
        coord, name = capi.ps_bam_sort_info(), capi.ps_bam_name_sort_info()
    finally:
        capi.ps_bam_name_sort_device(-1)
    assert (coord["on_device"], coord["n_calls_device"], coord["n_calls_host"]) == (0, 0, 0) and (name["n_calls_device"], name["n_calls_host"]) == (0, 0)
    assert _same(os.path.join(d, "coord.off.bam"), os.path.join(d, "coord.name_switch.bam"))
