"""The host-side streaming around the device BAM sort and compressor, at its seams (csrc/ps_bamsort.hip: run_route and Stager;
csrc/ps_bgzf.hip: compress_rounds).  PS_BAM_SORT_PIECE cuts the sort's page-locked staging into halves of 256, 320 and 4,096 bytes, so
that the upload, the column pieces and both downloads run many times and cuts fall inside records, their 36-byte fixed parts and their
names; PS_BGZF_PIECE=65280 takes the resident stream through the compressor one block per round; and all four device switches are
turned on at once.  The oracles are the ones the other files use: Python's sorted() (tests/bamsort_inputs.py, tests/namesort_inputs.py)
and the host route's files."""
import gzip
import json
import os
import signal
import struct
import subprocess
import sys

import numpy as np
import pytest

import bamsort_inputs as B
import bgzf_inputs as Z
import namesort_inputs as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ["coordinate", "name"]


@pytest.fixture(autouse=True)
def time_limit():
    """every test of this file ends after two minutes at the latest (none takes more than a few seconds)"""
    def over(signum, frame):
        raise TimeoutError("test_gpu_bam_seams: a test ran into its time limit")
    old = signal.signal(signal.SIGALRM, over)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(autouse=True)
def switches_off():
    """every test starts and ends with the four switches off, whatever it did"""
    import capi

    def off():
        capi.ps_bam_records_device(0)
        capi.ps_bam_sort_device(-1)
        capi.ps_bam_name_sort_device(-1)
        capi.ps_bgzf_device(-1)
    off()
    yield
    off()


# ---------------------------------------------------------------- a, b: the staged calls
def _records(order, lengths, rng):
    """one record per length: keys with many ties and unplaced records for the coordinate order, names of every class for the name
    order (a name that needs more room than the length gives is cut to fit: the length is what the test is about)"""
    out = []
    for length in lengths:
        if order == "coordinate":
            ref, pos = (-1, -1) if rng.random() < 0.1 else (int(rng.integers(0, 5)), int(rng.integers(0, 400)))
            out.append(B.record(ref, pos, length, rng))
        else:
            assert length >= 37
            out.append(N.record(N.random_name(rng, max_len=min(40, length - 37)), int(rng.integers(0, 4096)), length, rng))
    return out


def _sorts_as_python(order, recs, piece, monkeypatch):
    import capi
    monkeypatch.setenv("PS_BAM_SORT_PIECE", str(piece))
    call, oracle = {"coordinate": (capi.ps_bam_sort_records, B.python_sorted), "name": (capi.ps_bam_name_sort_records, N.python_sorted)}[order]
    data = b"".join(recs)
    got, st, guard = call(data, device=0, threads=4, guard=64)
    want = oracle(recs)
    bad = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
    assert got == want, (order, piece, len(recs), len(got), len(want), bad)
    assert guard == b"\xee" * 64
    assert (st["on_device"], st["n_calls_device"], st["n_calls_host"], st["n_records"], st["bytes"]) == (1, 1, 0, len(recs), len(data))
    return st


@pytest.mark.parametrize("n", [1, 12, 13, 64, 65, 129, 1500])
@pytest.mark.parametrize("piece", [256, 320, 4096])
@pytest.mark.parametrize("order", ORDERS)
def test_forced_seams(order, piece, n, monkeypatch):
    """mixed lengths through halves of `piece` bytes.  At 256 bytes a column piece holds 12 records, so 12 and 13 straddle it; the
    permutation (4 n bytes) comes down in 1, 2 and 3 pieces at 64, 65 and 129 records, so the stream's first piece lands on either
    half and the piece carried over from the permutation's download is of both parities"""
    rng = np.random.default_rng(0x5EA0 + 7 * n + piece)
    lengths = [max(l, 37) if order == "name" else l for l in B.mixed_lengths(n, rng)]
    recs = _records(order, lengths, rng)
    if n >= 64:
        assert len(b"".join(recs)) > 2 * piece                                       # both halves are used more than once
    _sorts_as_python(order, recs, piece, monkeypatch)


@pytest.mark.parametrize("order", ORDERS)
def test_records_that_end_on_the_cuts(order, monkeypatch):
    """halves of 256 bytes and 64 records of exactly 64: every fourth record ends on a cut of the upload and of the stream's download"""
    P = 256
    rng = np.random.default_rng(0xC075)
    recs = _records(order, [P // 4] * 64, rng)
    assert len(b"".join(recs)) == 16 * P
    _sorts_as_python(order, recs, P, monkeypatch)


@pytest.mark.parametrize("order", ORDERS)
def test_records_one_byte_off_the_cuts(order, monkeypatch):
    """the same 64 records with one of 255 and one of 257 bytes among them: every record behind them is shifted off the cuts"""
    P = 256
    rng = np.random.default_rng(0xC075)
    recs = _records(order, [P // 4] * 64, rng)
    short, long_ = _records(order, [P - 1, P + 1], rng)
    recs = recs[:5] + [short] + recs[5:20] + [long_] + recs[20:]
    assert len(recs) == 66 and len(b"".join(recs)) == 18 * P
    _sorts_as_python(order, recs, P, monkeypatch)


@pytest.mark.parametrize("order", ORDERS)
def test_one_record_of_many_pieces(order, monkeypatch):
    """a record of 70,000 bytes (about 273 halves of 256 bytes) among 300 small ones"""
    rng = np.random.default_rng(0xB16)
    lengths = [max(l, 37) for l in B.mixed_lengths(301, rng)]
    lengths[150] = 70000
    recs = _records(order, lengths, rng)
    assert len(recs[150]) == 70000
    _sorts_as_python(order, recs, 256, monkeypatch)


# ---------------------------------------------------------------- c, d: the file writers
@pytest.fixture(scope="module")
def mapped(example, workdir):
    """the 2,000 reads the other GPU tests map, as SAM text and as an unsorted BAM (switches off); a SAM of its first three records"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "bamseams")
    os.makedirs(d)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], 2000, 50, seed=21, indel_scale=30))
    if not os.path.exists(example["fa"] + ".bwt"):
        capi.ps_index(example["fa"])
    sam, bam, sam3 = os.path.join(d, "r.sam"), os.path.join(d, "unsorted.bam"), os.path.join(d, "three.sam")
    capi.ps_bam_sort_device(-1)
    capi.ps_bam_name_sort_device(-1)
    capi.ps_bgzf_device(-1)
    capi.ps_map(4, "2", None, None, example["fa"], fq, sam)
    capi.ps_map_to_bam(4, "2", None, None, example["fa"], fq, bam)
    lines = open(sam).read().split("\n")
    head, recs = [l for l in lines if l.startswith("@")], [l for l in lines if l and not l.startswith("@")]
    assert len(recs) == 2000
    with open(sam3, "w") as f:
        f.write("\n".join(head + recs[:3]) + "\n")
    return dict(dir=d, fq=fq, fa=example["fa"], sam=sam, bam=bam, sam3=sam3)


def _profile():
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    return P


@pytest.fixture(scope="module")
def mid_input(mid, workdir):
    """the 30,000 ragged reads of test_gpu_bam_records.py's mid_input, drawn the same way"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "bamseams_mid")
    os.makedirs(d)
    sim = S.simulate_reads(mid["genome"], n_reads=30000, read_len=50, seed=91, indel_scale=30, n_frac=0.002, min_len=28)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, sim)
    ep, ip = os.path.join(d, "p.errorprofile"), os.path.join(d, "p.indelprofile")
    with open(ep, "w") as f:
        for row in _profile():
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    open(ip, "w").write("2.1E-5\t5.9E-4")
    if not os.path.exists(mid["fa"] + ".bwt"):
        capi.ps_index(mid["fa"])
    return dict(dir=d, fq=fq, ep=ep, ip=ip, fa=mid["fa"])


def _same_files(a, b, tag):
    assert open(a, "rb").read() == open(b, "rb").read(), tag
    assert os.path.exists(a + ".bai") == os.path.exists(b + ".bai"), tag
    if os.path.exists(a + ".bai"):
        assert open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read(), tag


def _off_and_on(write, tag, d, by_name=False):
    """write(path) with the sort's switch off, then on -> the info of the second; the .bam and the .bai must be the same files"""
    import capi
    switch, info_of = (capi.ps_bam_name_sort_device, capi.ps_bam_name_sort_info) if by_name else (capi.ps_bam_sort_device, capi.ps_bam_sort_info)
    off, on = os.path.join(d, tag + ".off.bam"), os.path.join(d, tag + ".on.bam")
    switch(-1)
    write(off)
    assert info_of()["n_calls_device"] == 0
    switch(0)
    try:
        write(on)
        info = info_of()
    finally:
        switch(-1)
    _same_files(off, on, tag)
    assert info["on_device"] == 1
    return info


def test_the_file_writers_with_forced_seams(mapped, monkeypatch):
    """halves of 4,096 bytes: the parts of four threads, each of many pieces, through every writer that sorts"""
    import capi
    monkeypatch.setenv("PS_BAM_SORT_PIECE", "4096")
    d = mapped["dir"]
    info = _off_and_on(lambda p: capi.ps_sam_to_bam(mapped["sam"], p, sort_by_coordinate=True, write_index=True, threads=4), "sam", d)
    assert (info["n_calls_device"], info["n_calls_host"], info["n_records"]) == (1, 0, 2000) and info["bytes"] > 20 * 4096
    assert os.path.exists(os.path.join(d, "sam.on.bam.bai"))
    info = _off_and_on(lambda p: capi.ps_bam_sort(mapped["bam"], p, by_name=False, threads=4), "coord", d)
    assert (info["n_calls_device"], info["n_calls_host"], info["n_records"]) == (1, 0, 2000)
    info = _off_and_on(lambda p: capi.ps_bam_sort(mapped["bam"], p, by_name=True, threads=4), "name", d, by_name=True)
    assert (info["n_calls_device"], info["n_calls_host"], info["n_records"]) == (1, 0, 2000)
    # three records on four threads: some parts are empty
    info = _off_and_on(lambda p: capi.ps_sam_to_bam(mapped["sam3"], p, sort_by_coordinate=True, write_index=True, threads=4), "three", d)
    assert (info["n_calls_device"], info["n_calls_host"], info["n_records"]) == (1, 0, 3)


def test_map_to_bam_in_several_parts_of_many_pieces(mid_input, monkeypatch):
    """30,000 ragged reads mapped in chunks of 1 MB: several parts, each of many halves of 4,096 bytes; sorted and indexed"""
    import capi
    monkeypatch.setenv("PS_BAM_SORT_PIECE", "4096")
    monkeypatch.setenv("PS_CHUNK_MB", "1")
    m = mid_input
    stats = []
    info = _off_and_on(lambda p: stats.append(capi.ps_map_to_bam(8, "-1", m["ep"], m["ip"], m["fa"], m["fq"], p, sort_by_coordinate=True, write_index=True)), "map", m["dir"])
    assert stats[0] == stats[1] and stats[1]["n_in"] == 30000 and stats[1]["n_out"] > 20000
    assert (info["n_calls_device"], info["n_calls_host"], info["n_records"]) == (1, 0, stats[1]["n_out"]) and info["bytes"] > 100 * 4096


def _body_sizes(bam):
    """the uncompressed sizes of the BGZF blocks between the header's and the end-of-file block"""
    raw = open(bam, "rb").read()
    ms = Z.members(raw)
    stream = gzip.decompress(raw)
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 12 + l_text
    for _ in range(struct.unpack_from("<i", stream, 8 + l_text)[0]):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    sizes = [int.from_bytes(m[-4:], "little") for m in ms]
    assert sizes[0] == at and sizes[-1] == 0                                      # the header has a block of its own; the file ends with the empty one
    assert sum(sizes) == len(stream)
    return sizes[1:-1]


def test_the_resident_stream_in_more_than_one_round(mapped, monkeypatch):
    """both switches on device 0 and one block per launch of the compressor: round r reads the stream where it lies, r blocks in.
    The files are the ones the compressor alone writes with no knob set -- its bytes are a pure function of its input"""
    import capi
    d = mapped["dir"]
    writers = dict(sort=lambda p: capi.ps_bam_sort(mapped["bam"], p, by_name=False, threads=4),
                   sam=lambda p: capi.ps_sam_to_bam(mapped["sam"], p, sort_by_coordinate=True, write_index=True, threads=4))
    for tag, write in sorted(writers.items()):
        alone, both = os.path.join(d, "rounds_%s.alone.bam" % tag), os.path.join(d, "rounds_%s.both.bam" % tag)
        capi.ps_bgzf_device(0)
        write(alone)
        assert capi.ps_bam_sort_info()["n_calls_device"] == 0
        with monkeypatch.context() as mp:
            mp.setenv("PS_BGZF_PIECE", str(Z.BLK))
            mp.setenv("PS_BAM_SORT_PIECE", "4096")
            capi.ps_bam_sort_device(0)
            try:
                write(both)
                info = capi.ps_bam_sort_info()
            finally:
                capi.ps_bam_sort_device(-1)
        capi.ps_bgzf_device(-1)
        assert (info["n_calls_device"], info["n_resident"], info["n_calls_host"], info["n_records"]) == (1, 1, 0, 2000), tag
        sizes = _body_sizes(both)
        assert len(sizes) >= 3 and all(s == Z.BLK for s in sizes[:-1]) and 0 < sizes[-1] < Z.BLK, (tag, sizes)
        _same_files(alone, both, tag)


def test_the_device_buffer_changes_owner_twice(mapped):
    """the stream's buffer leaves the sort's set for the body of a file and comes back, across a switch that goes off and on: a
    resident write, the sort's switch off (its buffers are given back) and on, a second resident write, then the compressor's switch
    off and a third write, whose stream comes down.  Every file holds the host route's records, and its index says the same about them"""
    import capi
    d = mapped["dir"]
    write = lambda p: capi.ps_sam_to_bam(mapped["sam"], p, sort_by_coordinate=True, write_index=True, threads=4)
    host, first, second, third = (os.path.join(d, "owner.%s.bam" % t) for t in ("host", "first", "second", "third"))
    st_host = write(host)
    assert capi.ps_bam_sort_info()["n_calls_device"] == 0
    capi.ps_bgzf_device(0)
    capi.ps_bam_sort_device(0)
    st_first, info_first = write(first), capi.ps_bam_sort_info()
    capi.ps_bam_sort_device(-1)
    assert capi.ps_bam_sort_info()["on_device"] == 0
    capi.ps_bam_sort_device(0)
    assert capi.ps_bam_sort_info()["n_calls_device"] == 0                          # the counters start again with the switch
    st_second, info_second = write(second), capi.ps_bam_sort_info()
    capi.ps_bgzf_device(-1)
    st_third, info_third = write(third), capi.ps_bam_sort_info()
    capi.ps_bam_sort_device(-1)
    counters = lambda i: (i["on_device"], i["n_calls_device"], i["n_calls_host"], i["n_resident"], i["n_records"])
    assert counters(info_first) == (1, 1, 0, 1, 2000) and counters(info_second) == (1, 1, 0, 1, 2000)      # resident, resident
    assert counters(info_third) == (1, 2, 0, 1, 4000)                                                      # and not resident
    want, want_bai = open(host, "rb").read(), open(host + ".bai", "rb").read()
    for path, st in ((first, st_first), (second, st_second)):
        got = open(path, "rb").read()
        assert got != want and gzip.decompress(got) == gzip.decompress(want), path
        assert _bai_over_the_stream(open(path + ".bai", "rb").read(), got) == _bai_over_the_stream(want_bai, want), path
        assert (st["n_in"], st["n_out"]) == (st_host["n_in"], st_host["n_out"]) == (2000, 2000)
    _same_files(host, third, "third")                                              # zlib again: the host route's very files
    assert st_third == st_host


# ---------------------------------------------------------------- e: everything on at once
_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import capi
capi.ps_map_route(sys.argv[2], sys.argv[3], sys.argv[4], transcripts_fa=sys.argv[5], threads=4)
print("INFO", json.dumps(dict(records=capi.ps_bam_records_info(), sort=capi.ps_bam_sort_info(), name=capi.ps_bam_name_sort_info())))
"""


def _bai_over_the_stream(bai, bam):
    """a .bai with every virtual file offset (block start << 16 | byte in the block) replaced by the position in the inflated stream
    that it names: what the index says about the records, whatever the compressor made of the blocks.  Everything else as it is."""
    starts, at, pos = {}, 0, 0
    for m in Z.members(bam):
        starts[at] = pos
        at += len(m)
        pos += int.from_bytes(m[-4:], "little")
    starts[at] = pos
    v = lambda x: starts[x >> 16] + (x & 0xffff)
    assert bai[:4] == b"BAI\x01"
    n_ref, p, out = struct.unpack_from("<i", bai, 4)[0], 8, []
    for _ in range(n_ref):
        bins = []
        n_bin = struct.unpack_from("<i", bai, p)[0]
        p += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, p)
            chunks = [struct.unpack_from("<QQ", bai, p + 8 + 16 * k) for k in range(n_chunk)]
            p += 8 + 16 * n_chunk
            # the pseudo-bin: its first chunk is the reference's range in the file, its second two counts
            bins.append((b, [(v(c[0]), v(c[1])) if b != 37450 or k == 0 else c for k, c in enumerate(chunks)]))
        n_intv = struct.unpack_from("<i", bai, p)[0]
        out.append((bins, [v(x) for x in struct.unpack_from("<%dQ" % n_intv, bai, p + 4)]))
        p += 4 + 8 * n_intv
    return out, bai[p:]                                                          # the count of unplaced records, if any


def test_map_route_with_every_switch_on(workdir):
    """the route test's input with transcripts (sorted + indexed passes whose records are kept, a name-sorted pass) in a fresh process
    with the four switches in the environment and both piece knobs small, against the same call here with every switch off: the same
    files, the BAMs compressed differently around the same streams; the child's counters show that every route was taken"""
    import capi
    import map_route as M
    d = os.path.join(workdir, "bamseams_route")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    for where in ("host", "dev"):
        os.makedirs(os.path.join(d, where))
    capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "host", "o"), transcripts_fa=data["transcripts_fa"], threads=4)
    assert capi.ps_bam_records_info()["n_reads"] == 0 and capi.ps_bam_sort_info()["n_calls_device"] == 0 and capi.ps_bam_name_sort_info()["n_calls_device"] == 0
    e = dict(os.environ)
    for k in ("PS_BAM_SORT_MAX_MB", "PS_BGZF_BTYPE", "PS_VERBOSE"):
        e.pop(k, None)
    e.update(PS_BAM_RECORDS_GPU="1", PS_BAM_SORT_GPU="0", PS_BAM_NAME_SORT_GPU="0", PS_BGZF_GPU="0", PS_BAM_SORT_PIECE="4096", PS_BGZF_PIECE=str(Z.BLK))
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "para-suite_amd"), data["route_fastq"], data["genome_fa"], os.path.join(d, "dev", "o"),
                        data["transcripts_fa"]], env=e, timeout=100, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("INFO")][0][5:])
    assert info["records"]["n_device"] > 0 and info["records"]["n_reads"] > data["n_route_reads"], info
    for which in ("sort", "name"):
        assert info[which]["on_device"] == 1 and info[which]["n_calls_device"] >= 1 and info[which]["n_calls_host"] == 0 and info[which]["n_records"] > 0, info
    files = sorted(os.listdir(os.path.join(d, "host")))
    assert len([f for f in files if f.endswith(".bam")]) >= 3 and any(f.endswith(".bai") for f in files) and files == sorted(os.listdir(os.path.join(d, "dev")))
    for f in files:
        h, v = (open(os.path.join(d, w, f), "rb").read() for w in ("host", "dev"))
        if f.endswith(".bam"):
            assert h != v and gzip.decompress(h) == gzip.decompress(v), f
        elif f.endswith(".bai"):
            # an index names its records by their blocks' places in the file, which the other compressor moves: the two indexes must say
            # the same about the one inflated stream, offset for offset
            bams = [open(os.path.join(d, w, f[:-4]), "rb").read() for w in ("host", "dev")]
            assert _bai_over_the_stream(h, bams[0]) == _bai_over_the_stream(v, bams[1]), f
        else:
            assert h == v, f


def test_map_to_bam_with_every_switch_on(mid_input, monkeypatch):
    """the Python switches instead of the environment: records, sort and compressor on one device, the stream resident, every knob
    small -- the .bam and the .bai of the call that has the compressor's switch alone"""
    import capi
    monkeypatch.setenv("PS_CHUNK_MB", "1")
    m = mid_input
    alone, every = os.path.join(m["dir"], "every.alone.bam"), os.path.join(m["dir"], "every.on.bam")
    write = lambda p: capi.ps_map_to_bam(8, "-1", m["ep"], m["ip"], m["fa"], m["fq"], p, sort_by_coordinate=True, write_index=True)
    capi.ps_bgzf_device(0)
    st_alone = write(alone)
    assert capi.ps_bam_records_info()["n_reads"] == 0 and capi.ps_bam_sort_info()["n_calls_device"] == 0
    monkeypatch.setenv("PS_BAM_SORT_PIECE", "4096")
    monkeypatch.setenv("PS_BGZF_PIECE", str(Z.BLK))
    capi.ps_bam_records_device(1)
    capi.ps_bam_sort_device(0)
    capi.ps_bam_name_sort_device(0)
    st_every = write(every)
    records, sort, name = capi.ps_bam_records_info(), capi.ps_bam_sort_info(), capi.ps_bam_name_sort_info()
    assert st_every["n_in"] == 30000 and st_every["n_out"] > 20000
    assert records["n_device"] > 0 and records["n_reads"] == 30000 and records["n_device"] + records["n_host"] == records["n_records"] == st_every["n_out"]
    assert (sort["n_calls_device"], sort["n_calls_host"], sort["n_resident"], sort["n_records"]) == (1, 0, 1, st_every["n_out"])
    assert (name["on_device"], name["n_calls_device"], name["n_calls_host"]) == (1, 0, 0)       # a coordinate sort never asks the name switch
    assert st_alone == st_every
    _same_files(alone, every, "every")
    assert os.path.exists(every + ".bai") and len(_body_sizes(every)) >= 3
