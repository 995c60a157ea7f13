"""BGZF compression on the device (csrc/ps_bgzf.hip, csrc/ps_deflate.h).  Python's zlib is the oracle for what a member holds;
the host build of the same encoder (tests/deflate_check.cpp, the lanes run one after the other) is what the device's bytes are
compared with, byte for byte: the encoder's output is a pure function of its input, so a wrong block shows as a difference
and names itself."""
import gzip
import os
import shutil
import subprocess
import sys

import pytest

import bgzf_inputs as B

pytestmark = pytest.mark.gpu

INPUTS = B.edge_inputs()
# Size of the device's output over zlib level 1 on the same block cuts (what the library writes without the switch), on the
# BAM records of 2,000 mapped reads: measured 0.9828 (169,397 bytes against 172,361; test_mapped_records_and_the_size_guard
# prints it; the corpora of tools/bgzf_time.py are in DESIGN.md §4o), an excess of -1.7 %, rounded up to the next five
# percentage points: none.  An excess would have been allowed because the matcher keeps one candidate per hash where zlib level 1
# follows a chain of four; on these records the measurement shows none.
MAX_EXCESS_OVER_ZLIB1 = 1.00


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return B.build_check(tmp_path_factory.mktemp("deflate"), sanitize=False)


@pytest.fixture(scope="module")
def mapped(example, workdir):
    """2,000 reads of the golden genome through ps_map_to_bam, switch off: the BAM, and its records as the mapper built them"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "bgzf")
    os.makedirs(d)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], 2000, 50, seed=21, indel_scale=30))
    if not os.path.exists(example["fa"] + ".bwt"):
        capi.ps_index(example["fa"])
    capi.ps_bgzf_device(-1)
    bam = os.path.join(d, "host.bam")
    st = capi.ps_map_to_bam(4, "2", None, None, example["fa"], fq, bam)
    stream = gzip.decompress(open(bam, "rb").read())
    head = B.members(open(bam, "rb").read())[0]
    n_head = int.from_bytes(head[-4:], "little")
    return dict(dir=d, fq=fq, fa=example["fa"], bam=bam, st=st, stream=stream, records=stream[n_head:])


def _device(data, **env):
    import capi
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return capi.ps_bgzf_compress(data, 0)
    finally:
        for k in env:
            del os.environ[k]


def _check_input(exe, tmp_path, data, **env):
    raw, st = _device(data, **env)
    ms = B.check_members(raw, data)
    assert (st["n_blocks"], st["in_bytes"], st["out_bytes"]) == (len(ms), len(data), len(raw))
    assert [st["n_stored"], st["n_fixed"], st["n_dynamic"]] == [sum(B.btype(m) == t for m in ms) for t in (0, 1, 2)]
    host, _ = B.host_members(exe, data, tmp_path)
    for k, (m, h) in enumerate(zip(ms, B.members(host))):
        assert m == h, "block %d differs from the host build" % k
    assert raw == host
    # the chooser: by exact count the default is never larger than fixed-only or stored-only
    for mode in ("fixed", "stored"):
        raw_m, _ = _device(data, PS_BGZF_BTYPE=mode)
        B.check_members(raw_m, data)
        assert len(raw) <= len(raw_m), mode
    return raw, st


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_edge_inputs(exe, tmp_path, name):
    env = dict(PS_BGZF_PIECE=B.BLK) if name == "three_blocks_17" else {}          # one block per launch: four rounds
    raw, st = _check_input(exe, tmp_path, INPUTS[name], **env)
    if name == "random_block":
        assert st["n_stored"] == 1 and len(raw) == B.BLK + 5 + 26
    if name == "n0":
        assert raw == b"" and st["n_blocks"] == 0


def test_mapped_records_and_the_size_guard(exe, tmp_path, mapped):
    data = mapped["records"]
    assert len(data) > B.BLK                                                       # more than one block
    raw, st = _check_input(exe, tmp_path, data)
    ratio = len(raw) / B.zlib1_size(data)
    print("device / zlib level 1 on %d bytes of records: %.4f (%d / %d); blocks stored %d fixed %d dynamic %d"
          % (len(data), ratio, len(raw), B.zlib1_size(data), st["n_stored"], st["n_fixed"], st["n_dynamic"]))
    assert ratio <= MAX_EXCESS_OVER_ZLIB1


def test_capacity_is_checked():
    import ctypes as C
    import capi
    data = INPUTS["rep260"]
    raw, _ = capi.ps_bgzf_compress(data, 0)
    dst = C.create_string_buffer(b"\xee" * len(raw), len(raw))
    assert capi.lib().ps_bgzf_compress(data, len(data), 0, dst, len(raw) - 1, None) != 0
    assert b"destination holds" in capi.lib().ps_last_error() and dst.raw == b"\xee" * len(raw)
    assert capi.lib().ps_bgzf_compress(data, len(data), 0, dst, len(raw), None) == 0 and dst.raw == raw


def _sam(path, n):
    with open(path, "w") as f:
        f.write("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:100000\n@SQ\tSN:chrB\tLN:50000\n")
        for i in range(n):
            seq = "ACGTTGCAAG"[i % 7:] + "ACGTTGCAAGGTCA"[:5 + i % 9]
            f.write("q%d\t%d\t%s\t%d\t%d\t%dM\t*\t0\t0\t%s\t%s\tNM:i:%d\n"
                    % (i, 16 * (i & 1), "chrA" if i % 3 else "chrB", 1 + (i * 7919) % 49000, i % 61, len(seq), seq, "I" * len(seq), i % 3))


def test_sam_to_bam_index_and_view(tmp_path):
    """sorted and indexed, with the switch and without: the same byte stream and record count; the .bai beside the
    device-compressed file is what ps_bam_index derives from that file; ps_bam_view reads it back record for record"""
    import capi
    sam = str(tmp_path / "a.sam")
    _sam(sam, 6000)
    host, dev = str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    capi.ps_bgzf_device(-1)
    st_h = capi.ps_sam_to_bam(sam, host, sort_by_coordinate=True, write_index=True, threads=4)
    capi.ps_bgzf_device(0)
    try:
        st_d = capi.ps_sam_to_bam(sam, dev, sort_by_coordinate=True, write_index=True, threads=4)
        view = str(tmp_path / "view.bam")
        st_v = capi.ps_bam_view(dev, view, min_mapq=0, threads=4)
    finally:
        capi.ps_bgzf_device(-1)
    raw_h, raw_d = open(host, "rb").read(), open(dev, "rb").read()
    assert raw_h != raw_d and gzip.decompress(raw_h) == gzip.decompress(raw_d)
    assert st_h["n_out"] == st_d["n_out"] == 6000 and st_d["bam_bytes"] == len(raw_d)
    ms = B.members(raw_d)
    assert len(ms) >= 4 and ms[-1] == raw_h[-28:] and len(ms) == len(B.members(raw_h))
    copy = str(tmp_path / "copy.bam")
    shutil.copyfile(dev, copy)
    capi.ps_bam_index(copy, threads=4)
    assert open(copy + ".bai", "rb").read() == open(dev + ".bai", "rb").read()
    assert st_v["n_in"] == st_v["n_out"] == 6000 and gzip.decompress(open(view, "rb").read()) == gzip.decompress(raw_d)


def test_map_to_bam_with_the_switch(mapped):
    import capi
    dev = os.path.join(mapped["dir"], "dev.bam")
    capi.ps_bgzf_device(0)
    try:
        st = capi.ps_map_to_bam(4, "2", None, None, mapped["fa"], mapped["fq"], dev)
    finally:
        capi.ps_bgzf_device(-1)
    assert {k: st[k] for k in ("n_in", "n_out")} == {k: mapped["st"][k] for k in ("n_in", "n_out")} and st["n_out"] == 2000
    raw = open(dev, "rb").read()
    assert raw != open(mapped["bam"], "rb").read() and gzip.decompress(raw) == mapped["stream"] and st["bam_bytes"] == len(raw)


_CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import capi
kind, args = sys.argv[2], sys.argv[3:]
if kind == "route":
    capi.ps_map_route(args[0], args[1], args[2], transcripts_fa=args[3], threads=4)
else:
    capi.ps_sam_to_bam(args[0], args[1], threads=4)
"""


def _child(env, *args):
    e = dict(os.environ)
    e.pop("PS_BGZF_GPU", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(B.ROOT, "para-suite_amd")] + list(args), env=e, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_map_route_under_the_environment_switch(workdir):
    """the route test's smallest input: every BAM of a ps_map_route call made with PS_BGZF_GPU=0 in the environment holds the
    bytes of the same call with host compression, and is not the same file"""
    import capi
    import map_route as M
    d = os.path.join(workdir, "bgzf_route")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    for where in ("host", "dev"):
        os.makedirs(os.path.join(d, where))
    capi.ps_bgzf_device(-1)
    capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "host", "o"), transcripts_fa=data["transcripts_fa"], threads=4)
    _child(dict(PS_BGZF_GPU="0"), "route", data["route_fastq"], data["genome_fa"], os.path.join(d, "dev", "o"), data["transcripts_fa"])
    bams = sorted(f for f in os.listdir(os.path.join(d, "host")) if f.endswith(".bam"))
    assert len(bams) >= 3 and sorted(os.listdir(os.path.join(d, "host"))) == sorted(os.listdir(os.path.join(d, "dev")))
    for f in bams:
        a, b = open(os.path.join(d, "host", f), "rb").read(), open(os.path.join(d, "dev", f), "rb").read()
        assert a != b and gzip.decompress(a) == gzip.decompress(b), f


def test_the_switch_goes_back_and_refuses_a_missing_device(tmp_path):
    """-1 restores zlib's output byte for byte, compared with a process that never set the switch"""
    import capi
    sam = str(tmp_path / "a.sam")
    _sam(sam, 3000)
    never, dev, back = (str(tmp_path / x) for x in ("never.bam", "dev.bam", "back.bam"))
    _child({}, "sam", sam, never)
    capi.ps_bgzf_device(0)
    try:
        capi.ps_sam_to_bam(sam, dev, threads=4)
    finally:
        capi.ps_bgzf_device(-1)
    capi.ps_sam_to_bam(sam, back, threads=4)
    assert open(back, "rb").read() == open(never, "rb").read() != open(dev, "rb").read()
    with pytest.raises(capi.PsError, match="no HIP device 1000"):
        capi.ps_bgzf_device(1000)
    capi.ps_sam_to_bam(sam, back, threads=4)                                      # the failed call changed nothing
    assert open(back, "rb").read() == open(never, "rb").read()
