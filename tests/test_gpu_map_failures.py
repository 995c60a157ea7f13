"""The streaming map pass on its error paths and in its fused-profile mode, small: host-side file errors in each of the three
stages' reach (options before any thread starts, the parser, the writer with several pieces in flight), each followed by a good call
in the same process that must give what the same call gave before any failure -- no stage left waiting, contexts and the
deferred-free threads sound -- and ps_map_profiled cut into pieces and on two workers against the single-piece call.
No test here provokes a device fault: every failure is a file that is not there.

20,000 reads of 50 bp are 2.8 MiB of FASTQ: PS_CHUNK_MB=1 cuts them into three pieces, the smallest input on which the ordered
hand-over and the bounded map of finished pieces are in play."""
import os

import pytest

pytestmark = pytest.mark.gpu

CALLS = ("map", "to_bam", "profiled")
# what ps_last_error() says, up to the path it names: the texts of the library as it was before the pass moved out of ps_capi.hip
# (load_reads_chunked, batch_write_sam and the BGZF writer, read_profile_files), which this change must leave as they are
EXPECTED = {
    "no_reads": "cannot open reads ",
    "no_out_dir": "cannot write ",
    "no_profile": "cannot open error profile ",
}


def _bam_records(path):
    from test_gpu_map_to_bam import _recs
    return _recs(path)


@pytest.fixture(scope="module")
def job(example, workdir):
    """inputs, and the output of every call made once before any failure"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "fail")
    os.makedirs(d)
    fa = example["fa"]
    if not os.path.exists(fa + ".bwt"):
        capi.ps_index(fa)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], n_reads=20000, read_len=50, seed=5, indel_scale=30, n_frac=0.002))
    assert 2 << 20 < os.path.getsize(fq) < 3 << 20
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    ep, ip = os.path.join(d, "in.errorprofile"), os.path.join(d, "in.indelprofile")
    with open(ep, "w") as f:
        for row in P:
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    open(ip, "w").write("2.1E-5\t5.9E-4")
    j = dict(d=d, fa=fa, fq=fq, ep=ep, ip=ip)
    assert "PS_CHUNK_MB" not in os.environ and "PARASUITE_GPU_IDS" not in os.environ
    good = {c: _call(c, j, os.path.join(d, "ref_" + c)) for c in CALLS}
    assert good["map"] == good["profiled"][0] and 0 < len(good["to_bam"][2]) < 20000
    j["good"] = good
    return j


def _call(which, j, out, fq=None, ep=None):
    """one call with 8 threads and profile costs; returns what the call wrote, in a form that compares: SAM bytes, BAM records"""
    import capi
    fq, ep = fq or j["fq"], ep or j["ep"]
    if which == "map":
        capi.ps_map(8, "-1", ep, j["ip"], j["fa"], fq, out + ".sam")
        return open(out + ".sam", "rb").read()
    if which == "to_bam":
        capi.ps_map_to_bam(8, "-1", ep, j["ip"], j["fa"], fq, out + ".bam", min_mapq=10)
        return _bam_records(out + ".bam")
    capi.ps_map_profiled(8, "-1", ep, j["ip"], j["fa"], fq, out + ".sam", 10, 101, out)
    return tuple(open(out + x, "rb").read() for x in (".sam", ".errorprofile", ".indelprofile"))


@pytest.mark.parametrize("failure", sorted(EXPECTED))
@pytest.mark.parametrize("which", CALLS)
def test_failure_names_the_path_and_the_next_call_is_sound(job, which, failure, monkeypatch):
    import capi
    d = job["d"]
    tag = "%s_%s" % (which, failure)
    kw, path = {}, None
    if failure == "no_reads":
        path = kw["fq"] = os.path.join(d, "no_such.fq")
    elif failure == "no_profile":
        path = kw["ep"] = os.path.join(d, "no_such.errorprofile")
    out = os.path.join(d, tag)
    if failure == "no_out_dir":                                # the writer fails on its first piece while two more are on their way
        monkeypatch.setenv("PS_CHUNK_MB", "1")
        out = os.path.join(d, "no_such_dir", tag)
        path = out + (".bam" if which == "to_bam" else ".sam")
    with pytest.raises(capi.PsError) as ei:
        _call(which, job, out, **kw)
    print(tag, "->", str(ei.value))
    assert EXPECTED[failure] + path in str(ei.value)
    monkeypatch.delenv("PS_CHUNK_MB", raising=False)
    assert _call(which, job, os.path.join(d, tag + "_after")) == job["good"][which]


@pytest.mark.parametrize("env", [dict(PS_CHUNK_MB="1"), dict(PS_CHUNK_MB="1", PARASUITE_GPU_IDS="0,0")], ids=["pieces", "two_workers"])
def test_profiled_in_pieces_equals_the_single_piece_call(job, env, monkeypatch, capfd):
    import re
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PS_VERBOSE", "1")
    capfd.readouterr()
    got = _call("profiled", job, os.path.join(job["d"], "prof_" + "_".join(sorted(env))))
    err = capfd.readouterr().err
    pieces = re.findall(r"piece (\d+) on device 0 worker (\d+)", err)
    print(sorted(env), "->", pieces)
    assert len(pieces) == 3, err
    if "PARASUITE_GPU_IDS" in env:
        assert "1 device(s) x 2 worker(s)" in err
    sam, eprof, iprof = job["good"]["profiled"]
    assert got[1] == eprof and got[2] == iprof
    assert got[0] == sam == job["good"]["map"]
