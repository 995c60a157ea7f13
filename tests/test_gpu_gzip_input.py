"""gzip and BGZF compressed inputs on the GPU paths (csrc/ps_inflate.h): the reads of ps_map, ps_map_to_bam, ps_map_profiled and
ps_batch_from_fastq, the FASTA of ps_index and ps_pileup_clusters, all three inputs of ps_map_route -- every output equal to the
one from the plain file -- and a reads file cut in the middle of its data while pieces are in flight: the call fails naming the
file and the next call in the same process is sound.  No test here provokes a device fault: the failure is a damaged file.

The shape is that of tests/test_gpu_map_failures.py: 20,000 reads of 50 bp are 2.8 MiB of FASTQ, three pieces with PS_CHUNK_MB=1,
the smallest input on which the ordered hand-over is in play."""
import os
import shutil

import pytest

import gz_forms as G

pytestmark = pytest.mark.gpu

MAKE = {"gz": G.gz, "bgzf": G.bgzf}


def _call(*a, **kw):
    from test_gpu_map_failures import _call as call
    return call(*a, **kw)


@pytest.fixture(scope="module")
def job(example, workdir):
    """the inputs plain and compressed, and the output of every call on the plain reads"""
    import capi
    import simulate as S
    from test_gpu_map_failures import CALLS
    d = os.path.join(workdir, "gzin")
    os.makedirs(d)
    fa = example["fa"]
    if not os.path.exists(fa + ".bwt"):
        capi.ps_index(fa)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], n_reads=20000, read_len=50, seed=5, indel_scale=30, n_frac=0.002))
    text = open(fq, "rb").read()
    assert 2 << 20 < len(text) < 3 << 20
    j = dict(d=d, fa=fa, fq=fq)
    for form, make in MAKE.items():
        j[form] = os.path.join(d, "r.fq." + form)
        open(j[form], "wb").write(make(text))
    j["cut"] = os.path.join(d, "cut.fq.gz")
    open(j["cut"], "wb").write(G.gz(text)[:len(G.gz(text)) // 2])
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    j["ep"], j["ip"] = os.path.join(d, "in.errorprofile"), os.path.join(d, "in.indelprofile")
    with open(j["ep"], "w") as f:
        for row in P:
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    open(j["ip"], "w").write("2.1E-5\t5.9E-4")
    assert "PS_CHUNK_MB" not in os.environ and "PS_UNIT_MB" not in os.environ
    j["good"] = {c: _call(c, j, os.path.join(d, "ref_" + c)) for c in CALLS}
    assert 0 < len(j["good"]["to_bam"][2]) < 20000
    return j


@pytest.mark.parametrize("form", sorted(MAKE))
@pytest.mark.parametrize("which", ["map", "to_bam", "profiled"])
def test_compressed_reads_give_the_plain_output(job, which, form, monkeypatch, capfd):
    import re
    assert _call(which, job, os.path.join(job["d"], "%s_%s_one" % (which, form)), fq=job[form]) == job["good"][which]
    monkeypatch.setenv("PS_CHUNK_MB", "1")
    monkeypatch.setenv("PS_UNIT_MB", "1")
    monkeypatch.setenv("PS_VERBOSE", "1")
    capfd.readouterr()
    got = _call(which, job, os.path.join(job["d"], "%s_%s_pieces" % (which, form)), fq=job[form])
    pieces = re.findall(r"piece (\d+) on device 0 worker (\d+)", capfd.readouterr().err)
    assert len(pieces) == 3, pieces
    assert got == job["good"][which]


def test_batch_from_compressed_fastq(job):
    import capi
    ctx = capi.Ctx.open(job["fa"])
    try:
        ctx.set_profile_files(job["ep"], job["ip"], "-1")
        out = []
        for path in (job["fq"], job["gz"], job["bgzf"]):
            b = ctx.batch_from_fastq(path)
            b.run(4)
            out.append((b.n_aln().copy(), b.hits().copy()))
            b.free()
        assert out[0][0].size == 20000 and out[0][0].sum() > 10000
        for n_aln, hits in out[1:]:
            assert (n_aln == out[0][0]).all() and hits.tobytes() == out[0][1].tobytes()
    finally:
        ctx.close()


def test_compressed_reference(job):
    """the index of genome.fa.gz is named after the path as given and holds the same bytes; the same string then serves ps_map and
    ps_pileup_clusters"""
    import capi
    from conftest import sam_records
    from test_gpu_pileup_clusters import _paths, _read
    d = job["d"]
    fz = os.path.join(d, "genome.fa.gz")
    fb = os.path.join(d, "genome_b.fa.gz")
    text = open(job["fa"], "rb").read()
    open(fz, "wb").write(G.gz(text))
    open(fb, "wb").write(G.bgzf(text))
    for f in (fz, fb):
        capi.ps_index(f)
        for ext in (".bwt", ".sa", ".pac", ".ann"):
            assert open(f + ext, "rb").read() == open(job["fa"] + ext, "rb").read(), (f, ext)
    sam = os.path.join(d, "on_gz_index.sam")
    capi.ps_map(8, "-1", job["ep"], job["ip"], fz, job["gz"], sam)
    plain = os.path.join(d, "ref_map.sam")
    assert sam_records(sam) == sam_records(plain) and len(sam_records(sam)) == 20000
    bam = os.path.join(d, "sorted.bam")
    capi.ps_map_to_bam(8, "-1", job["ep"], job["ip"], job["fa"], job["fq"], bam, min_mapq=10, sort_by_coordinate=True, write_index=True)
    st = capi.ps_pileup_clusters(bam, job["fa"], os.path.join(d, "cl_plain"), None, 1, os.path.join(d, "cl_plain"))
    want = _read(_paths(os.path.join(d, "cl_plain"), os.path.join(d, "cl_plain")))
    assert st["n_clusters"] > 0 and len(want) == 6 and len(want[".ccr.fasta"]) > 0
    for name, f in (("cl_gz", fz), ("cl_bgzf", fb)):
        assert capi.ps_pileup_clusters(bam, f, os.path.join(d, name), None, 1, os.path.join(d, name)) == st
        assert _read(_paths(os.path.join(d, name), os.path.join(d, name))) == want, name


@pytest.fixture(scope="module")
def route(workdir):
    """the data of tests/map_route.py plain and gzip, all four indexes, and the all-plain call"""
    import capi
    import map_route as M
    d = os.path.join(workdir, "gz_route")
    os.makedirs(d)
    data = M.make_data(d)
    for k in ("genome_fa", "transcripts_fa", "route_fastq"):
        open(data[k] + ".gz", "wb").write(G.gz(open(data[k], "rb").read()))
    for f in (data["genome_fa"], data["transcripts_fa"], data["genome_fa"] + ".gz", data["transcripts_fa"] + ".gz"):
        capi.ps_index(f)
    os.makedirs(os.path.join(d, "plain"))
    st = capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "plain", "o"), transcripts_fa=data["transcripts_fa"],
                           threads=4, refine=True)
    assert st["n_fastq_parses"] == 1 and st["combine"]["n_lifted"] > 0
    return dict(d=d, data=data, plain=os.path.join(d, "plain"))


@pytest.mark.parametrize("keep_mb,parses", [(None, 1), ("1", 2)], ids=["kept", "parsed_again"])
def test_route_with_every_input_compressed(route, keep_mb, parses, monkeypatch):
    """refine with transcripts: reads, genome and transcripts gzip against the all-plain call"""
    import capi
    import map_route as M
    from test_gpu_map_route import _same_files
    data = route["data"]
    assert os.path.getsize(data["route_fastq"]) > 1 << 20                  # a 1 MB bound is below the input
    if keep_mb:
        monkeypatch.setenv("PS_ROUTE_KEEP_MB", keep_mb)
    where = os.path.join(route["d"], "gz_" + (keep_mb or "all"))
    os.makedirs(where)
    st = capi.ps_map_route(data["route_fastq"] + ".gz", data["genome_fa"] + ".gz", os.path.join(where, "o"),
                           transcripts_fa=data["transcripts_fa"] + ".gz", threads=4, refine=True)
    refine, transcripts, given = M.CASES["refine_transcripts"]
    assert sorted(os.path.join(where, f) for f in os.listdir(where)) == M.output_names(os.path.join(where, "o"), refine, transcripts, given)
    _same_files(where, route["plain"])
    assert st["n_fastq_parses"] == parses and st["n_index_loads_genome"] == 1 and st["n_index_loads_transcripts"] == 1
    assert st["n_reads"] == data["n_route_reads"]
    shutil.rmtree(where)


@pytest.mark.parametrize("which", ["map", "to_bam"])
def test_cut_reads_file_fails_and_the_next_call_is_sound(job, which, monkeypatch):
    """a file error, not a device fault: the inflater meets the end of the input in the middle of the deflate data after the
    first pieces have gone to the device"""
    import capi
    monkeypatch.setenv("PS_CHUNK_MB", "1")
    with pytest.raises(capi.PsError) as ei:
        _call(which, job, os.path.join(job["d"], which + "_cut"), fq=job["cut"])
    print(which, "->", str(ei.value))
    assert job["cut"] in str(ei.value) and "ends inside" in str(ei.value)
    assert job["cut"] in capi.lib().ps_last_error().decode()
    monkeypatch.delenv("PS_CHUNK_MB")
    assert _call(which, job, os.path.join(job["d"], which + "_after_cut"), fq=job["gz"]) == job["good"][which]
