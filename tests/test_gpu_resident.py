"""The resident scope on the GPU (include/parasuite_hip.h: ps_resident_begin / _end / _info): inside a scope every mapping call
writes what it writes outside one, byte for byte, while the scope's counters show that the index was loaded once, found again,
reloaded when its files changed, evicted at the bound and dropped after a failed call.

Data: the `example` genome (483 kb) with 2,000 simulated reads of 50 bp, and the genome, transcripts and reads of
tests/map_route.py for the second reference and the route.  What the calls write outside any scope is computed once per module and
shared.  No test provokes a device fault: the failing call fails in the host parser."""
import os
import shutil

import pytest

import map_route as M

pytestmark = pytest.mark.gpu

INDEX_EXT = (".ann", ".bwt", ".sa", ".pac")
T = 4                                                          # host threads of every call


def _bam(path):
    from test_gpu_map_to_bam import _recs
    return _recs(path)


def _read(path):
    return open(path, "rb").read()


def _write_profile(d):
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    ep, ip = os.path.join(d, "in.errorprofile"), os.path.join(d, "in.indelprofile")
    with open(ep, "w") as f:
        for row in P:
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    open(ip, "w").write("2.1E-5\t5.9E-4")
    return ep, ip


def four_calls(j, out):
    """ps_map stock, ps_map with a profile, ps_map_to_bam, ps_map_profiled against the one genome -> what they wrote, comparable"""
    import capi
    os.makedirs(out)
    p = lambda name: os.path.join(out, name)
    capi.ps_map(T, "2", None, None, j["fa"], j["fq"], p("stock.sam"))
    capi.ps_map(T, "-1", j["ep"], j["ip"], j["fa"], j["fq"], p("profile.sam"))
    capi.ps_map_to_bam(T, "2", None, None, j["fa"], j["fq"], p("stock.bam"), min_mapq=10)
    capi.ps_map_profiled(T, "2", None, None, j["fa"], j["fq"], p("profiled.sam"), 10, 101, p("profiled"))
    return dict(stock=_read(p("stock.sam")), profile=_read(p("profile.sam")), bam=_bam(p("stock.bam")),
                profiled=tuple(_read(p("profiled" + x)) for x in (".sam", ".errorprofile", ".indelprofile")))


def alternate(j, out):
    """genome, transcripts, genome, transcripts -> the four SAM files"""
    import capi
    os.makedirs(out)
    got = []
    for i, (fa, fq) in enumerate([(j["fa"], j["fq"]), (j["t_fa"], j["t_fq"])] * 2):
        sam = os.path.join(out, "%d.sam" % i)
        capi.ps_map(T, "2", None, None, fa, fq, sam)
        got.append(_read(sam))
    return got


def map_sam(j, out, fa=None, fq=None):
    import capi
    capi.ps_map(T, "2", None, None, fa or j["fa"], fq or j["fq"], out)
    return _read(out)


@pytest.fixture(scope="module")
def job(example, workdir):
    """the inputs with their indexes built, and what the calls write outside any scope"""
    import capi
    import simulate as S
    assert capi.ps_resident_info()["active"] == 0
    assert "PS_JUMP_LEVELS" not in os.environ and "PARASUITE_GPU_IDS" not in os.environ      # what test_key_parts sets
    d = os.path.join(workdir, "resident")
    os.makedirs(d)
    fa = os.path.join(d, "genome.fa")
    S.write_fasta(fa, example["genome"])
    capi.ps_index(fa)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, S.simulate_reads(example["genome"], n_reads=2000, read_len=50, seed=77, indel_scale=30, n_frac=0.002))
    ep, ip = _write_profile(d)
    os.makedirs(os.path.join(d, "route"))
    data = M.make_data(os.path.join(d, "route"))
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    j = dict(d=d, fa=fa, fq=fq, ep=ep, ip=ip, data=data, t_fa=data["transcripts_fa"], t_fq=data["fastq"])
    j["four"] = four_calls(j, os.path.join(d, "four.outside"))
    j["alt"] = alternate(j, os.path.join(d, "alt.outside"))
    assert j["alt"][0] == j["alt"][2] == j["four"]["stock"] and j["alt"][1] == j["alt"][3] != j["alt"][0]
    assert j["four"]["stock"] != j["four"]["profile"] and sum(1 for l in j["four"]["stock"].split(b"\n") if l and l[:1] != b"@") == 2000
    assert not any(capi.ps_resident_info()[k] for k in ("active", "n_calls", "n_index_loads"))        # calls outside a scope count nothing
    yield j
    if capi.ps_resident_info()["active"]:                      # a test that failed inside its scope: the tests of other modules start outside one
        capi.ps_resident_end()


def counters(**want):
    import capi
    i = capi.ps_resident_info()
    base = dict(n_index_loads=0, n_index_reuses=0, n_stale_reloads=0, n_evictions=0, n_dropped_after_error=0)
    base.update(want)
    assert {k: i[k] for k in base} == base, i
    return i


# ---- 1 --------------------------------------------------------------------------------------------------------------------------
def test_same_output_one_load(job):
    import capi
    with capi.resident():
        got = four_calls(job, os.path.join(job["d"], "four.inside"))
        i = counters(n_calls=4, n_index_loads=1, n_index_reuses=3, n_references=1, active=1)
        assert i["bytes_index_resident"] > 0
    for k in ("stock", "profile", "profiled"):
        assert got[k] == job["four"][k], k                     # SAM and profile files byte for byte
    assert got["bam"] == job["four"]["bam"]                    # header text, references, every record
    assert len(got["bam"][2]) > 1000


# ---- 2 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_references,want", [(2, dict(n_index_loads=2, n_index_reuses=2, n_evictions=0, n_references=2)),
                                                 (1, dict(n_index_loads=4, n_index_reuses=0, n_evictions=3, n_references=1))], ids=["two", "one"])
def test_two_references_alternating(job, max_references, want):
    import capi
    with capi.resident(max_references=max_references):
        got = alternate(job, os.path.join(job["d"], "alt.inside%d" % max_references))
        counters(n_calls=4, **want)
    assert got == job["alt"]


# ---- 3 --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_genomes(job):
    """a second genome of the example's shape, and what the reads give against it outside any scope"""
    import capi
    import simulate as S
    d = os.path.join(job["d"], "stale")
    os.makedirs(d)
    other = os.path.join(d, "other.fa")
    S.write_fasta(other, S.example_genome(seed=0x5EED0A11))
    capi.ps_index(other)
    sam = map_sam(job, os.path.join(d, "other.outside.sam"), fa=other)
    assert sam != job["four"]["stock"]
    return dict(d=d, other=other, other_sam=sam)


def test_stale_index_rebuilt_by_ps_index(job, two_genomes):
    """ps_index of another genome at the same path inside the scope: it drops the path's entry itself, the next call loads the new
    index -- an invalidation, not a stale find"""
    import capi
    d = two_genomes["d"]
    path = os.path.join(d, "rebuilt.fa")
    shutil.copyfile(job["fa"], path)
    capi.ps_index(path)
    with capi.resident():
        assert map_sam(job, os.path.join(d, "rebuilt.a.sam"), fa=path) == job["four"]["stock"]
        counters(n_index_loads=1, n_references=1)
        shutil.copyfile(two_genomes["other"], path)
        capi.ps_index(path)
        assert capi.ps_resident_info()["n_references"] == 0
        got = map_sam(job, os.path.join(d, "rebuilt.b.sam"), fa=path)
        counters(n_index_loads=2, n_stale_reloads=0, n_references=1)
    assert got == two_genomes["other_sam"] == map_sam(job, os.path.join(d, "rebuilt.outside.sam"), fa=path)


def test_stale_index_files_replaced_behind_the_library(job, two_genomes):
    """another index's files moved over the path's with os.replace: the next call finds the entry's files changed"""
    import capi
    d = two_genomes["d"]
    path, donor = os.path.join(d, "moved.fa"), os.path.join(d, "donor.fa")
    for src, dst in ((job["fa"], path), (two_genomes["other"], donor)):
        shutil.copyfile(src, dst)
        for x in INDEX_EXT:
            shutil.copyfile(src + x, dst + x)
    with capi.resident():
        assert map_sam(job, os.path.join(d, "moved.a.sam"), fa=path) == job["four"]["stock"]
        assert map_sam(job, os.path.join(d, "moved.a2.sam"), fa=path) == job["four"]["stock"]
        counters(n_index_loads=1, n_index_reuses=1, n_references=1)
        for x in ("",) + INDEX_EXT:
            os.replace(donor + x, path + x)
        got = map_sam(job, os.path.join(d, "moved.b.sam"), fa=path)
        counters(n_index_loads=2, n_index_reuses=1, n_stale_reloads=1, n_references=1)
    assert got == two_genomes["other_sam"] == map_sam(job, os.path.join(d, "moved.outside.sam"), fa=path)


# ---- 4 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [dict(PS_JUMP_LEVELS="3"), dict(PARASUITE_GPU_IDS="0,0")], ids=["jump_levels", "two_workers"])
def test_key_parts(job, monkeypatch, env):
    import capi
    with capi.resident():
        assert map_sam(job, os.path.join(job["d"], "key.a.sam")) == job["four"]["stock"]
        counters(n_index_loads=1, n_references=1)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert map_sam(job, os.path.join(job["d"], "key.b.sam")) == job["four"]["stock"]
        counters(n_index_loads=2, n_references=2)              # another key: a second entry, loaded from the files
        assert map_sam(job, os.path.join(job["d"], "key.c.sam")) == job["four"]["stock"]
        counters(n_index_loads=2, n_index_reuses=1, n_references=2)
        for k in env:
            monkeypatch.delenv(k)
        assert map_sam(job, os.path.join(job["d"], "key.d.sam")) == job["four"]["stock"]
        counters(n_index_loads=2, n_index_reuses=2, n_references=2)   # and the first entry is still there


# ---- 5 --------------------------------------------------------------------------------------------------------------------------
def test_a_failing_call_drops_its_entry(job):
    """the reads file cut off after the '+' line of its last record: the host parser refuses it"""
    import capi
    lines = _read(job["fq"]).rstrip(b"\n").split(b"\n")
    assert len(lines) == 4 * 2000 and lines[-4][:1] == b"@" and lines[-2][:1] == b"+"
    cut = os.path.join(job["d"], "cut.fq")
    open(cut, "wb").write(b"\n".join(lines[:-1]) + b"\n")
    with capi.resident():
        assert map_sam(job, os.path.join(job["d"], "fail.a.sam")) == job["four"]["stock"]
        counters(n_index_loads=1, n_references=1)
        with pytest.raises(capi.PsError, match=r"cut\.fq: the last FASTQ record \(\S+\) is cut off after its '\+' line"):
            map_sam(job, os.path.join(job["d"], "fail.b.sam"), fq=cut)
        i = counters(n_index_loads=1, n_index_reuses=1, n_dropped_after_error=1, n_references=0)
        assert i["bytes_index_resident"] == 0 and i["active"] == 1
        assert map_sam(job, os.path.join(job["d"], "fail.c.sam")) == job["four"]["stock"]
        counters(n_index_loads=2, n_index_reuses=1, n_dropped_after_error=1, n_references=1, n_calls=3)
    with pytest.raises(capi.PsError, match="cut off after its"):           # outside a scope the same input fails the same way
        map_sam(job, os.path.join(job["d"], "fail.d.sam"), fq=cut)
    assert capi.ps_resident_info()["n_calls"] == 3


# ---- 6 --------------------------------------------------------------------------------------------------------------------------
def test_the_route_by_steps_and_the_route_twice(job):
    import capi
    from test_gpu_map_route import _same_files
    data, d = job["data"], os.path.join(job["d"], "route")
    refine, transcripts, given = M.CASES["refine_transcripts"]

    def call(where):
        os.makedirs(where)
        return capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(where, "o"), transcripts_fa=data["transcripts_fa"],
                                 threads=T, refine=refine)

    outside = os.path.join(d, "call.outside")
    st0 = call(outside)
    assert (st0["n_index_loads_genome"], st0["n_index_loads_transcripts"]) == (1, 1)
    assert sorted(os.path.join(outside, f) for f in os.listdir(outside)) == M.output_names(os.path.join(outside, "o"), refine, transcripts, given)
    steps = os.path.join(d, "steps.inside")
    os.makedirs(steps)
    with capi.resident():
        exp = M.route_by_steps(M.LibMapper(T), data, os.path.join(steps, "o"), refine=refine, transcripts=transcripts)
        counters(n_calls=3, n_index_loads=2, n_index_reuses=1, n_references=2)      # first pass, refine pass, transcript pass: 1 genome load, 1 transcript load
    _same_files(steps, outside)
    assert exp["n_reads"] == st0["n_reads"] == data["n_route_reads"]
    c = M.route_counts(data, os.path.join(steps, "o"), refine, exp["extract"]["n_weak"])
    M.assert_route_conditions(c, refine)
    with capi.resident():
        a, b = os.path.join(d, "call.a"), os.path.join(d, "call.b")
        st_a, st_b = call(a), call(b)
        assert (st_a["n_index_loads_genome"], st_a["n_index_loads_transcripts"]) == (1, 1)
        assert (st_b["n_index_loads_genome"], st_b["n_index_loads_transcripts"]) == (0, 0)
        counters(n_calls=2, n_index_loads=2, n_index_reuses=2, n_references=2)
    _same_files(a, outside)
    _same_files(b, outside)
    for k in ("n_reads", "first", "refine", "transcript", "extract", "combine", "n_fastq_parses"):
        assert st_a[k] == st_b[k] == st0[k], k


# ---- 7 --------------------------------------------------------------------------------------------------------------------------
def test_after_end(job):
    import capi
    ctx = capi.Ctx.open(job["fa"])
    blob_bytes = sum(ctx.blob(w)[1] for w in range(3))
    ctx.close()
    assert blob_bytes > 483000 // 4
    with capi.resident():
        assert map_sam(job, os.path.join(job["d"], "end.a.sam")) == job["four"]["stock"]
        i = counters(n_calls=1, n_index_loads=1, n_references=1, active=1)
        assert i["bytes_index_resident"] == blob_bytes * 1            # one device holds the index
    i = counters(n_calls=1, n_index_loads=1, active=0, n_references=0, bytes_index_resident=0)    # the counters of the last scope
    assert map_sam(job, os.path.join(job["d"], "end.b.sam")) == job["four"]["stock"]
    assert capi.ps_resident_info() == i                               # a plain ps_map works and counts nothing
