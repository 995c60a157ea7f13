"""ps_map_route on the GPU: the five cases of the `map` mode (Main.java:249-420) file for file against the call-by-call route
through the library's own calls (tests/map_route.py); the refine + transcripts case against where the generator cut the reads;
the same output whatever the cut, the number of workers or the host memory the call may keep; the trap reads' names; a
failure after two passes; and what is resident during and after the call."""
import gzip
import os
import shutil

import pytest

import map_route as M

pytestmark = pytest.mark.gpu

STAT_KEYS = ("n_genome", "n_transcript", "n_unplaced", "n_unlocated", "n_missed_indel_splice", "n_groups", "n_groups_ambiguous",
             "n_no_contig", "n_mt_unplaced", "n_lifted", "n_spliced", "n_strand_flipped")


@pytest.fixture(scope="module")
def route(workdir):
    """the data with both indexes built, and every case run once each way: route(name) -> dict(call=dir, steps=dir, st=, exp=)"""
    import capi
    d = os.path.join(workdir, "map_route")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    runs = {}

    def given_profile():
        """the profile files of the refine case, copied: the input of the case that is handed a profile"""
        r = run("refine")
        out = [os.path.join(d, "given" + x) for x in (".errorprofile", ".indelprofile")]
        for x, o in zip((".errorprofile", ".indelprofile"), out):
            if not os.path.exists(o):
                shutil.copyfile(os.path.join(r["steps"], "o.BWA-genomic.bam" + x), o)
        return out

    def call(name, where, **kw):
        refine, transcripts, given = M.CASES[name]
        ep, ip = given_profile() if given else (None, None)
        os.makedirs(where)
        return capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(where, "o"),
                                 transcripts_fa=data["transcripts_fa"] if transcripts else None, threads=4, refine=refine,
                                 error_profile=ep, indel_profile=ip, **kw)

    def run(name):
        if name not in runs:
            refine, transcripts, given = M.CASES[name]
            ep, ip = given_profile() if given else (None, None)
            r = dict(call=os.path.join(d, name + ".call"), steps=os.path.join(d, name + ".steps"))
            os.makedirs(r["steps"])
            r["exp"] = M.route_by_steps(M.LibMapper(4), data, os.path.join(r["steps"], "o"), refine=refine, transcripts=transcripts,
                                        error_profile=ep, indel_profile=ip)
            r["st"] = call(name, r["call"])
            runs[name] = r
        return runs[name]

    run.data, run.call, run.dir = data, call, d
    return run


def _stream(path):
    return gzip.decompress(open(path, "rb").read())


def _same_files(a, b):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in sorted(os.listdir(a)):
        if f.endswith(".bam"):
            assert _stream(os.path.join(a, f)) == _stream(os.path.join(b, f)), f
        elif not f.endswith(".bai"):
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_case_equals_the_call_by_call_route(route, name):
    import java_combine as J  # noqa: F401  (test_gpu_combine's _check_index measures spans with it)
    from test_bam import read_bai, read_bam, reg2bins, voffset_to_u
    from test_gpu_combine import _check_index
    refine, transcripts, given = M.CASES[name]
    r = route(name)
    assert sorted(os.path.join(r["call"], f) for f in os.listdir(r["call"])) == M.output_names(os.path.join(r["call"], "o"), refine, transcripts, given)
    _same_files(r["call"], r["steps"])
    for f in os.listdir(r["call"]):
        if f.endswith(".bai"):
            _check_index(os.path.join(r["call"], f[:-4]), read_bam, read_bai, reg2bins, voffset_to_u, n_queries=6)
    if transcripts:
        mode = "PARAsuite" if refine else "BWA"
        assert read_bam(os.path.join(r["call"], "o.%s-transcript.bam" % mode))[0].startswith("@HD\tVN:1.6\tSO:queryname\n")
        assert not os.path.exists(os.path.join(r["call"], "o.%s-transcript.bam.bai" % mode))
    # the stats of the call against the stats of the single steps
    st, exp = r["st"], r["exp"]
    assert st["n_reads"] == exp["n_reads"] == route.data["n_route_reads"]
    for k in ("first", "refine", "transcript"):
        got = {x: st[k][x] for x in ("n_in", "n_out")}
        assert got == (exp[k] or dict(n_in=0, n_out=0)), (k, st[k], exp[k])
    for k, f in (("first", "o.BWA-genomic.bam"), ("refine", "o.PARAsuite-genomic.bam"),
                 ("transcript", "o.%s-transcript.bam" % ("PARAsuite" if refine else "BWA"))):
        assert st[k]["bam_bytes"] == (os.path.getsize(os.path.join(r["call"], f)) if exp[k] else 0)
    if transcripts:
        assert {x: st["extract"][x] for x in ("n_records", "n_weak", "n_kept")} == {x: exp["extract"][x] for x in ("n_records", "n_weak", "n_kept")}
        assert {x: st["combine"][x] for x in STAT_KEYS} == {x: exp["combine"][x] for x in STAT_KEYS}
        assert st["combine"]["bam_bytes"] == os.path.getsize(os.path.join(r["call"], "o.combined.bam"))
    else:
        assert not any(st["extract"].values()) and not any(st["combine"].values())
    # each index was read from its files once, the reads file was parsed once
    assert (st["n_index_loads_genome"], st["n_index_loads_transcripts"], st["n_fastq_parses"]) == (1, 1 if transcripts else 0, 1)


@pytest.mark.parametrize("name", ["stock_transcripts", "refine_transcripts"])
def test_against_the_truth(route, name):
    """independent of any restatement: the lifted `read<i>` records lie where the generator cut them, every read is there at most
    once, and the library's own counts meet the conditions the data was made for"""
    refine = M.CASES[name][0]
    r = route(name)
    c = M.route_counts(route.data, os.path.join(r["call"], "o"), refine, r["st"]["extract"]["n_weak"])
    print(name, c)
    M.assert_route_conditions(c, refine)
    assert c["n_lifted_all"] == r["st"]["combine"]["n_lifted"] >= c["n_lifted"]


@pytest.mark.parametrize("env,parses", [(dict(PS_CHUNK_MB="1"), 1), (dict(PARASUITE_GPU_IDS="0,0"), 1), (dict(PS_ROUTE_KEEP_MB="1"), 2)],
                         ids=["pieces", "two_workers", "parsed_again"])
def test_output_does_not_depend_on_the_path(route, monkeypatch, env, parses):
    r = route("refine_transcripts")
    assert os.path.getsize(route.data["route_fastq"]) > 1 << 20            # 1 MB pieces are several; a 1 MB bound is below the input
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    where = os.path.join(route.dir, "vary." + "".join(env))
    st = route.call("refine_transcripts", where)
    _same_files(where, r["call"])
    assert st["n_fastq_parses"] == parses and st["n_index_loads_genome"] == 1 and st["n_index_loads_transcripts"] == 1
    shutil.rmtree(where)


def test_trap_reads_carry_the_names_of_a_second_parse(route):
    from test_bam import read_bam
    r = route("refine_transcripts")
    names = lambda d, f: [x["name"] for x in read_bam(os.path.join(d, f))[2]]
    seen = 0
    for f, strip in (("o.BWA-genomic.bam", 1), ("o.PARAsuite-genomic.bam", 1), ("o.PARAsuite-transcript.bam", 2)):
        got = names(r["call"], f)
        assert got == names(r["steps"], f)
        expect = {M.strip_once(t) if strip == 1 else M.strip_once(M.strip_once(t)) for t in route.data["trap_names"]}
        traps = {n for n in got if n.startswith("trap")}
        assert traps and traps <= expect, (f, traps)
        seen += len(traps)
    t = set(names(r["call"], "o.PARAsuite-transcript.bam"))
    g = set(names(r["call"], "o.PARAsuite-genomic.bam"))
    assert "trapE" in t and "trapF/2" not in t and "trapC/1" in g and "trapK/3" in (t | g)   # /1/2 loses one suffix per parse; /3 is no suffix
    # lower-case bases come out in upper case, an IUPAC base as N, in whichever file the read landed
    found = {}
    for f in ("o.BWA-genomic.bam", "o.PARAsuite-genomic.bam", "o.PARAsuite-transcript.bam"):
        for x in read_bam(os.path.join(r["call"], f))[2]:
            if x["name"] in ("trapG", "trapH", "trapI", "trapJ", "trapN"):
                assert set(x["seq"]) <= set("ACGTN"), x
                assert x["name"] not in ("trapI", "trapJ") or x["seq"].count("N") == 1, x
                found[x["name"]] = f
    assert "trapG" in found and "trapH" in found, found
    assert seen >= 12


def test_fasta_reads_with_transcripts_fail_as_the_extraction_does(route, tmp_path):
    import capi
    fa = str(tmp_path / "reads.fa")
    with open(route.data["route_fastq"]) as f, open(fa, "w") as o:
        lines = f.read().split("\n")
        for i in range(0, 4 * 400, 4):
            o.write(">" + lines[i][1:] + "\n" + lines[i + 1] + "\n")
    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(capi.PsError, match="first pass: extract: .*no QUAL"):
        capi.ps_map_route(fa, route.data["genome_fa"], str(out / "o"), transcripts_fa=route.data["transcripts_fa"], threads=4)
    assert os.listdir(str(out)) == []


def test_failure_after_two_passes_leaves_nothing(route, tmp_path):
    """a transcript header with fewer than six '|' fields: both passes run, the lift refuses"""
    import capi
    r = route("stock_transcripts")
    bad = str(tmp_path / "bad_transcripts.fa")
    with open(route.data["transcripts_fa"]) as f, open(bad, "w") as o:
        for line in f:
            o.write("|".join(line.split("|")[:5]) + "\n" if line.startswith(">") else line)
    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(capi.PsError, match="ps_map_route: combine: .*fewer than six") as ei:
        capi.ps_map_route(route.data["route_fastq"], route.data["genome_fa"], str(out / "o"), transcripts_fa=bad, threads=4)
    assert "ps_map_route: combine:" in str(ei.value)
    assert os.listdir(str(out)) == []
    assert sorted(p for p in os.listdir(str(tmp_path)) if not p.startswith("bad_transcripts.fa")) == ["out"]   # beside the outputs: index files only
    st = capi.ps_map_route(route.data["route_fastq"], route.data["genome_fa"], str(out / "o"), transcripts_fa=route.data["transcripts_fa"], threads=4)
    _same_files(str(out), r["call"])
    assert st["combine"]["n_lifted"] == r["st"]["combine"]["n_lifted"]


def test_nothing_stays_resident(route, tmp_path):
    """free device memory after the call is what it was before, within the noise of that reading; a ps_map afterwards works.
    The noise is the difference of two readings with no library call between them but a small torch allocation, a
    synchronisation and its release: what the runtime and torch's caching allocator move on their own."""
    import torch
    import capi
    r = route("refine_transcripts")                        # the runtime's own one-off allocations (code objects, queues) are made
    torch.cuda.synchronize()
    free = lambda: torch.cuda.mem_get_info(0)[0]
    a = free()
    x = torch.zeros(1024, device="cuda:0")
    torch.cuda.synchronize()
    del x
    b = free()
    noise = abs(a - b)
    st = route.call("refine_transcripts", str(tmp_path / "again"))
    torch.cuda.synchronize()
    after = free()
    print("free before %d %d, after %d" % (a, b, after))
    assert st["n_index_loads_genome"] == 1 and st["n_index_loads_transcripts"] == 1
    assert abs(after - b) <= noise, (a, b, after)
    _same_files(str(tmp_path / "again"), r["call"])
    sam = str(tmp_path / "after.sam")
    capi.ps_map(4, "2", None, None, route.data["genome_fa"], route.data["route_fastq"], sam)
    assert sum(1 for l in open(sam) if not l.startswith("@")) == route.data["n_route_reads"]
