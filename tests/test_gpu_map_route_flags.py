"""ps_map_route_opts on the GPU: --unaligned, --ref-refine and the search options file for file against the call-by-call
restatement through the library's own calls (tests/map_route_flags.py); a struct that holds the old fields only against
ps_map_route; the same calls inside a resident scope."""
import contextlib
import os
import shutil

import pytest

import map_route as M
import map_route_flags as F
from test_gpu_map_route import _same_files, _stream

pytestmark = pytest.mark.gpu

SEARCH = dict(max_gap_opens=0, seed_len=20, max_seed_diff=1, max_alt_hits=0)


@contextlib.contextmanager
def resident_scope(max_references):
    """a resident scope, and an empty one behind it: ps_resident_info() shows the counters of the last scope, and the modules that
    run later (tests/test_gpu_resident.py) start from a process in which no scope has counted anything"""
    import capi
    try:
        with capi.resident(max_references=max_references):
            yield
    finally:
        with capi.resident():
            pass
        assert not any(capi.ps_resident_info()[k] for k in ("active", "n_calls", "n_index_loads"))


@pytest.fixture(scope="module")
def env(workdir):
    import capi
    d = os.path.join(workdir, "map_route_flags")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    other = F.write_other_width(data["genome_fa"], os.path.join(d, "genome_other_width.fa"))      # not indexed: the first call that needs it does
    runs = {}

    def call(where, refine=False, transcripts=False, **kw):
        os.makedirs(where)
        return capi.ps_map_route_opts(data["route_fastq"], data["genome_fa"], os.path.join(where, "o"),
                                      transcripts_fa=data["transcripts_fa"] if transcripts else None, threads=4, refine=refine, **kw)

    def plain(name):
        """ps_map_route without any of the flags, once per case"""
        if name not in runs:
            refine, transcripts, _ = M.CASES[name]
            where = os.path.join(d, name + ".plain")
            os.makedirs(where)
            st = capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(where, "o"),
                                   transcripts_fa=data["transcripts_fa"] if transcripts else None, threads=4, refine=refine)
            runs[name] = (where, st)
        return runs[name]

    def once(key, refine, transcripts, **kw):
        """a call with flags whose files more than one test looks at, once -> (directory, stats)"""
        if key not in runs:
            where = os.path.join(d, key + ".call")
            runs[key] = (where, call(where, refine, transcripts, **kw))
        return runs[key]

    def steps(where, mapper, **kw):
        """the restatement, its single calls inside a resident scope: their output is what it is outside one, byte for byte
        (tests/test_gpu_resident.py), and they do not load every index and allocate every workspace anew"""
        os.makedirs(where)
        with resident_scope(3):
            return F.route_by_steps_flags(mapper, data, os.path.join(where, "o"), **kw)

    class Env:
        pass
    e = Env()
    e.data, e.dir, e.other, e.call, e.plain, e.once, e.steps = data, d, other, call, plain, once, steps
    return e


def _check_bai(d, tmp):
    """every .bai byte for byte what ps_bam_index writes for the file beside it"""
    import capi
    for f in sorted(os.listdir(d)):
        if f.endswith(".bai"):
            copy = os.path.join(tmp, f[:-4])
            shutil.copyfile(os.path.join(d, f[:-4]), copy)
            capi.ps_bam_index(copy, threads=4)
            assert open(copy + ".bai", "rb").read() == open(os.path.join(d, f), "rb").read(), f
            os.remove(copy); os.remove(copy + ".bai")


@pytest.mark.parametrize("name", ["stock", "refine", "refine_transcripts", "stock_transcripts"])
def test_keep_unaligned(env, tmp_path, name):
    refine, transcripts, _ = M.CASES[name]
    b = os.path.join(env.dir, name + ".keep.steps")
    a, st = env.once(name + ".keep", refine, transcripts, keep_unaligned=True)
    exp = env.steps(b, M.LibMapper(4), refine=refine, transcripts=transcripts, keep_unaligned=True)
    assert sorted(os.path.join(a, f) for f in os.listdir(a)) == F.output_names(os.path.join(a, "o"), refine, transcripts, False, True)
    _same_files(a, b)
    _check_bai(a, str(tmp_path))
    U = os.path.join(a, "o.unaligned.fastq")
    assert open(U, "rb").read() == open(os.path.join(b, "o.unaligned.fastq"), "rb").read()
    for k in ("first", "refine", "transcript"):
        assert {x: st[k][x] for x in ("n_in", "n_out")} == (exp[k] or dict(n_in=0, n_out=0)), (k, st[k], exp[k])
    assert {x: st["extract"][x] for x in ("n_records", "n_weak", "n_kept")} == ({x: exp["extract"][x] for x in ("n_records", "n_weak", "n_kept")} if refine or transcripts else dict(n_records=0, n_weak=0, n_kept=0))
    if name == "stock":
        assert os.path.getsize(U) == 0
    else:
        assert len(F.fastq_names(U)) == st["extract"]["n_weak"] >= 1000
    # every other file is what the call writes without the flag; in the refine case too: dropping the weak records from the sorted
    # file leaves what sorting the filtered pass leaves
    plain_dir, _ = env.plain(name)
    for f in os.listdir(plain_dir):
        if f.endswith(".bam"):
            assert _stream(os.path.join(plain_dir, f)) == _stream(os.path.join(a, f)), f
        elif not f.endswith(".bai"):
            assert open(os.path.join(plain_dir, f), "rb").read() == open(os.path.join(a, f), "rb").read(), f


@pytest.mark.parametrize("given,keep", [(False, False), (True, False), (False, True)], ids=["own_profile", "given_profile", "own_profile_unaligned"])
def test_ref_refine(env, tmp_path, given, keep):
    a, b = os.path.join(env.dir, "rr%d%d.call" % (given, keep)), os.path.join(env.dir, "rr%d%d.steps" % (given, keep))
    ep = ip = None
    if given:
        src = os.path.join(env.plain("refine")[0], "o.BWA-genomic.bam")
        ep, ip = str(tmp_path / "g.errorprofile"), str(tmp_path / "g.indelprofile")
        shutil.copyfile(src + ".errorprofile", ep); shutil.copyfile(src + ".indelprofile", ip)
    if keep:
        a, st = env.once("rr.keep", True, False, ref_refine=env.other, keep_unaligned=True)
    else:
        st = env.call(a, True, False, ref_refine=env.other, error_profile=ep, indel_profile=ip)
    assert os.path.exists(env.other + ".bwt")                               # ps_index ran for it
    env.steps(b, M.LibMapper(4), refine=True, ref_refine=env.other, error_profile=ep, indel_profile=ip, keep_unaligned=keep)
    assert sorted(os.path.join(a, f) for f in os.listdir(a)) == F.output_names(os.path.join(a, "o"), True, False, given, keep)
    _same_files(a, b)
    _check_bai(a, str(tmp_path))
    # two references by realpath: each loaded once.  With a given profile nothing maps against ref_fa, so one index is loaded
    assert (st["n_index_loads_genome"], st["n_fastq_parses"]) == ((1, 1) if given else (2, 1))
    # the same sequences: the files are those of the route without the flag
    plain_dir, pst = env.plain("refine")
    assert _stream(os.path.join(a, "o.PARAsuite-genomic.bam")) == _stream(os.path.join(plain_dir, "o.PARAsuite-genomic.bam"))


def test_ref_refine_that_is_no_second_reference(env, tmp_path):
    link = str(tmp_path / "genome_link.fa")                                 # a path to the same file
    os.symlink(env.data["genome_fa"], link)
    st = env.call(str(tmp_path / "same"), True, False, ref_refine=link)
    assert st["n_index_loads_genome"] == 1
    _same_files(str(tmp_path / "same"), env.plain("refine")[0])
    st = env.call(str(tmp_path / "norefine"), False, False, ref_refine=str(tmp_path / "never_read.fa"))      # without refine it is ignored
    assert st["n_index_loads_genome"] == 1
    _same_files(str(tmp_path / "norefine"), env.plain("stock")[0])


def test_ref_refine_without_a_contig_fails_at_the_profile(env, tmp_path):
    import capi
    contigs = sorted(env.data["genome"])
    fewer = F.without_contig(env.data["genome_fa"], str(tmp_path / "fewer.fa"), contigs[1])
    out = tmp_path / "out"
    with pytest.raises(capi.PsError, match="ps_map_route_opts: profile: .*names a sequence the reference does not have"):
        env.call(str(out), True, True, ref_refine=fewer, keep_unaligned=True)
    assert os.listdir(str(out)) == []
    assert sorted(p for p in os.listdir(str(tmp_path)) if not p.startswith("fewer.fa")) == ["out"]     # beside it: the index files ps_index wrote


def test_search_options_reach_every_pass(env, tmp_path):
    b = os.path.join(env.dir, "search.steps")
    a, st = env.once("search", True, True, search=SEARCH)
    env.steps(b, F.LibSearchMapper(SEARCH, 4), refine=True, transcripts=True)
    assert sorted(os.path.join(a, f) for f in os.listdir(a)) == M.output_names(os.path.join(a, "o"), True, True, False)
    _same_files(a, b)
    _check_bai(a, str(tmp_path))
    assert (st["n_index_loads_genome"], st["n_index_loads_transcripts"], st["n_fastq_parses"]) == (1, 1, 1)
    plain_dir, _ = env.plain("refine_transcripts")
    differ = [f for f in sorted(os.listdir(a)) if f.endswith(".bam") and _stream(os.path.join(a, f)) != _stream(os.path.join(plain_dir, f))]
    print("files that differ from the call without search options:", differ)
    assert {"o.BWA-genomic.bam", "o.PARAsuite-genomic.bam", "o.PARAsuite-transcript.bam"} <= set(differ)       # every pass took them


def test_old_fields_only_is_ps_map_route(env, tmp_path):
    import ctypes as C
    import capi
    plain_dir, pst = env.plain("refine_transcripts")
    where = str(tmp_path / "old")
    st = env.call(where, True, True, keep_unaligned=True, search=dict(max_gap_opens=0), struct_size=capi.ROUTE_OPTS_OLD_SIZE)   # the fields beyond are not read
    _same_files(where, plain_dir)
    assert st["extract"] == pst["extract"] and st["combine"]["n_lifted"] == pst["combine"]["n_lifted"]
    with pytest.raises(capi.PsError, match="struct_size %d must be" % (C.sizeof(capi.RouteOpts2) + 4)):
        env.call(str(tmp_path / "long"), True, True, struct_size=C.sizeof(capi.RouteOpts2) + 4)
    assert os.listdir(str(tmp_path / "long")) == []


def test_inside_a_resident_scope(env, tmp_path):
    import capi
    with resident_scope(2):
        st1 = env.call(str(tmp_path / "keep"), True, True, keep_unaligned=True)
        st2 = env.call(str(tmp_path / "rr"), True, False, ref_refine=env.other, keep_unaligned=True)
        st3 = env.call(str(tmp_path / "search"), True, True, search=SEARCH)
        info = capi.ps_resident_info()
    _same_files(str(tmp_path / "keep"), env.once("refine_transcripts.keep", True, True, keep_unaligned=True)[0])
    _same_files(str(tmp_path / "search"), env.once("search", True, True, search=SEARCH)[0])
    _same_files(str(tmp_path / "rr"), env.once("rr.keep", True, False, ref_refine=env.other, keep_unaligned=True)[0])     # the two flags together
    _check_bai(str(tmp_path / "rr"), str(tmp_path))
    # the first call loads genome and transcripts; the second finds the genome and loads the other reference; the third finds or
    # loads again what the scope's two places kept -- never more than one load per reference and call
    assert (st1["n_index_loads_genome"], st1["n_index_loads_transcripts"]) == (1, 1)
    assert st2["n_index_loads_genome"] == 1
    assert st3["n_index_loads_genome"] <= 1 and st3["n_index_loads_transcripts"] <= 1
    assert info["n_calls"] == 3 and info["n_dropped_after_error"] == 0
