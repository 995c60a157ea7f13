"""--unaligned, --ref-refine and ps_route_opts2 without a GPU: the restatement tests/map_route_flags.py with the oracle as the
mapper, pinned to its own answers; the struct's size rule, the refusals made before anything is touched and the mirror."""
import ctypes as C
import os
import shutil

import pytest

import map_route as M
import map_route_flags as F
from test_capi_cpu import _no_gpu


class CopyingOrc(M.OrcMapper):
    """the oracle as the mapper; every unfiltered genomic BAM it leaves is also copied aside, as the mapper wrote it"""

    def __init__(self, aside):
        super().__init__()
        self.aside, self.copies = aside, {}

    def map(self, mm, ep, ip, ref, fq, out_bam, min_mapq):
        st = super().map(mm, ep, ip, ref, fq, out_bam, min_mapq)
        if min_mapq == 0 and "-genomic" in out_bam:
            self.copies[os.path.basename(out_bam)] = shutil.copyfile(out_bam, os.path.join(self.aside, os.path.basename(out_bam)))
        return st


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return M.make_data(str(tmp_path_factory.mktemp("route_flags")))


def _run(data, tmp_path, name, **kw):
    out, aside = tmp_path / name, tmp_path / (name + ".aside")
    out.mkdir(); aside.mkdir()
    mapper = CopyingOrc(str(aside))
    st = F.route_by_steps_flags(mapper, data, str(out / "o"), keep_unaligned=True, **kw)
    return str(out / "o"), mapper, st


def _listed(prefix, refine, transcripts):
    d = os.path.dirname(prefix)
    want = [f for f in F.output_names(prefix, refine, transcripts, False, True) if ".combined." not in f]     # the oracle's lift stays in memory
    assert sorted(os.path.join(d, f) for f in os.listdir(d)) == want


def test_stock_unaligned_is_empty(data, tmp_path):
    from test_bam import read_bam
    prefix, mapper, st = _run(data, tmp_path, "stock")
    _listed(prefix, False, False)
    assert os.path.getsize(prefix + ".unaligned.fastq") == 0 and st["extract"]["n_weak"] == 0
    recs = read_bam(prefix + ".BWA-genomic.bam")[2]
    assert recs and all(r["mapq"] >= 10 for r in recs) and st["extract"]["n_kept"] == len(recs) == st["first"]["n_out"]


def test_refine_unaligned_holds_the_weak_records_in_sorted_order(data, tmp_path):
    import capi
    from test_bam import read_bam
    prefix, mapper, st = _run(data, tmp_path, "refine", refine=True)
    _listed(prefix, True, False)
    unfiltered = mapper.copies["o.PARAsuite-genomic.bam"]
    capi.ps_bam_sort(unfiltered, unfiltered + ".sorted", threads=4)
    recs = read_bam(unfiltered + ".sorted")[2]
    assert len(recs) == data["n_route_reads"]
    weak = [r["name"] for r in recs if r["mapq"] < 10]
    assert len(weak) >= 1000 and F.fastq_names(prefix + ".unaligned.fastq") == weak
    kept = read_bam(prefix + ".PARAsuite-genomic.bam")[2]
    assert [r["name"] for r in kept] == [r["name"] for r in recs if r["mapq"] >= 10]
    key = [(r["ref"] & 0xffffffff, r["pos"]) for r in kept]
    assert key == sorted(key)
    capi.ps_bam_index(prefix + ".PARAsuite-genomic.bam")                 # the .bai is the one of the file as it ended up (deviation 1)
    assert os.path.exists(prefix + ".PARAsuite-genomic.bam.bai")


@pytest.mark.parametrize("refine", [False, True], ids=["stock", "refine"])
def test_transcripts_unaligned_is_the_first_extraction(data, tmp_path, refine):
    import capi
    prefix, mapper, st = _run(data, tmp_path, "t", refine=refine, transcripts=True)
    _listed(prefix, refine, True)
    first = mapper.copies["o.%s-genomic.bam" % ("PARAsuite" if refine else "BWA")]       # the file :299-302 / :371-374 read, in input order
    ex = capi.ps_extract_weak_reads(first, first + ".kept", first + ".fq", 10)
    assert open(prefix + ".unaligned.fastq", "rb").read() == open(first + ".fq", "rb").read()
    assert ex["n_weak"] == st["extract"]["n_weak"] >= 1000 and st["transcript"]["n_in"] == ex["n_weak"]


def test_ref_refine_same_genome_other_file(data, tmp_path):
    """a refine reference that is the same sequences in another file: the profile is taken and the refine pass maps against IT,
    and every file equals the route without the flag"""
    other = F.write_other_width(data["genome_fa"], str(tmp_path / "other_genome.fa"))
    seen = []

    class Spy(M.OrcMapper):
        def map(self, mm, ep, ip, ref, fq, out_bam, min_mapq):
            seen.append(("map", os.path.basename(out_bam), ref))
            return super().map(mm, ep, ip, ref, fq, out_bam, min_mapq)

        def profile(self, bam, ref, max_len):
            seen.append(("profile", os.path.basename(bam), ref))
            return super().profile(bam, ref, max_len)

    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    F.route_by_steps_flags(Spy(), data, str(tmp_path / "a" / "o"), refine=True, ref_refine=other)
    assert seen == [("map", "o.BWA-genomic.bam", data["genome_fa"]), ("profile", "o.BWA-genomic.bam", other), ("map", "o.PARAsuite-genomic.bam", other)]
    M.route_by_steps(M.OrcMapper(), data, str(tmp_path / "b" / "o"), refine=True)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    from test_bam import read_bam
    for f in sorted(os.listdir(tmp_path / "a")):
        if f.endswith(".bam"):
            assert read_bam(str(tmp_path / "a" / f))[:3] == read_bam(str(tmp_path / "b" / f))[:3], f
        elif not f.endswith(".bai"):
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    seen.clear()
    (tmp_path / "c").mkdir()
    F.route_by_steps_flags(Spy(), data, str(tmp_path / "c" / "o"), refine=False, ref_refine=other)      # without refine it is never read
    assert [s[2] for s in seen] == [data["genome_fa"]]


# ---- the struct and the refusals ----------------------------------------------------------------------------------------------
def _inputs(d):
    fq, fa, ep = (os.path.join(d, x) for x in ("r.fq", "g.fa", "x.errorprofile"))
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    open(fa, "w").write(">c\nACGTACGT\n")
    open(ep, "w").write("1\t0\t0\t0\t\n0\t1\t0\t0\t\n0\t0\t1\t0\t\n0\t0\t0\t1\t\n")
    return fq, fa, ep


def _listing(d):
    return sorted((p, os.path.getsize(os.path.join(d, p))) for p in os.listdir(d))


def test_struct_size_rule(tmp_path):
    import capi
    d = str(tmp_path)
    fq, fa, ep = _inputs(d)
    before = _listing(d)
    size = C.sizeof(capi.RouteOpts2)
    for bad in (0, 2, 23 + 3, size + 4, 28, 92, 100):                # no multiple of 4; one word too long; inside a pointer
        with pytest.raises(capi.PsError, match="ps_map_route_opts: struct_size %d " % bad):
            capi.ps_map_route_opts(fq, fa, os.path.join(d, "o"), struct_size=bad)
    # a struct that ends before the fields it would need keeps their defaults: no reads file, and the flags beyond it are not read
    with pytest.raises(capi.PsError, match=r"ps_map_route_opts: the reads file \(-q\) is required"):
        capi.ps_map_route_opts(fq, fa, os.path.join(d, "o"), struct_size=24)
    assert _listing(d) == before


@pytest.mark.skipif(not _no_gpu(), reason="the second call maps where there is a device")
def test_unaligned_counts_as_an_output_only_when_the_struct_holds_the_flag(tmp_path):
    import capi
    d = str(tmp_path)
    fq, fa, ep = _inputs(d)
    os.link(fq, os.path.join(d, "u.unaligned.fastq"))        # U IS the reads file, by another path
    before = _listing(d)
    with pytest.raises(capi.PsError, match="ps_map_route_opts: the output .*unaligned.fastq would overwrite the input"):
        capi.ps_map_route_opts(fq, fa, os.path.join(d, "u"), keep_unaligned=True)
    with pytest.raises(capi.PsError, match="no HIP device"):          # past the comparison: keep_unaligned lies beyond the 88 bytes
        capi.ps_map_route_opts(fq, fa, os.path.join(d, "u"), keep_unaligned=True, struct_size=capi.ROUTE_OPTS_OLD_SIZE)
    assert _listing(d) == before


def test_refusals_touch_nothing(tmp_path):
    import capi
    d = str(tmp_path)
    fq, fa, ep = _inputs(d)
    before = _listing(d)
    call = lambda **kw: capi.ps_map_route_opts(fq, fa, os.path.join(d, "o"), **kw)
    with pytest.raises(capi.PsError, match="ps_map_route_opts: an error profile without refine: nothing to map"):
        call(error_profile=ep)
    with pytest.raises(capi.PsError, match="ps_map_route_opts: ps_search_opts: max_gap_opens .*accepted: 0 to 7"):
        call(search=dict(max_gap_opens=8))
    with pytest.raises(capi.PsError, match="max_seed_diff .*accepted: 0 to 511"):      # a profile pass will run: its range holds too
        call(refine=True, search=dict(max_seed_diff=600))
    with pytest.raises(capi.PsError, match="would overwrite the input"):               # the refine reference is an input
        call(refine=True, ref_refine=os.path.join(d, "o.PARAsuite-genomic.bam.route-tmp"))
    bad = capi.SearchOpts(); bad.struct_size = 56
    with pytest.raises(capi.PsError, match="ps_search_opts: struct_size 56"):
        call(search=bad)
    assert _listing(d) == before


def test_main_mirror_takes_the_new_call_only_when_asked(monkeypatch):
    import __graft_entry__ as ge
    mod = ge.load_package()
    seen = {}

    def fake(name):
        def f(reads_fq, ref_fa, out_prefix, **kw):
            seen.clear(); seen.update(kw, call=name)
            return dict(n_reads=1)
        return f

    monkeypatch.setattr(mod.capi, "ps_map_route", fake("ps_map_route"))
    monkeypatch.setattr(mod.capi, "ps_map_route_opts", fake("ps_map_route_opts"))
    m = mod.mapping.Main()
    m.map("r.fq", "g.fa", "o", refine=True)
    assert seen["call"] == "ps_map_route" and "keep_unaligned" not in seen
    m.map("r.fq", "g.fa", "o", refine=True, keepUnaligned=True)
    assert seen["call"] == "ps_map_route_opts" and seen["keep_unaligned"] is True and seen["ref_refine"] is None and seen["search"] is None
    m.map("r.fq", "g.fa", "o", referenceRefineFileName="h.fa", search=dict(seed_len=20))
    assert (seen["call"], seen["ref_refine"], seen["search"], seen["keep_unaligned"]) == ("ps_map_route_opts", "h.fa", dict(seed_len=20), False)
