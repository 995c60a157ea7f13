"""ps_map_route without a GPU: the symbol (its two structs: test_capi_cpu.py), every refusal that is made before anything is touched, the no-device
failure, the `Main` mirror -- and the generated data of tests/map_route.py held to the route's conditions with the oracle as
the mapper (that last test checks the data, not the feature)."""
import os

import pytest

import map_route as M
from test_capi_cpu import _declared, _no_gpu


def test_symbol_in_header_library_and_exports():
    import capi
    names = _declared()
    assert "ps_map_route" in names and hasattr(capi.lib(), "ps_map_route")
    assert sorted(capi.EXPORTS) == names


def _listing(d):
    return sorted((p, os.path.getsize(os.path.join(d, p))) for p in os.listdir(d))


def test_refusals_touch_nothing(tmp_path):
    import capi
    d = str(tmp_path)
    fq, fa, ep = (os.path.join(d, x) for x in ("r.fq", "g.fa", "x.errorprofile"))
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    open(fa, "w").write(">c\nACGTACGT\n")
    open(ep, "w").write("1\t0\t0\t0\t\n0\t1\t0\t0\t\n0\t0\t1\t0\t\n0\t0\t0\t1\t\n")
    P = os.path.join(d, "out")
    os.link(fq, P + ".BWA-genomic.bam")                      # an output name that IS the reads file, by another path
    before = _listing(d)
    with pytest.raises(capi.PsError, match="nothing to map"):
        capi.ps_map_route(fq, fa, os.path.join(d, "o2"), error_profile=ep)
    with pytest.raises(capi.PsError, match="indel profile without an error profile"):
        capi.ps_map_route(fq, fa, os.path.join(d, "o2"), refine=True, indel_profile=ep)
    with pytest.raises(capi.PsError, match="would overwrite the input"):                # a temporary name counts too
        capi.ps_map_route(fq, fa, os.path.join(d, "o3"), refine=True, error_profile=ep, transcripts_fa=os.path.join(d, "o3.combined.bam.route-tmp.bai"))
    for kw, what in ((dict(reads_fq=None), "reads file"), (dict(ref_fa=""), "reference"), (dict(out_prefix=None), "output prefix")):
        args = dict(reads_fq=fq, ref_fa=fa, out_prefix=os.path.join(d, "o2"))
        args.update(kw)
        with pytest.raises(capi.PsError, match=what + r" \(-[qro]\) is required"):
            capi.ps_map_route(**args)
    with pytest.raises(capi.PsError, match="would overwrite the input"):
        capi.ps_map_route(fq, fa, P)
    assert _listing(d) == before


def test_an_output_that_names_the_transcripts_is_refused(tmp_path):
    import capi
    d = str(tmp_path)
    fq, fa = os.path.join(d, "r.fq"), os.path.join(d, "g.fa")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    open(fa, "w").write(">c\nACGTACGT\n")
    tfa = os.path.join(d, "o.combined.bam")
    open(tfa, "w").write(">a|b|1|1|4|1\nACGT\n")
    before = _listing(d)
    with pytest.raises(capi.PsError, match="would overwrite the input"):
        capi.ps_map_route(fq, fa, os.path.join(d, "o"), transcripts_fa=tfa)
    assert _listing(d) == before


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_fails_without_a_device_and_leaves_nothing(tmp_path):
    import capi
    d = str(tmp_path)
    fq, fa = os.path.join(d, "r.fq"), os.path.join(d, "g.fa")
    open(fq, "w").write("@r\nACGT\n+\nIIII\n")
    open(fa, "w").write(">c\nACGTACGT\n")
    before = _listing(d)
    for kw in (dict(), dict(refine=True, transcripts_fa=fa)):
        with pytest.raises(capi.PsError, match="no HIP device"):
            capi.ps_map_route(fq, fa, os.path.join(d, "out"), **kw)
    assert _listing(d) == before


def test_main_mirror(monkeypatch):
    import __graft_entry__ as ge
    mod = ge.load_package()
    seen = {}

    def fake(reads_fq, ref_fa, out_prefix, **kw):
        seen.clear()
        seen.update(kw, reads_fq=reads_fq, ref_fa=ref_fa, out_prefix=out_prefix)
        return dict(n_reads=7)

    monkeypatch.setattr(mod.capi, "ps_map_route", fake)
    m = mod.mapping.Main()
    assert m.map("r.fq", "g.fa", "o") == "o.BWA-genomic.bam"
    assert seen == dict(reads_fq="r.fq", ref_fa="g.fa", out_prefix="o", transcripts_fa=None, threads=1, refine=False, max_read_len=101,
                        mapq_genomic=10, mapq_transcript=1, bwa_mm="2", parasuite_mm="-1", error_profile=None, indel_profile=None)
    assert m.stats == dict(n_reads=7)
    assert m.map("r.fq", "g.fa", "o", transcriptFileName="t.fa") == "o.combined.bam" and seen["transcripts_fa"] == "t.fa"
    assert m.map("r.fq", "g.fa", "o", refine=True) == "o.PARAsuite-genomic.bam" and seen["refine"] is True
    assert m.map("r.fq", "g.fa", "o", "t.fa", refine=True) == "o.combined.bam"
    assert m.map("r.fq", "g.fa", "o", None, 3, 76, 12, 2, True, "3", "4", "x.ep", "x.ip") == "o.PARAsuite-genomic.bam"
    assert seen == dict(reads_fq="r.fq", ref_fa="g.fa", out_prefix="o", transcripts_fa=None, threads=3, refine=True, max_read_len=76,
                        mapq_genomic=12, mapq_transcript=2, bwa_mm="3", parasuite_mm="4", error_profile="x.ep", indel_profile="x.ip")

    def failing(*a, **kw):
        raise mod.capi.PsError("ps_map_route: combine: broken")

    monkeypatch.setattr(mod.capi, "ps_map_route", failing)
    with pytest.raises(mod.mapping.ExternalCallErrorException) as ei:
        m.map("r.fq", "g.fa", "o")
    assert "map -q r.fq" in ei.value.getMappingCommand() and "combine" in ei.value.getMappingCommand()


def test_binding_marshals_every_field(monkeypatch):
    """ps_map_route() of capi.py fills ps_route_opts field by field (seen through a stand-in for the library's entry point)"""
    import capi
    got = {}

    class Lib:
        class ps_map_route:
            argtypes = None

            def __new__(cls, o, st):
                o = o._obj
                got.update({f: getattr(o, f) for f, _ in capi.RouteOpts._fields_})
                return 0

    monkeypatch.setattr(capi, "lib", lambda: Lib)
    st = capi.ps_map_route("r.fq", "g.fa", "o", "t.fa", 3, True, 76, 12, 2, "3", -1, "e", "i")
    assert got == dict(reads_fq=b"r.fq", ref_fa=b"g.fa", out_prefix=b"o", transcripts_fa=b"t.fa", bwa_mm=b"3", parasuite_mm=b"-1",
                       error_profile=b"e", indel_profile=b"i", threads=3, refine=1, max_read_len=76, mapq_genomic=12, mapq_transcript=2)
    assert st["n_reads"] == 0 and st["combine"]["n_lifted"] == 0 and st["first"] == dict(n_in=0, n_out=0, bam_bytes=0)


def test_route_data_with_the_oracle_mapper(tmp_path):
    """the stock and the refine route, transcripts given, call by call with the oracle as the mapper: the generated data meets the
    conditions the GPU tier asserts on the library's own counts"""
    d = str(tmp_path)
    data = M.make_data(d)
    for refine in (False, True):
        out = os.path.join(d, "refine" if refine else "stock")
        os.makedirs(out)
        prefix = os.path.join(out, "o")
        orc_mapper = M.OrcMapper()
        st = M.route_by_steps(orc_mapper, data, prefix, refine=refine, transcripts=True)
        assert sorted(os.path.join(out, f) for f in os.listdir(out)) == [f for f in M.output_names(prefix, refine, True, False) if ".combined." not in f]
        assert st["n_reads"] == data["n_route_reads"] == st["extract"]["n_records"]
        c = M.route_counts(data, prefix, refine, st["extract"]["n_weak"], combined=orc_mapper.combined)
        print("refine" if refine else "stock", c, st["combine"])
        M.assert_route_conditions(c, refine)
        assert c["n_lifted_all"] == st["combine"]["n_lifted"] >= c["n_lifted"]
