"""ps_combine_genome_transcript on the GPU: the hand-worked cases of tests/test_combine_cpu.py from SAM and from BAM, record
for record and counter for counter what the restatement tests/java_combine.py gives; the sorted form against ps_bam_sort and
the independent index reader of tests/test_bam.py; and the whole `map -t` route (Main.java:363-416) on generated data, every
step through the library, against the restatement AND against where the generator cut the reads."""
import gzip
import os

import numpy as np
import pytest

import combine_route as R
import java_combine as J
from test_combine_cpu import CASES, ERRORS, GENOME_RECS, g_header, t_header

pytestmark = pytest.mark.gpu


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


def _stats_equal(st, exp, out):
    assert {k: st[k] for k in J.STAT_KEYS} == exp, (st, exp)
    assert st["bam_bytes"] == os.path.getsize(out) and set(st) == set(J.STAT_KEYS) | {"bam_bytes"}


@pytest.mark.parametrize("from_bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked_cases(tmp_path, name, from_bam):
    import capi
    from test_bam import read_bam
    body, sq, lifted, _ = CASES[name]
    g, t, out = _write(str(tmp_path / "g.sam"), g_header(sq) + GENOME_RECS), _write(str(tmp_path / "t.sam"), t_header() + body), str(tmp_path / "c.bam")
    exp_text, exp_refs, exp, exp_st = J.combine(J.parse_sam(open(g).read()), J.parse_sam(open(t).read()))
    assert len(exp) == 2 + len(lifted)                                   # the hand-worked answer, through the restatement
    if from_bam:
        capi.ps_sam_to_bam(g, g[:-3] + "bam")
        capi.ps_sam_to_bam(t, t[:-3] + "bam")
        g, t = g[:-3] + "bam", t[:-3] + "bam"
    st = capi.ps_combine_genome_transcript(g, t, out, threads=3)
    text, refs, recs, _ = read_bam(out)
    assert text == exp_text and refs == exp_refs
    assert J.same_records(recs, exp) is None, J.same_records(recs, exp)
    _stats_equal(st, exp_st, out)
    assert not os.path.exists(out + ".bai")


def test_all_cases_in_one_file_sorted_and_indexed(tmp_path):
    """every hand-worked case as a read group of ONE name-sorted file (names made distinct): the unsorted and the sorted form,
    the latter byte for byte what ps_bam_sort makes of the former, and its .bai read by the independent reader"""
    import capi
    from test_bam import read_bai, read_bam, reg2bins, voffset_to_u
    sq = CASES["one_exon_fwd"][1]
    body = ""
    for i, name in enumerate(sorted(CASES)):
        if CASES[name][1] != sq:
            continue
        for line in CASES[name][0].splitlines(True):
            body += "c%02d_%s" % (i, line)
    g, t = _write(str(tmp_path / "g.sam"), g_header(sq) + GENOME_RECS), _write(str(tmp_path / "t.sam"), t_header() + body)
    u, s, su = (str(tmp_path / x) for x in ("u.bam", "s.bam", "su.bam"))
    genome, transcript = J.parse_sam(open(g).read()), J.parse_sam(open(t).read())
    st_u = capi.ps_combine_genome_transcript(g, t, u)
    st_s = capi.ps_combine_genome_transcript(g, t, s, sort_by_coordinate=True, write_index=True)
    for path, st, sort in ((u, st_u, False), (s, st_s, True)):
        exp_text, exp_refs, exp, exp_st = J.combine(genome, transcript, sort)
        text, refs, recs, starts = read_bam(path)
        assert text == exp_text and refs == exp_refs and J.same_records(recs, exp) is None, J.same_records(recs, exp)
        _stats_equal(st, exp_st, path)
    assert st_u["n_lifted"] >= 12 and st_u["n_groups_ambiguous"] >= 2 and st_u["n_strand_flipped"] >= 3
    capi.ps_bam_sort(u, su)
    assert gzip.decompress(open(s, "rb").read()) == gzip.decompress(open(su, "rb").read())
    _check_index(s, read_bam, read_bai, reg2bins, voffset_to_u)
    with pytest.raises(capi.PsError, match="coordinate-sorted"):
        capi.ps_combine_genome_transcript(g, t, str(tmp_path / "x.bam"), sort_by_coordinate=False, write_index=True)
    assert not os.path.exists(str(tmp_path / "x.bam"))


def _check_index(bam, read_bam, read_bai, reg2bins, voffset_to_u, n_queries=40):
    """region queries through the binning and linear index against a scan of the records (as tests/test_bam.py does)"""
    _, refs, recs, starts = read_bam(bam)
    idx, n_no_coor = read_bai(bam + ".bai")
    assert len(idx) == len(refs) and n_no_coor == sum(r["ref"] < 0 for r in recs)
    span = lambda r: (r["pos"], r["pos"] + (J.ref_length(r["cigar"]) or 1))
    rng = np.random.default_rng(2)
    for tid, (name, ln) in enumerate(refs):
        bins, lin = idx[tid]
        mine = [r for r in recs if r["ref"] == tid]
        for _ in range(n_queries if mine else 1):
            beg = int(rng.integers(0, ln - 1)); end = min(ln, beg + int(rng.integers(1, 40000)))
            want = sorted({r["name"] + str(r["pos"]) for r in mine if span(r)[0] < end and span(r)[1] > beg})
            min_off = lin[beg >> 14] if (beg >> 14) < len(lin) else (lin[-1] if lin else 0)
            got = set()
            for b in reg2bins(beg, end):
                for cb, ce in bins.get(b, []):
                    if ce <= min_off:
                        continue
                    u0, u1 = voffset_to_u(starts, cb), voffset_to_u(starts, ce)
                    got |= {r["name"] + str(r["pos"]) for r in mine if u0 <= r["u0"] < u1 and span(r)[0] < end and span(r)[1] > beg}
            assert sorted(got) == want, (name, beg, end)
        if mine:
            assert bins[37450][1][0] == sum(not r["flag"] & 4 for r in mine)


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_errors_write_nothing(tmp_path, name):
    import capi
    head, body = ERRORS[name]
    g, t = _write(str(tmp_path / "g.sam"), g_header() + GENOME_RECS), _write(str(tmp_path / "t.sam"), head + body)
    with pytest.raises(J.CombineError):
        J.combine(J.parse_sam(open(g).read()), J.parse_sam(open(t).read()))
    with pytest.raises(capi.PsError, match="queryname" if name == "not_name_sorted" else "TZ"):
        capi.ps_combine_genome_transcript(g, t, str(tmp_path / "c.bam"), sort_by_coordinate=True, write_index=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["g.sam", "t.sam"]


def test_a_failed_call_leaves_the_output_from_before(tmp_path):
    """the output files exist before a call that fails on its input: they are still there with their old bytes, and no temporary is"""
    import capi
    head, body = ERRORS[sorted(ERRORS)[0]]
    g, t = _write(str(tmp_path / "g.sam"), g_header() + GENOME_RECS), _write(str(tmp_path / "t.sam"), head + body)
    noq = _write(str(tmp_path / "noq.sam"), g_header() + "noq\t0\tchr1\t5\t3\t4M\t*\t0\t0\tACGT\t*\n")     # a weak record without QUAL
    old = {n: ("from before: " + n).encode() for n in ("c.bam", "c.bam.bai", "k.bam", "w.fq")}
    for n, text in old.items():
        (tmp_path / n).write_bytes(text)
    with pytest.raises(capi.PsError):
        capi.ps_combine_genome_transcript(g, t, str(tmp_path / "c.bam"), sort_by_coordinate=True, write_index=True)
    with pytest.raises(capi.PsError, match="noq has MAPQ below 10 and no QUAL"):
        capi.ps_extract_weak_reads(noq, str(tmp_path / "k.bam"), str(tmp_path / "w.fq"), 10)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(["g.sam", "t.sam", "noq.sam"] + list(old))
    assert {n: (tmp_path / n).read_bytes() for n in old} == old
    with pytest.raises(capi.PsError, match="would overwrite the input"):
        capi.ps_combine_genome_transcript(g, t, g)
    assert open(g).read() == g_header() + GENOME_RECS


def test_route_end_to_end(workdir):
    """ps_map_to_bam (genome, filter 0) -> ps_extract_weak_reads (10) -> ps_map_to_bam (transcripts, MAPQ 1) -> ps_bam_sort -n ->
    ps_combine_genome_transcript (sorted, indexed): (a) equals the restatement on the same two intermediate files, (b) lies
    where the generator cut the reads -- independent of the restatement --, (c) holds every read at most once"""
    import capi
    from test_bam import read_bai, read_bam, reg2bins, voffset_to_u
    d = os.path.join(workdir, "combine_route")
    os.makedirs(d, exist_ok=True)
    data = R.make_data(d)
    p = lambda x: os.path.join(d, x)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    st = capi.ps_map_to_bam(4, "2", None, None, data["genome_fa"], data["fastq"], p("g.bam"), min_mapq=0)
    assert st["n_out"] == data["n_reads"]
    ex = capi.ps_extract_weak_reads(p("g.bam"), p("g.kept.bam"), p("weak.fq"), 10, threads=4)
    assert ex["n_records"] == data["n_reads"] and ex["n_weak"] > 1000 and ex["n_weak"] + ex["n_kept"] == data["n_reads"]
    os.replace(p("g.kept.bam"), p("g.bam"))                                # Main.java:376-377
    capi.ps_map_to_bam(4, "2", None, None, data["transcripts_fa"], p("weak.fq"), p("t.bam"), min_mapq=1)
    capi.ps_bam_sort(p("t.bam"), p("t.byname.bam"), by_name=True, threads=4)
    st = capi.ps_combine_genome_transcript(p("g.bam"), p("t.byname.bam"), p("combined.bam"), sort_by_coordinate=True, write_index=True, threads=4)
    genome, transcript = read_bam(p("g.bam"))[:3], read_bam(p("t.byname.bam"))[:3]
    text, refs, recs, _ = read_bam(p("combined.bam"))
    # (a)
    exp_text, exp_refs, exp, exp_st = J.combine(genome, transcript, sort_by_coordinate=True)
    assert text == exp_text and refs == exp_refs and J.same_records(recs, exp) is None, J.same_records(recs, exp)
    _stats_equal(st, exp_st, p("combined.bam"))
    # (b)
    c = R.check_lifted(data, (text, refs, recs), transcript[2])
    print(st, c)
    assert c["n_lifted"] == st["n_lifted"]
    R.assert_conditions(c)
    # (c)
    R.assert_at_most_once(data, recs)
    _check_index(p("combined.bam"), read_bam, read_bai, reg2bins, voffset_to_u, n_queries=8)


def test_mirrors(tmp_path):
    """the Java-named mirrors: extractReads, then combine (sorted, as htsjdk's writer does)"""
    import __graft_entry__ as ge
    from test_bam import read_bam
    mod = ge.load_package()
    body, sq, lifted, _ = CASES["two_junctions_rev"]
    g, t = _write(str(tmp_path / "g.sam"), g_header(sq) + GENOME_RECS), _write(str(tmp_path / "t.sam"), t_header() + body)
    ex = mod.mapping.ExtractWeakMappingReads().extractReads(g, str(tmp_path / "g.kept.bam"), str(tmp_path / "weak.fq"), 30)
    assert (ex["n_weak"], ex["n_kept"]) == (1, 1) and open(str(tmp_path / "weak.fq")).read().startswith("@g2\n")
    st = mod.mapping.CombineGenomeTranscript().combine(str(tmp_path / "g.kept.bam"), t, str(tmp_path / "c.bam"))
    text, _, recs, _ = read_bam(str(tmp_path / "c.bam"))
    assert st["n_lifted"] == 1 and text.startswith("@HD\tVN:1.6\tSO:coordinate\n")
    assert [(r["name"], r["pos"] + 1, r["cigar"], r["mapq"]) for r in recs] == [("g1", 500, "20M", 37), ("r", 5090, "10M900N100M900N10M", 10)]
