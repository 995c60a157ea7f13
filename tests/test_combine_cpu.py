"""CombineGenomeTranscript.combine (CombineGenomeTranscript.java:36-666) as tests/java_combine.py restates it, against
answers worked out by hand on hand-written SAM records, and ps_extract_weak_reads (host code) on a BAM made by ps_sam_to_bam.
The GPU entry point ps_combine_genome_transcript is held to the same records in tests/test_gpu_combine.py, which imports the
cases from here."""
import os

import numpy as np
import pytest

import java_combine as J
from test_capi_cpu import _no_gpu

# transcripts: Gene|Transcript|Chr|exon starts|exon ends|strand; exons of TA / TB are 100 bases with 900-base introns
TA = "GA|TA|1|1000;2000;3000|1099;2099;3099|1"
TA2 = "GA|TA2|1|1000;2000|1099;2099|1"
TB = "GB|TB|1|5000;6000;7000|5099;6099;7099|-1"
TC = "GC|TC|1|99990;100000|99995;100009|1"          # as strings "100000" < "99990" and "100009" < "99995": exon 0 is 100000-100009
TD = "GD|TD|1|1000;1100|1099;1199|1"                # intron of length 0
TE = "GE|TE|1|1000|1099|+"
TX = "GX|TX|9|1000|1099|1"                          # chr9 is not in the genomic header
TM = "GM|TM|MT|100|199|1"
TRANSCRIPTS = (TA, TA2, TB, TC, TD, TE, TX, TM)

G_SQ = (("chr1", 300000), ("chr2", 5000), ("chrMT", 16569), ("chrM", 16569))


def g_header(sq=G_SQ, so="coordinate"):
    return "@HD\tVN:1.6\tSO:%s\n" % so + "".join("@SQ\tSN:%s\tLN:%d\n" % x for x in sq)


def t_header(names=TRANSCRIPTS, so="queryname"):
    return "@HD\tVN:1.6\tSO:%s\n" % so + "".join("@SQ\tSN:%s\tLN:400\n" % n for n in names)


S20 = "AAAAAAAAAACCCCCGGGTN"                         # reverse complement: NACCCGGGGGTTTTTTTTTT
S21 = "AACCCCCCCCCCCCCCCCCRT"                        # odd length, R keeps its value: ARGGGGGGGGGGGGGGGGGTT
S120 = "A" * 100 + "C" * 19 + "N"                    # N + 19 G + 100 T


def qual(n):
    return "".join(chr(40 + i % 50) for i in range(n))


def rd(name, flag, contig, pos, cigar, seq=S20, mapq=23, tags="NM:i:1\tXT:A:U\tZZ:Z:%s"):
    return "%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\t%s\n" % (name, flag, contig, pos, mapq, cigar, seq, qual(len(seq)), tags % name if "%s" in tags else tags)


GENOME_RECS = rd("g1", 0, "chr1", 500, "20M", mapq=37) + rd("g2", 16, "chr2", 40, "10M1D10M", mapq=25, tags="NM:i:300\tXA:Z:chr1,+5,20M,0;")

# name: (transcript SAM body, genomic @SQ, expected lifted records [(name, flag, contig or None, POS, CIGAR, SEQ)], expected stats that are not 0)
CASES = {
    # i = 0: 11 <= 100 -> start = 1000 + 11 - 1; end 29 <= 100 and start >= 1000: the record's own CIGAR
    "one_exon_fwd": (rd("r", 0, TA, 11, "5M1I14M"), G_SQ, [("r", 0, "chr1", 1010, "5M1I14M", S20)], dict(n_groups=1, n_lifted=1)),
    # i = 2 (7000-7099): end = 7099 - 11 + 1 = 7089 <= 7099: own CIGAR, start = 7089 - 20 (READ length, the span is 22) + 1
    "one_exon_rev": (rd("r", 0, TB, 11, "5M2D15M"), G_SQ, [("r", 16, "chr1", 7070, "5M2D15M", "NACCCGGGGGTTTTTTTTTT")],
                     dict(n_groups=1, n_lifted=1, n_strand_flipped=1)),
    "one_exon_rev_odd": (rd("r", 16, TB, 11, "21M", seq=S21), G_SQ, [("r", 0, "chr1", 7069, "21M", "ARGGGGGGGGGGGGGGGGGTT")],
                         dict(n_groups=1, n_lifted=1, n_strand_flipped=1)),
    # 91..210 of the transcript: 10 bases of exon 0 from 1090, intron 900, exon 1 whole, intron 900, 210 - 200 = 10 bases
    "two_junctions_fwd": (rd("r", 0, TA, 91, "120M", seq=S120), G_SQ, [("r", 0, "chr1", 1090, "10M900N100M900N10M", S120)],
                          dict(n_groups=1, n_lifted=1, n_spliced=1)),
    # downwards from exon 2: end = 7099 - 91 + 1 = 7009, 10M of 7000-7009, exon 1 whole, then 10 bases: start = 5099 - 10 + 1
    "two_junctions_rev": (rd("r", 0, TB, 91, "120M", seq=S120), G_SQ, [("r", 16, "chr1", 5090, "10M900N100M900N10M", "N" + "G" * 19 + "T" * 100)],
                          dict(n_groups=1, n_lifted=1, n_spliced=1, n_strand_flipped=1)),
    # start 1090 is set, end 109 > 100 and the CIGAR holds an I: the walk ends with nothing built, the record is still emitted
    "indel_junction_fwd": (rd("r", 0, TA, 91, "10M1I9M"), G_SQ, [("r", 0, "chr1", 1090, "*", S20)],
                           dict(n_groups=1, n_lifted=1, n_missed_indel_splice=1)),
    "indel_junction_rev": (rd("r", 0, TB, 91, "10M1D9M"), G_SQ, [], dict(n_groups=1, n_unlocated=1, n_missed_indel_splice=1)),
    # exon 0 is 100000-100009 after the string sort: POS 3 -> 100002 (numeric order would give 99992)
    "string_sort": (rd("r", 0, TC, 3, "5M"), G_SQ, [("r", 0, "chr1", 100002, "5M", S20)], dict(n_groups=1, n_lifted=1)),
    # POS 8, end 13 > 10: 100009 - 100007 + 1 = 3M, then the "intron" 99990 - 100009 - 1 < 0 ends the walk
    "string_sort_junction": (rd("r", 0, TC, 8, "6M"), G_SQ, [("r", 0, "chr1", 100007, "3M", S20)], dict(n_groups=1, n_lifted=1)),
    "intron_zero": (rd("r", 0, TD, 91, "20M"), G_SQ, [("r", 0, "chr1", 1090, "10M", S20)], dict(n_groups=1, n_lifted=1)),
    # 291..310 of a 300-base transcript: 10M of the last exon from 3090, then the walk runs out
    "past_last_exon_fwd": (rd("r", 0, TA, 291, "20M"), G_SQ, [("r", 0, "chr1", 3090, "10M", S20)], dict(n_groups=1, n_lifted=1)),
    # on -1 the start is only set where the alignment ends: never here
    "past_last_exon_rev": (rd("r", 0, TB, 291, "20M"), G_SQ, [], dict(n_groups=1, n_unlocated=1)),
    "strand_plus": (rd("r", 0, TE, 11, "20M"), G_SQ, [], dict(n_groups=1, n_unlocated=1)),
    # getAlignmentEnd = 0 with flag 4: 0 <= 100 ends the walk in exon 0 -- located at 1090 with its own 20M, not 10M900N10M
    "bridging_inside": (rd("r", 4, TA, 91, "20M"), G_SQ, [("r", 4, "chr1", 1090, "20M", S20)], dict(n_groups=1, n_lifted=1)),
    "bridging_outside": (rd("r", 4, TA, 150, "20M"), G_SQ, [], dict(n_groups=1, n_unlocated=1)),
    # -1: end stays -1 <= 7099, own CIGAR, start = -1 - 20 + 1 = -20: below base 1, not located (deviation 2)
    "bridging_outside_rev": (rd("r", 20, TB, 150, "20M"), G_SQ, [], dict(n_groups=1, n_unlocated=1)),
    "duplicates_equal": (rd("r", 0, TA, 11, "20M") + rd("r", 256, TA2, 11, "20M", tags="NM:i:0"), G_SQ,
                         [("r", 0, "chr1", 1010, "20M", S20)], dict(n_groups=1, n_lifted=1)),
    "duplicates_unequal": (rd("r", 0, TA, 11, "20M") + rd("r", 256, TA, 21, "20M") + rd("s", 0, TA, 31, "20M"), G_SQ,
                           [("s", 0, "chr1", 1030, "20M", S20)], dict(n_groups=2, n_groups_ambiguous=1, n_lifted=1)),
    # the second record has no 0x100: primaryIndex = 1, its own CIGAR and tags go out
    "secondary_first": (rd("r", 256, TA, 11, "20M") + rd("r", 0, TA2, 11, "8M2I10M", tags="NM:i:7"), G_SQ,
                        [("r", 0, "chr1", 1010, "8M2I10M", S20)], dict(n_groups=1, n_lifted=1)),
    # the unlocated primary stores nothing; of the two located secondaries entry 0 goes out
    "secondary_only": (rd("r", 0, TE, 11, "20M") + rd("r", 256, TA, 11, "20M", tags="NM:i:3") + rd("r", 256, TA2, 11, "20M", tags="NM:i:4"), G_SQ,
                       [("r", 256, "chr1", 1010, "20M", S20)], dict(n_groups=1, n_unlocated=1, n_lifted=1)),
    # a record without reference neither breaks nor starts a group: q's two hits still disagree
    "unplaced_inside_group": (rd("q", 0, TA, 11, "20M") + rd("q", 4, "*", 0, "*") + rd("q", 256, TA, 12, "20M"), G_SQ, [],
                              dict(n_groups=1, n_unplaced=1, n_groups_ambiguous=1)),
    "no_contig": (rd("r", 0, TX, 11, "20M") + rd("s", 0, TA, 11, "20M"), G_SQ, [("s", 0, "chr1", 1010, "20M", S20)],
                  dict(n_groups=2, n_no_contig=1, n_lifted=1)),
    "mt_with_chrM": (rd("r", 0, TM, 11, "20M"), G_SQ, [("r", 0, "chrM", 110, "20M", S20)], dict(n_groups=1, n_lifted=1)),
    "mt_without_chrM": (rd("r", 0, TM, 11, "20M"), G_SQ[:3], [("r", 0, None, 110, "20M", S20)], dict(n_groups=1, n_lifted=1, n_mt_unplaced=1)),
    # "chrMT" is looked up first: a header with chrM alone has no place for MT
    "mt_without_chrMT": (rd("r", 0, TM, 11, "20M"), G_SQ[:2] + G_SQ[3:], [], dict(n_groups=1, n_no_contig=1)),
}

ERRORS = {     # name: (transcript header, transcript SAM body)
    "five_fields": (t_header(("GZ|TZ|1|1000|1099",)), rd("r", 0, "GZ|TZ|1|1000|1099", 11, "20M")),
    "trailing_empty_field": (t_header(("GZ|TZ|1|1000|1099|",)), rd("r", 0, "GZ|TZ|1|1000|1099|", 11, "20M")),
    "not_a_number": (t_header(("GZ|TZ|1|1000;2k|1099;2099|1",)), rd("r", 0, "GZ|TZ|1|1000;2k|1099;2099|1", 11, "20M")),
    "counts_differ": (t_header(("GZ|TZ|1|1000;2000|1099|1",)), rd("r", 0, "GZ|TZ|1|1000;2000|1099|1", 11, "20M")),
    "not_name_sorted": (t_header(so="coordinate"), rd("r", 0, TA, 11, "20M")),
}


def run(name, sort=False):
    body, sq, _, _ = CASES[name]
    return J.combine(J.parse_sam(g_header(sq) + GENOME_RECS), J.parse_sam(t_header() + body), sort)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_worked(name):
    body, sq, lifted, stats = CASES[name]
    text, refs, recs, st = run(name)
    genome = J.parse_sam(g_header(sq) + GENOME_RECS)
    assert text == g_header(sq) and refs == list(sq)
    assert J.same_records(recs[:2], genome[2]) is None                # the genomic records first, untouched
    names = [n for n, _ in sq]
    got = [(r["name"], r["flag"], names[r["ref"]] if r["ref"] >= 0 else None, r["pos"] + 1, r["cigar"], r["seq"]) for r in recs[2:]]
    assert got == lifted
    for r in recs[2:]:
        assert r["mapq"] == 10 and r["qual"] == qual(len(r["seq"])) and (r["nref"], r["npos"], r["tlen"]) == (-1, -1, 0)
        span = J.ref_length(r["cigar"]) or 1
        assert r["bin"] == J.reg2bin(r["pos"], r["pos"] + span)
    exp = dict.fromkeys(J.STAT_KEYS, 0)
    exp.update(n_genome=2, n_transcript=body.count("\n"), **stats)
    assert st == exp


def test_emitted_record_keeps_its_own_tags():
    assert run("secondary_first")[2][2]["tags"] == ["NM:i:7"]
    assert run("secondary_only")[2][2]["tags"] == ["NM:i:3"]
    assert run("duplicates_equal")[2][2]["tags"] == ["NM:i:1", "XT:A:U", "ZZ:Z:r"]


def test_sorted_form():
    text, _, recs, _ = run("two_junctions_rev", sort=True)
    assert text.startswith("@HD\tVN:1.6\tSO:coordinate\n")
    assert [(r["name"], r["ref"], r["pos"]) for r in recs] == [("g1", 0, 499), ("r", 0, 5089), ("g2", 1, 39)]
    _, _, recs, _ = run("mt_without_chrM", sort=True)
    assert [r["name"] for r in recs] == ["g1", "g2", "r"] and recs[2]["ref"] == -1


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_errors(name):
    head, body = ERRORS[name]
    with pytest.raises(J.CombineError):
        J.combine(J.parse_sam(g_header() + GENOME_RECS), J.parse_sam(head + body))


def test_java_split():
    assert J.java_split("a|b||", "|") == ["a", "b"] and J.java_split("", ";") == [""] and J.java_split("|a", "|") == ["", "a"]
    assert J.exon_table(TC)[1:] == ([100000, 99990], [100009, 99995])


# ---- ps_extract_weak_reads (host code)

def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def test_extract_weak_reads(tmp_path):
    """a mapping made by the oracle on the three-contig genome: the FASTQ holds exactly the weak reads as they were sequenced,
    in BAM order; the kept BAM is what ps_bam_view keeps at that threshold"""
    import capi
    import orc
    import simulate as S
    from test_bam import read_bam
    rng = np.random.default_rng(11)
    g = [("c%d" % i, S.make_contig(n, rng, [])) for i, n in enumerate((30000, 20000, 12000))]
    g[2][1][1000:9000] = g[0][1][4000:12000]                                  # a second copy: MAPQ 0
    fa, fq, sam = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "r.sam")
    S.write_fasta(fa, g)
    S.write_fastq(fq, S.simulate_reads(g, n_reads=3000, read_len=50, min_len=25, seed=4, indel_scale=60, n_frac=0.002))
    orc.Index.from_fasta(fa).map_fastq(orc.stock_opt("0.04"), fq, sam, n_threads=4)
    bam, kept, weak, view = str(tmp_path / "r.bam"), str(tmp_path / "kept.bam"), str(tmp_path / "weak.fq"), str(tmp_path / "view.bam")
    capi.ps_sam_to_bam(sam, bam, threads=4)
    lines = open(fq).read().split("\n")
    reads = {lines[i][1:].split()[0]: lines[i:i + 4] for i in range(0, len(lines) - 1, 4)}
    for src in (bam, sam):
        st = capi.ps_extract_weak_reads(src, kept, weak, 10, threads=4)
        _, _, recs, _ = read_bam(bam)
        weak_recs = [r for r in recs if r["mapq"] < 10]
        assert 100 < len(weak_recs) < len(recs) - 100 and any(r["flag"] & 16 for r in weak_recs)
        exp = "".join("@%s\n%s\n+\n%s\n" % (r["name"], reads[r["name"]][1], reads[r["name"]][3]) for r in weak_recs)
        assert open(weak).read() == exp
        # and the same from the records alone
        assert exp == "".join("@%s\n%s\n+\n%s\n" % (r["name"], _revcomp(r["seq"]) if r["flag"] & 16 else r["seq"],
                                                     r["qual"][::-1] if r["flag"] & 16 else r["qual"]) for r in weak_recs)
        capi.ps_bam_view(bam, view, 10, threads=4)
        a, b = read_bam(kept), read_bam(view)
        assert a[0] == b[0] and a[1] == b[1] and J.same_records(a[2], b[2]) is None and len(a[2]) == len(recs) - len(weak_recs)
        assert st == dict(n_records=len(recs), n_weak=len(weak_recs), n_kept=len(a[2]), bam_bytes=os.path.getsize(kept))


def test_extract_weak_reads_errors(tmp_path):
    import capi
    sam = tmp_path / "m.sam"
    sam.write_text(g_header() + rd("ok", 0, "chr1", 10, "20M", mapq=30) + "bad\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n")
    with pytest.raises(capi.PsError, match="bad"):
        capi.ps_extract_weak_reads(str(sam), str(tmp_path / "k.bam"), str(tmp_path / "w.fq"), 10)
    sam.write_text(g_header() + "noq\t0\tchr1\t5\t3\t4M\t*\t0\t0\tACGT\t*\n")
    with pytest.raises(capi.PsError, match="noq"):
        capi.ps_extract_weak_reads(str(sam), str(tmp_path / "k.bam"), str(tmp_path / "w.fq"), 10)
    with pytest.raises(capi.PsError, match="may not be the input"):
        capi.ps_extract_weak_reads(str(sam), str(sam), str(tmp_path / "w.fq"), 10)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.sam"]
    # at threshold 0 nothing is weak: a record without SEQ passes through
    st = capi.ps_extract_weak_reads(str(sam), str(tmp_path / "k.bam"), str(tmp_path / "w.fq"), 0)
    assert st["n_weak"] == 0 and st["n_kept"] == 1 and open(str(tmp_path / "w.fq")).read() == ""


def test_mirrors_keep_the_error_contract(tmp_path):
    import __graft_entry__ as ge
    mod = ge.load_package()
    with pytest.raises(mod.mapping.ExternalCallErrorException, match="ExtractWeakMappingReads"):
        mod.mapping.ExtractWeakMappingReads().extractReads(str(tmp_path / "none.bam"), str(tmp_path / "a.bam"), str(tmp_path / "a.fq"), 10)
    with pytest.raises(mod.mapping.ExternalCallErrorException, match="CombineGenomeTranscript"):
        mod.mapping.CombineGenomeTranscript().combine(str(tmp_path / "none.bam"), str(tmp_path / "none2.bam"), str(tmp_path / "c.bam"))


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_combine_fails_loudly_without_device(tmp_path):
    import capi
    g, t = tmp_path / "g.sam", tmp_path / "t.sam"
    g.write_text(g_header() + GENOME_RECS)
    t.write_text(t_header() + CASES["one_exon_fwd"][0])
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_combine_genome_transcript(str(g), str(t), str(tmp_path / "c.bam"))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["g.sam", "t.sam"]
