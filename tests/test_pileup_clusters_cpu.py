"""PileupClusters.calculateReadPileups (PileupClusters.java:62-673) as tests/java_pileupclusters.py restates it, against
answers worked out by hand on hand-built SAM records over a small FASTA.  The GPU entry point ps_pileup_clusters is held to
the same bytes in tests/test_gpu_pileup_clusters.py, which imports the cases from here."""
import gzip
import math

import pytest

import java_pileupclusters as J
from test_capi_cpu import _no_gpu

L1, L2 = 400, 65600
T_SITES = (31, 33, 104, 116, 136, 160, 390) + tuple(range(50, 63))


def make_ref():
    """chr1: "ACG" repeats (no T) with T at T_SITES, N at 70..72, soft-masked 80..90 with a 't' at 85; c2: "ACG" repeats
    with T at 65537 and 65552"""
    c1 = bytearray((b"ACG" * 134)[:L1])
    for p in T_SITES:
        c1[p - 1] = ord("T")
    c1[69:72] = b"NNN"
    c1[79:90] = bytes(c1[79:90]).lower()
    c1[84] = ord("t")
    c2 = bytearray((b"ACG" * 21900)[:L2])
    c2[65536] = c2[65551] = ord("T")
    return {"chr1": bytes(c1), "c2": bytes(c2)}


REF = make_ref()
FA = "".join(">%s\n%s" % (n, "".join(s[i:i + 60].decode() + "\n" for i in range(0, len(s), 60))) for n, s in REF.items())
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n@SQ\tSN:c2\tLN:%d\n" % (L1, L2)


def rd(name, flag, chrom, pos, cigar, subs=None):
    """a SAM record whose SEQ copies the reference along the CIGAR (I and S bases: A), with subs {reference position: base}"""
    subs, seq, g = subs or {}, [], pos
    for op, n in J.cigar_ops(cigar):
        if op in "M=X":
            for k in range(n):
                seq.append(subs.get(g + k, chr(REF[chrom][g + k - 1]).upper()))
            g += n
        elif op in "IS":
            seq.append("A" * n)
        elif op in "DN":
            g += n
    s = "".join(seq)
    return "%s\t%d\t%s\t%d\t37\t%s\t*\t0\t0\t%s\t%s\n" % (name, flag, chrom, pos, cigar, s, "I" * len(s))


def sam(*recs, header=HEADER):
    return header + "".join(recs)


def ref_at(a, b, chrom="chr1"):
    return REF[chrom][a - 1:b].decode()


def revcomp(s):
    return J._revcomp(s.encode()).decode()


C = {31: "C", 33: "C"}
CASES = {      # name: (SAM text, VCF bytes or None, MIN_COVERAGE)
    "basic": (sam(rd("a", 0, "chr1", 30, "10M"), rd("b", 0, "chr1", 32, "10M"), rd("c", 0, "chr1", 60, "10M"),
                  rd("d", 0, "chr1", 80, "10M")), None, 1),
    "tie_31_33": (sam(rd("a", 0, "chr1", 25, "10M", C), rd("z", 0, "chr1", 100, "10M")), None, 1),
    "tie_65537": (sam(rd("a", 0, "c2", 65530, "30M", {65537: "C", 65552: "C"}), rd("z", 0, "c2", 65580, "10M")), None, 1),
    "cap16": (sam(rd("b", 0, "chr1", 110, "30M", {116: "C", 136: "C"}), rd("z", 0, "chr1", 300, "10M")), None, 1),
    "cap32": (sam(rd("a", 0, "chr1", 45, "20M", {p: "C" for p in range(50, 63)}), rd("b", 0, "chr1", 110, "30M", {116: "C", 136: "C"}),
                  rd("z", 0, "chr1", 300, "10M")), None, 1),
    "sitefreq": (sam(rd("a", 0, "chr1", 25, "10M", C), rd("b", 0, "chr1", 25, "10M", {31: "C"}), rd("c", 0, "chr1", 100, "10M", {104: "C"}),
                     rd("d", 0, "chr1", 100, "10M"), rd("z", 0, "chr1", 200, "10M")), None, 1),
    "snp": (sam(rd("a", 0, "chr1", 25, "10M", C), rd("b", 0, "chr1", 25, "10M", {31: "C"}), rd("c", 0, "chr1", 100, "10M", {104: "C"}),
                rd("d", 0, "chr1", 100, "10M"), rd("z", 0, "chr1", 200, "10M")),
            b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n1\t31\t.\tT\tC\n1\t33\t.\tT\tA,C\n1\t104\t.\tTT\tCT\nchr1\t31\t.\tT\tC\n", 1),
    "strand": (sam(rd("a", 0, "chr1", 25, "10M"), rd("b", 16, "chr1", 27, "10M"), rd("c", 16, "chr1", 28, "10M"), rd("d", 16, "chr1", 100, "10M"),
                   rd("e", 0, "chr1", 101, "10M"), rd("f", 0, "chr1", 200, "10M"), rd("z", 0, "chr1", 300, "10M")), None, 1),
    "deletion": (sam(rd("a", 0, "chr1", 25, "5M2D5M", {33: "C"}), rd("s", 0, "chr1", 26, "5M1D2N5M"), rd("z", 0, "chr1", 200, "10M")), None, 1),
    "assembly": (sam(rd("a", 0, "chr1", 25, "10M"), rd("b", 0, "chr1", 29, "10S9M"), rd("c", 0, "chr1", 64, "12M"), rd("d", 16, "chr1", 80, "10M", {82: "G"}),
                     rd("z", 0, "chr1", 200, "10M")), None, 1),
    "ccr_past_end": (sam(rd("a", 0, "chr1", 385, "10M", {390: "C"}), rd("z", 0, "c2", 100, "10M")), None, 1),
    "span3": (sam(rd("a", 0, "chr1", 100, "10M"), rd("b", 0, "chr1", 106, "3M"), rd("c", 0, "chr1", 107, "10M"), rd("z", 0, "chr1", 200, "10M")), None, 1),
    "index60": (sam(rd("a", 0, "chr1", 100, "70M", {160: "C"}), rd("z", 0, "chr1", 300, "10M")), None, 1),
}


def run(name, min_cov=None):
    text, vcf, mc = CASES[name]
    return J.cluster(text, REF, vcf, mc if min_cov is None else min_cov)


def lines(b):
    return b.decode().split("\n")[:-1]


def test_fasta_round_trip(tmp_path):
    p = tmp_path / "r.fa"
    p.write_text(FA)
    assert J.read_fasta(str(p)) == REF


def test_last_cluster_unwritten_ids_and_pseudo_line():
    f, st, _ = run("basic")
    out = lines(f[""])
    assert out[0] == J.HEADER.rstrip("\n")
    # cl_2 = a + b: b ends at 41 > 39, so the overhang 40..41 of its 10M is appended; cl_3 = c; cl_4 = d is never written
    assert out[1:] == ["cl_2_chr1\tchr1\t30\t41\t+\t2\t0\t0\t0.0\t%s\t+\t12" % ref_at(30, 41),
                       "cl_3_chr1\tchr1\t60\t69\t+\t1\t0\t0\t0.0\t%s\t+\t10" % ref_at(60, 69)]
    assert st["n_clusters"] == 3 and st["n_clusters_written"] == 2 and st["n_kept"] == 4
    f0, st0, _ = run("basic", 0)
    assert lines(f0[""])[1] == "\t\t0\t0\t+\t0\t0\t0\t0.0\t\t+\t0" and lines(f0[""])[2:] == out[1:]
    assert st0["n_clusters_written"] == 3
    f2, _, _ = run("basic", 2)
    assert lines(f2[""])[1:] == out[1:2]
    assert f[".ccr.fasta"] == b"" and lines(f[".ccr.tsv"]) == [J.CCR_HEADER.rstrip("\n")]
    assert f[".sitefrequency.tsv"] == b"" and lines(f[".sitepositions.tsv"]) == ["NaN"] * 51
    assert lines(f[".report"]) == ["Double stranded clusters found: 0", "Loci found that are SNPs: 0", "0 insertion or deletion skipped",
                                   "T-C mutations identified as SNPs: 0", "T-C mutations identified as SNVs (100% T-C in 1 site): 0"]


def test_tie_31_33():
    # 31 and 33 both 1/1; cap 16: 33 sits in bucket 1, 31 in bucket 15, so 31 comes last and `>=` keeps it, while "largest"
    # and "last inserted" (31 at read index 6, then 33 at 8) both give 33
    f, st, info = run("tie_31_33")
    assert lines(f[".ccr.fasta"]) == [">cl_2_chr1 20-anchor-20 chr1:+:11-51", ref_at(11, 51).upper()]
    assert lines(f[".ccr.tsv"])[1] == "Gene\tcl_2_chr1\t+\tchr1\t25\t34\t11\t51\t%s\t31\t1\t2\t1\t1.0\t2\t2.0" % ref_at(11, 51).upper()
    assert info["ties_hashmap"] == 1 and st["n_snv_sites"] == 2 and st["n_crosslinked"] == 1


def test_tie_hash_spread():
    # 65537 = 0x10001 -> (h ^ h >>> 16) & 15 = 0; 65552 = 0x10010 -> 1: the spread puts 65537 first, so 65552 wins;
    # the unspread bucket (p & 15) would give 1 and 0 and pick 65537
    assert (J.bucket(65537, 16), J.bucket(65552, 16)) == (0, 1) and (65537 & 15, 65552 & 15) == (1, 0)
    f, _, _ = run("tie_65537")
    assert lines(f[".ccr.fasta"])[0] == ">cl_2_c2 20-anchor-20 c2:+:65532-65572"
    assert lines(f[".ccr.tsv"])[1].split("\t")[9] == "65552"


def test_cap_grows_with_an_earlier_cluster():
    # 116 and 136 tie; cap 16: buckets 4 and 8 -> 136; after a 13-site cluster the table has 32 buckets: 20 and 8 -> 116
    assert (J.bucket(116, 16), J.bucket(136, 16), J.bucket(116, 32), J.bucket(136, 32)) == (4, 8, 20, 8)
    f16, _, i16 = run("cap16")
    f32, st, i32 = run("cap32")
    assert lines(f16[".ccr.tsv"])[1].split("\t")[9] == "136"
    assert lines(f32[".ccr.tsv"])[2].split("\t")[9] == "116"
    assert (i16["max_cap"], i32["max_cap"]) == (16, 32)
    assert lines(f32[""])[1].split("\t")[6:8] == ["13", "13"]


def test_sitefrequency_doubles_the_first_cluster():
    # cluster 1: 31 -> 2/2, 33 -> 1/2, sorted [1.0, 0.5]; cluster 2: 104 -> 1/2, sorted [0.5]; two crosslinked clusters
    # rank 0: (1.0 + 0.5) / 2; rank 1: (0.5 + 0.5) / 2 -- the Java adds the first cluster's rank 1 to itself
    f, st, _ = run("sitefreq")
    assert lines(f[".sitefrequency.tsv"]) == ["0.75", "0.5"]
    # read-index flags: cluster 1 at 6 and 8, cluster 2 at 4; three flags in all
    exp = ["0.0"] * 51
    for j in (4, 6, 8):
        exp[j] = "0.3333333333333333"
    assert lines(f[".sitepositions.tsv"]) == exp
    out = lines(f[""])
    assert out[1] == "cl_2_chr1\tchr1\t25\t34\t+\t2\t3\t2\t1.5\t%s\t+\t10" % ref_at(25, 34)
    assert out[2] == "cl_3_chr1\tchr1\t100\t109\t+\t2\t1\t1\t0.5\t%s\t+\t10" % ref_at(100, 109)
    assert st["n_crosslinked"] == 2 and st["n_ccr"] == 2


def test_snp_removal():
    # "1 31 T C" matches chr1:31 after "chr" is stripped; "1 33 T A,C" does not (first ALT A); "1 104 TT CT" does;
    # "chr1 31" names no stripped contig.  #T2C sites counts before removal; SNVs are sites of count 1, removed or not
    f, st, _ = run("snp")
    out = lines(f[""])
    assert out[1] == "cl_2_chr1\tchr1\t25\t34\t+\t2\t3\t2\t0.5\t%s\t+\t10" % ref_at(25, 34)
    assert out[2] == "cl_3_chr1\tchr1\t100\t109\t+\t2\t1\t1\t0.0\t%s\t+\t10" % ref_at(100, 109)
    assert [l.split("\t")[9] for l in lines(f[".ccr.tsv"])[1:]] == ["33"]
    assert (st["n_snp_hits"], st["n_snv_sites"], st["n_crosslinked"]) == (2, 2, 1)
    assert lines(f[".report"])[3:] == ["T-C mutations identified as SNPs: 2", "T-C mutations identified as SNVs (100% T-C in 1 site): 2"]
    assert J.read_vcf(gzip.compress(CASES["snp"][1])) == J.read_vcf(CASES["snp"][1]) == {("1", 31), ("1", 104), ("chr1", 31)}


def test_strands():
    f, st, _ = run("strand")
    out = [l.split("\t") for l in lines(f[""])[1:]]
    # forward first + two reverse members: "+", "+/-", two double-stranded counts; reverse first: "-", "-", sequence
    # reverse-complemented (100..109 and the overhang 110 of the forward member); forward only: "+", "+"
    assert [(o[4], o[10]) for o in out] == [("+", "+/-"), ("-", "-"), ("+", "+")]
    assert out[1][9] == revcomp(ref_at(100, 110))
    assert st["n_double_stranded"] == 2 and lines(f[".report"])[0] == "Double stranded clusters found: 2"


def test_deletion_shifts_positions_and_indel_n_is_skipped():
    # 5M2D5M at 25: the read base over reference 33 is concatenation index 6, booked at 25 + 6 = 31
    f, st, _ = run("deletion")
    tsv = lines(f[".ccr.tsv"])[1].split("\t")
    assert tsv[9] == "31" and tsv[11] == "1"
    assert st["n_skipped_indel"] == 1 and lines(f[".report"])[2] == "1 insertion or deletion skipped"
    assert lines(f[""])[1].split("\t")[2:4] == ["25", "36"]


def test_sequence_assembly():
    f, _, _ = run("assembly")
    out = [l.split("\t") for l in lines(f[""])[1:]]
    # b = 10S9M at 29 (end 37 > 34): the 10S reaches the end, so it moves the end to 37, and the 9M, shifted to 39, starts
    # beyond it: prepended
    assert out[0][9] == ref_at(39, 47) + ref_at(25, 34) and out[0][11] == "19"
    assert out[1][9] == ref_at(64, 75) and "NNN" in out[1][9]
    # reverse read over the soft-masked 80..89 with a T->C at 'a' 82 (read G): lower case kept in the cluster sequence, the
    # CCR (strand "-") reverse-complemented and upper-cased, its N kept
    assert out[2][9] == revcomp(ref_at(80, 89)) and out[2][9] != out[2][9].upper()
    fa = lines(f[".ccr.fasta"])
    assert fa == [">cl_4_chr1 20-anchor-20 chr1:-:62-102", revcomp(ref_at(62, 102)).upper()] and "NNN" in fa[1]


def test_ccr_past_contig_end():
    f, st, _ = run("ccr_past_end")
    assert lines(f[".ccr.fasta"]) == [">cl_2_chr1 20-anchor-20 chr1:+:370-410", ""]
    assert lines(f[".ccr.tsv"])[1].split("\t")[8] == "" and st["n_ccr_past_end"] == 1


def test_span3_after_boundary():
    # a (100..109); b = 3M at 106: 109 - 106 < 5 opens a cluster that ends at 108, below the running maximum 109;
    # c at 107: 108 - 107 < 5 opens again
    f, _, _ = run("span3")
    assert [l.split("\t")[:4] for l in lines(f[""])[1:]] == [["cl_2_chr1", "chr1", "100", "109"], ["cl_3_chr1", "chr1", "106", "108"],
                                                           ["cl_4_chr1", "chr1", "107", "116"]]


def test_t2c_beyond_read_index_51():
    f, st, _ = run("index60")
    assert st["n_t2c_beyond_51"] == 1 and st["n_crosslinked"] == 1
    assert lines(f[""])[1].split("\t")[6:9] == ["1", "1", "1.0"]
    assert lines(f[".sitepositions.tsv"]) == ["NaN"] * 51


def test_fixture_conditions_raise():
    with pytest.raises(J.FixtureError):       # CCR window before base 1
        J.cluster(sam(rd("a", 0, "chr1", 1, "10M", {4: "C"}), rd("z", 0, "chr1", 100, "10M")), {**REF, "chr1": b"ACGT" + REF["chr1"][4:]}, None, 1)
    m = J.JMap()
    for k in range(8):
        m.put_count(16 * 2 ** 20 * k + 5)     # 8 keys in bucket 5 of 16 (the spread only touches bits 8 and up)
    with pytest.raises(J.FixtureError):
        m.put_count(16 * 2 ** 20 * 9 + 5)


def test_unsorted_raises():
    with pytest.raises(ValueError, match="SO:unsorted"):
        J.cluster(CASES["basic"][0].replace("SO:coordinate", "SO:unsorted"), REF, None, 1)


def test_nan_and_division():
    # the .sitepositions output is int / int in double: NaN for 0 / 0
    assert J.jd(float("nan")) == "NaN" and J.jd(1 / 3) == "0.3333333333333333" and math.isnan(float("nan"))


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_library_fails_loudly_without_device(tmp_path):
    import capi
    fa, sam = tmp_path / "r.fa", tmp_path / "m.sam"
    fa.write_text(FA)
    sam.write_text(CASES["basic"][0])
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_pileup_clusters(str(sam), str(fa), str(tmp_path / "out"), None, 1)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.sam", "r.fa"]
