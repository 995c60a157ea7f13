"""The six files of ErrorProfiling.inferErrorProfile (ErrorProfiling.java:100-631) as tests/java_errorprofile.py restates
them, against answers worked out by hand on hand-built SAM records over a tiny FASTA.  The GPU entry point
ps_error_profile_full is held to the same bytes in tests/test_gpu_error_profile_full.py."""
import math
import random

import orc
import java_errorprofile as J

FA = ">c1 some text\nACGTACGTACGTACGTACGTNNNNACGTACGTAAAACCCCGGGGTTTT\n>c2\nTTTTTTTTTTGGGGGGGGGG\n"
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:48\n@SQ\tSN:c2\tLN:20\n"
ML = 8

# QUAL characters: '+' 10, '5' 20, '?' 30, 'I' 40, 'A' 32, 'B' 33, 'C' 34, 'D' 35
RECORDS = [
    ("r1", 0, "c1", 1, "4M", "ACGA", "ABCD"),            # T->A at position 3
    ("r2", 16, "c2", 1, "4M", "TTCT", "+5?I"),            # reverse: read AGAA vs AAAA; the A->G at column 1 takes QUAL[1] = 20, not QUAL[2]
    ("r3", 0, "c1", 1, "2M1I2M", "ACTGT", "IIIII"),       # insertion: rebuilt over 5 columns, gap booked at 4; no .qualityPerMismatch
    ("r4", 0, "c1", 25, "2M1D2M", "ACTA", "5555"),        # deletion: width 5, qualities only at i < 4 (the Java fails at QUAL[4])
    ("r5", 0, "c1", 5, "4M", "ACGT", "*"),                # QUAL '*': counted, no quality booked
    ("r6", 0, "c1", 19, "4M", "GTAC", "????"),            # reference GTNN: two columns in the hole, qualities still booked at all four
    ("r7", 4, "*", 0, "*", "ACGT", "IIII"),               # unmapped
    ("r8", 1024, "c1", 1, "4M", "TTTT", "IIII"),          # duplicate
    ("r9", 0, "c1", 0, "4M", "TTTT", "IIII"),             # no position
    ("r10", 16, "c1", 1, "4M2N", "ACGT", "+5?I"),         # reverse N record: width 6, pairs at 5..2; 5 and 4 lie past QUAL
]


def sam_text(records, header=HEADER):
    return header + "".join("%s\t%d\t%s\t%d\t37\t%s\t*\t0\t0\t%s\t%s\n" % r for r in records)


def _sd(vals):
    m = sum(vals) / len(vals)
    s = 0.0
    for v in vals:
        s += (v - m) * (v - m)
    return m, math.sqrt(s / len(vals))


def _files(infer_q=True):
    ref = {"c1": b"ACGTACGTACGTACGTACGTNNNNACGTACGTAAAACCCCGGGGTTTT", "c2": b"TTTTTTTTTTGGGGGGGGGG"}
    return J.infer(sam_text(RECORDS), ref, ML, infer_q)


def test_fasta_reader(tmp_path):
    p = tmp_path / "r.fa"
    p.write_text(FA)
    assert J.read_fasta(str(p)) == {"c1": b"ACGTACGTACGTACGTACGTNNNNACGTACGTAAAACCCCGGGGTTTT", "c2": b"TTTTTTTTTTGGGGGGGGGG"}


def test_stats():
    _, st = _files()
    assert st == dict(n_records=10, n_counted=7, n_unmapped=1, n_duplicate=1, n_start_zero=1, n_indel_reads=3, n_skipped=0,
                      n_without_qual=1, n_qual_beyond_read=2)


def test_errorprofile_and_vcf_blocks():
    f, _ = _files()
    # A: 9 A->A, 1 A->G; C: 5; G: 5; T: 1 T->A, 5 T->T (the hole and the inserted / deleted columns count nothing)
    assert f[".errorprofile"] == ("0.9\t0.0\t0.1\t0.0\t\n0.0\t1.0\t0.0\t0.0\t\n0.0\t0.0\t1.0\t0.0\t\n%s\t0.0\t0.0\t%s\t\n"
                                  % (orc.java_double(1 / 6), orc.java_double(5 / 6))).encode()
    assert f[".errorprofile.vcf"] == ("A\tA\t9.0\nA\tC\t0.0\nA\tG\t1.0\nA\tT\t0.0\n\n"
                                      "C\tA\t0.0\nC\tC\t5.0\nC\tG\t0.0\nC\tT\t0.0\n\n"
                                      "G\tA\t0.0\nG\tC\t0.0\nG\tG\t5.0\nG\tT\t0.0\n\n"
                                      "T\tA\t1.0\nT\tC\t0.0\nT\tG\t0.0\nT\tT\t5.0\n\n").encode()


def test_quality_per_mismatch_unreversed():
    f, _ = _files()
    # pairs of r1 (32..35), r2 (10, 20, 30, 40 at columns 0..3 of the reverse read), r6 (30, 30), r10 (columns 2, 3: 30, 40);
    # r3 and r4 carry I / D, r5 has no QUAL.  A->A: 32 + 10 + 30 + 40 + 30 over 5; A->G: r2's QUAL[1] = 20
    assert f[".qualityPerMismatch"] == (b"28.4\tNaN\t20.0\tNaN\t\n"
                                        b"NaN\t36.5\tNaN\tNaN\t\n"
                                        b"NaN\tNaN\t32.0\tNaN\t\n"
                                        b"35.0\tNaN\tNaN\t30.0\t\n")


def test_indels_and_indelprofile():
    f, _ = _files()
    # bases per position 6 6 4 6 3 1 0 0; one insertion (r3) and one deletion (r4) at column 4
    third = orc.java_double(1 / 3)
    assert f[".indels"] == ("0.0\t0.0\n" * 4 + "%s\t%s\n" % (third, third) + "0.0\t0.0\n" * 3).encode()
    assert f[".indelprofile"] == ("%s\t%s" % (third, third)).encode()


def test_qualities_positions():
    f, _ = _files()
    cols = [[32, 10, 40, 20, 30, 10], [33, 20, 40, 20, 30, 20], [34, 30, 40, 20, 30, 30], [35, 40, 40, 20, 30, 40], [40]]
    exp = ""
    for c in cols:
        m, s = _sd(c)
        exp += orc.java_double(m) + "\t" + orc.java_double(s) + "\n"
    exp += "NaN\tNaN\n" * 3                                   # positions nobody reaches: 0.0 / 0 in the Java
    assert f[".qualities"] == exp.encode()
    assert f[".qualities"].split(b"\n")[0] == b"23.666666666666668\t" + orc.java_double(_sd(cols[0])[1]).encode()
    assert f[".qualities"].split(b"\n")[4] == b"40.0\t0.0"
    g, _ = _files(False)
    assert g[".qualities"] == b"" and all(g[k] == f[k] for k in J.FILES if k != ".qualities")


def order_records(seed, n=4000):
    """one set of 40 bp records over a random contig written in two orders (shared with the GPU test)"""
    rng = random.Random(seed)
    contig = "".join(rng.choice("ACGT") for _ in range(400))
    recs = []
    for r in range(n):
        pos = rng.randrange(1, 400 - 40)
        seq = contig[pos - 1:pos + 39]
        qual = "".join(chr(33 + rng.choice((2, 11, 25, 37, 41))) for _ in range(40))
        recs.append(("o%d" % r, 16 if r % 2 else 0, "s1", pos, "40M", seq, qual))
    shuffled = recs[:]
    rng.shuffle(shuffled)
    return contig, recs, shuffled


ORDER_SEED = 7


def test_order_matters_for_the_sd_only():
    contig, a, b = order_records(ORDER_SEED)
    hdr = "@SQ\tSN:s1\tLN:400\n"
    fa, _ = J.infer(sam_text(a, hdr), {"s1": contig.encode()}, 40, True)
    fb, _ = J.infer(sam_text(b, hdr), {"s1": contig.encode()}, 40, True)
    assert all(fa[k] == fb[k] for k in J.FILES if k != ".qualities")
    assert fa[".qualities"] != fb[".qualities"]                # the file-order sum shows in the last bits
    ma = [l.split(b"\t")[0] for l in fa[".qualities"].split(b"\n")]
    assert ma == [l.split(b"\t")[0] for l in fb[".qualities"].split(b"\n")]          # the means are exact
