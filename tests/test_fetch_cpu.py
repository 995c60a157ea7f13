"""FetchSequencesForBindingSites / FetchSequencesForBEDFile.fetchSequences (the `fetch` and `fetchBed` modes) as
tests/java_fetch.py restates them, against answers worked out by hand on one small genome.  The GPU entry point
ps_fetch_sequences is held to the same bytes and counters in tests/test_gpu_fetch.py, which imports the cases from here."""
import os
import re

import pytest

import java_fetch as J
from test_capi_cpu import ROOT, _no_gpu

# c1, 20 bases:  A C G T N N N N a c  g  t  R  A  C  G  T  T  G  C      (holes: N at 5-8, R at 13; soft-masked 9-12)
#                1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20
# 7:  AAAACCCC          chr7:  GGGGTTTTAC   (both names exist: fetchBed turns "7" into "chr7")
GENOME = (b">c1 first contig\nACGTNNNNac\ngtRACGTTGC\n"
          b">7\nAAAACCCC\n"
          b">chr7\nGGGGTTTTAC\n")
# the header `clust` writes: field 11 is SeqLength, field 9 the Java's "Seqenece"
HEADER = b"ClusterID\tChr\tStart\tEnd\tStrand\t#reads\t#T2C\t#T2C sites\tT2C Fraction\tSeqenece\tCombStrand\tSeqLength"


def row(chrom, start, end, strand, last=b"6", tail=(), cid=b"cl1"):
    """a line of the cluster table: twelve fields, `last` in field 11 (the input's SeqLength, or the sequence that replaces it),
    and further fields behind it"""
    f = [cid, chrom, str(start).encode(), str(end).encode(), strand, b"7", b"3", b"2", b"0.42", b"ACGTAC", b"+-", last] + list(tail)
    return b"\t".join(f)


def table(*rows, end=b"\n", header=HEADER):
    return b"".join(r + end for r in (header,) + rows)


def counters(**kw):
    st = dict.fromkeys(J.INT_KEYS, 0)
    st.update(kw)
    return st


CASES = {}          # key -> (sites file, bed, expected output, expected counters)

# Holes, forward and reverse: c1 3-14 is G T N N N N a c g t R A.  Forward, upper-cased: GTNNNNACGTRA.  Reverse: the order
# reversed, A R t g c a N N N N T G, then A, C, G, T of either case swapped and R and N kept: T R a c g t N N N N A C.
# Five of the twelve bases come from holes, on either strand.
CASES["holes_both_strands"] = (table(row(b"c1", 3, 14, b"+"), row(b"c1", 3, 14, b"-")), False,
                               table(row(b"c1", 3, 14, b"+", b"GTNNNNACGTRA"), row(b"c1", 3, 14, b"-", b"TRACGTNNNNAC")),
                               counters(n_lines=3, n_sites=2, n_reverse=1, n_bases=24, n_hole_bases=10))

# A lone R: 13-13 is "R" on both strands; 12-14 is t R A -> TRA forward, reversed A R t -> complemented T R a -> TRA.
CASES["lone_r"] = (table(row(b"c1", 13, 13, b"+"), row(b"c1", 13, 13, b"-"), row(b"c1", 12, 14, b"+"), row(b"c1", 12, 14, b"-")), False,
                   table(row(b"c1", 13, 13, b"+", b"R"), row(b"c1", 13, 13, b"-", b"R"), row(b"c1", 12, 14, b"+", b"TRA"), row(b"c1", 12, 14, b"-", b"TRA")),
                   counters(n_lines=5, n_sites=4, n_reverse=2, n_bases=8, n_hole_bases=4))

# start == end + 1 is a legal empty sequence (no exception, nothing counted): field 11 becomes "", the line ends in a TAB
CASES["empty_but_legal"] = (table(row(b"c1", 5, 4, b"+"), row(b"c1", 1, 0, b"-"), row(b"c1", 21, 20, b"+")), False,
                            table(row(b"c1", 5, 4, b"+", b""), row(b"c1", 1, 0, b"-", b""), row(b"c1", 21, 20, b"+", b"")),
                            counters(n_lines=4, n_sites=3, n_reverse=1))

# The contig's end: 18-20 is T G C; 20-20 the last base; 18-21 is one past the end: empty
CASES["contig_end"] = (table(row(b"c1", 18, 20, b"+"), row(b"c1", 20, 20, b"-"), row(b"c1", 18, 21, b"+"), row(b"7", 1, 8, b"+"), row(b"7", 1, 9, b"-")), False,
                       table(row(b"c1", 18, 20, b"+", b"TGC"), row(b"c1", 20, 20, b"-", b"G"), row(b"c1", 18, 21, b"+", b""),
                             row(b"7", 1, 8, b"+", b"AAAACCCC"), row(b"7", 1, 9, b"-", b"")),
                       counters(n_lines=6, n_sites=5, n_reverse=2, n_bases=12, n_past_end=2))

# Before base 1: start 0 and -3 are empty by the library's rule; 0 to -1 is start == end + 1, legal for htsjdk, and still
# starts before base 1
CASES["before_start"] = (table(row(b"c1", 0, 3, b"+"), row(b"c1", -3, 2, b"-"), row(b"c1", 0, -1, b"+")), False,
                         table(row(b"c1", 0, 3, b"+", b""), row(b"c1", -3, 2, b"-", b""), row(b"c1", 0, -1, b"+", b"")),
                         counters(n_lines=4, n_sites=3, n_reverse=1, n_before_start=3))

# start > end + 1 is checked first: on an unknown contig, past the end and before the start it still counts as inverted;
# end 2147483647: end + 1 wraps to -2147483648 in a Java int, so any start is "after" it
CASES["inverted"] = (table(row(b"c1", 5, 3, b"+"), row(b"nowhere", 9, 2, b"-"), row(b"c1", 30, 25, b"+"), row(b"c1", 0, -2, b"+"), row(b"c1", 1, 2147483647, b"+")), False,
                     table(row(b"c1", 5, 3, b"+", b""), row(b"nowhere", 9, 2, b"-", b""), row(b"c1", 30, 25, b"+", b""), row(b"c1", 0, -2, b"+", b""),
                           row(b"c1", 1, 2147483647, b"+", b"")),
                     counters(n_lines=6, n_sites=5, n_reverse=1, n_inverted=5))

# An unknown contig, checked before the end and the start; `fetch` takes the name as it is: "chrc1" and "C1" are unknown
CASES["unknown_contig"] = (table(row(b"c9", 1, 3, b"+"), row(b"c9", 0, 99, b"-"), row(b"chrc1", 1, 3, b"+"), row(b"C1", 1, 3, b"+"), row(b"c1", 1, 3, b"+")), False,
                           table(row(b"c9", 1, 3, b"+", b""), row(b"c9", 0, 99, b"-", b""), row(b"chrc1", 1, 3, b"+", b""), row(b"C1", 1, 3, b"+", b""),
                                 row(b"c1", 1, 3, b"+", b"ACG")),
                           counters(n_lines=6, n_sites=5, n_reverse=1, n_bases=3, n_no_contig=4))

# 13 fields: the 13th stays behind the sequence.  A 13th EMPTY field is dropped by split and stays dropped: twelve fields out.
# An empty 13th before a 14th is kept.  An empty sequence in front of a kept tail leaves two TABs.
CASES["more_than_12_fields"] = (table(row(b"c1", 1, 4, b"+", tail=[b"x"]), row(b"c1", 1, 4, b"+", tail=[b""]), row(b"c1", 1, 4, b"+", tail=[b"", b"y"]),
                                      row(b"c1", 1, 4, b"+", tail=[b"", b""]), row(b"c1", 5, 4, b"+", tail=[b"x"])), False,
                                b"".join([HEADER + b"\n",
                                          b"cl1\tc1\t1\t4\t+\t7\t3\t2\t0.42\tACGTAC\t+-\tACGT\tx\n",
                                          b"cl1\tc1\t1\t4\t+\t7\t3\t2\t0.42\tACGTAC\t+-\tACGT\n",
                                          b"cl1\tc1\t1\t4\t+\t7\t3\t2\t0.42\tACGTAC\t+-\tACGT\t\ty\n",
                                          b"cl1\tc1\t1\t4\t+\t7\t3\t2\t0.42\tACGTAC\t+-\tACGT\n",
                                          b"cl1\tc1\t5\t4\t+\t7\t3\t2\t0.42\tACGTAC\t+-\t\tx\n"]),
                                counters(n_lines=6, n_sites=5, n_bases=16))

# A real `clust` header and line: the sequence lands in SeqLength (field 11); "Seqenece" (field 9) keeps the cluster's own text.
# Empty fields in the middle are kept.  Strand: only exactly "-" is reverse ("--", "" and "+" are forward).
CASES["field_11_overwritten"] = (b"".join([HEADER + b"\n",
                                           b"cl_7\tchr7\t2\t6\t-\t12\t4\t2\t0.3333\tGGGTT\t-\t5\n",
                                           b"cl_8\tchr7\t2\t6\t--\t\t\t\t\t\t\t5\n",
                                           b"cl_9\tchr7\t2\t6\t\t1\t1\t1\t1\t1\t1\t1\n"]), False,
                                 b"".join([HEADER + b"\n",
                                           b"cl_7\tchr7\t2\t6\t-\t12\t4\t2\t0.3333\tGGGTT\t-\tAACCC\n",
                                           b"cl_8\tchr7\t2\t6\t--\t\t\t\t\t\t\tGGGTT\n",
                                           b"cl_9\tchr7\t2\t6\t\t1\t1\t1\t1\t1\t1\tGGGTT\n"]),
                                 counters(n_lines=4, n_sites=3, n_reverse=1, n_bases=15))

# Line ends "\r\n", "\r" and none after the last line; the output always ends its lines with "\n"
CASES["line_ends"] = (HEADER + b"\r\n" + row(b"c1", 1, 2, b"+") + b"\r" + row(b"c1", 3, 4, b"+") + b"\r\n" + row(b"c1", 1, 4, b"-"), False,
                      table(row(b"c1", 1, 2, b"+", b"AC"), row(b"c1", 3, 4, b"+", b"GT"), row(b"c1", 1, 4, b"-", b"ACGT")),
                      counters(n_lines=4, n_sites=3, n_reverse=1, n_bases=8))

# Soft-masked bases come out in upper case: 9-11 is a c g -> ACG; reversed g c a, complemented c g t -> CGT
CASES["lower_case"] = (table(row(b"c1", 9, 11, b"+"), row(b"c1", 9, 11, b"-"), row(b"c1", 8, 13, b"+")), False,
                       table(row(b"c1", 9, 11, b"+", b"ACG"), row(b"c1", 9, 11, b"-", b"CGT"), row(b"c1", 8, 13, b"+", b"NACGTR")),
                       counters(n_lines=4, n_sites=3, n_reverse=1, n_bases=12, n_hole_bases=2))

# Only a header: it is copied, nothing is fetched.  The header may be anything, an empty line too.
CASES["header_only"] = (HEADER + b"\n", False, HEADER + b"\n", counters(n_lines=1))
CASES["empty_header"] = (b"\n" + row(b"c1", 1, 3, b"+") + b"\n", False, b"\n" + row(b"c1", 1, 3, b"+", b"ACG") + b"\n",
                         counters(n_lines=2, n_sites=1, n_bases=3))

# ---- fetchBed.  Line 1 is copied as a header in this mode too: the first BED record is never fetched.
# "7" becomes "chr7" (GGGGTTTTAC), never the contig "7" (AAAACCCC); "chr7" stays; "c1" becomes "chrc1", which does not exist.
CASES["bed_chr_prefix"] = (b"chr7\t1\t4\tfirst\t+\n" + b"7\t1\t4\tplain\t0\n" + b"chr7\t5\t8\twith_chr\t0\n" + b"c1\t1\t4\tother\t0\n", True,
                           b"chr7\t1\t4\tfirst\t+\n" + b">plain\nGGGG\n" + b">with_chr\nTTTT\n" + b">other\n\n",
                           counters(n_lines=4, n_sites=3, n_bases=8, n_no_contig=1))

# The strand is read from field 4, BED's score column: "-" there reverses (7-10 is T T A C -> G T A A); a proper BED line
# with score 5 and strand "-" in field 5 is fetched forward
CASES["bed_strand_is_field_4"] = (b"track\n" + b"chr7\t7\t10\tscore_minus\t-\t+\n" + b"chr7\t7\t10\tproper_bed\t5\t-\n", True,
                                  b"track\n" + b">score_minus\nGTAA\n" + b">proper_bed\nTTAC\n",
                                  counters(n_lines=3, n_sites=2, n_reverse=1, n_bases=8))

# BED's 0-based half-open 4-8 means bases 5-8, TTTT; the Java hands 4 and 8 to getSubsequenceAt as 1-based inclusive: bases
# 4-8, GTTTT, one base longer and shifted.  A BED interval from 0 starts before base 1: empty.
CASES["bed_off_by_one"] = (b"#bed\n" + b"chr7\t4\t8\tshifted\t0\n" + b"chr7\t0\t4\tfrom_zero\t0\n" + b"chr7\t9\t10\tlast\t0\tmore\tfields\n", True,
                           b"#bed\n" + b">shifted\nGTTTT\n" + b">from_zero\n\n" + b">last\nAC\n",
                           counters(n_lines=4, n_sites=3, n_bases=7, n_before_start=1))

# Where the library fails and the Java dies or misleads: (sites file, bed, what the message names)
ERRORS = {
    "empty_file": (b"", False, "empty"),
    "empty_file_bed": (b"", True, "empty"),
    "eleven_fields": (table(row(b"c1", 1, 4, b"+"), b"\t".join(row(b"c1", 1, 4, b"+").split(b"\t")[:11])), False, "line 3"),
    "twelfth_field_empty": (table(row(b"c1", 1, 4, b"+", b"")), False, "line 2"),          # split drops it: eleven fields
    "blank_line": (table(row(b"c1", 1, 4, b"+"), b"", row(b"c1", 1, 4, b"+")), False, "line 3"),
    "blank_last_line": (table(row(b"c1", 1, 4, b"+")) + b"\n", False, "line 3"),
    "bed_four_fields": (b"h\nchr7\t1\t4\tname\n", True, "line 2"),
    "bed_blank_line": (b"h\nchr7\t1\t4\tname\t+\n\r\nchr7\t1\t4\tname\t+\n", True, "line 3"),
    "start_not_a_number": (table(row(b"c1", 1, 4, b"+"), row(b"c1", "12a", 4, b"+")), False, "line 3"),
    "end_too_large": (table(row(b"c1", 1, "2147483648", b"+")), False, "line 2"),
    "end_empty": (table(row(b"c1", 1, "", b"+")), False, "line 2"),
    "start_with_space": (b"h\nchr7\t 1\t4\tname\t+\n", True, "line 2"),
    "first_bad_line_is_named": (table(row(b"c1", 1, 4, b"+"), row(b"c1", "x", 4, b"+"), b"short", row(b"c1", 1, "y", b"+")), False, "line 3"),
}


@pytest.mark.parametrize("key", sorted(CASES))
def test_hand_worked_cases(key):
    sites, bed, exp_out, exp_st = CASES[key]
    out, st = J.fetch(GENOME, sites, bed)
    assert out == exp_out
    assert st == exp_st


@pytest.mark.parametrize("key", sorted(ERRORS))
def test_where_the_java_dies(key):
    sites, bed, what = ERRORS[key]
    with pytest.raises(J.FetchError, match=what):
        J.fetch(GENOME, sites, bed)


def test_restatement_primitives():
    g = J.read_fasta(GENOME)
    assert g == {b"c1": b"ACGTNNNNacgtRACGTTGC", b"7": b"AAAACCCC", b"chr7": b"GGGGTTTTAC"}
    assert J.read_fasta(b"junk\n>a x y\r\nAC GT\r\n\r\nN\n>b\n>a\nTTTT\n>\nGG") == {b"a": b"ACGTN", b"b": b"", b"": b"GG"}
    assert J.reverse_complement(b"ACGTacgtNnRy*") == b"*yRnNacgtACGT"
    st = dict.fromkeys(J.INT_KEYS, 0)
    assert J.subsequence(g, b"7", 2, 1, st) == b"" and J.subsequence(g, b"7", 8, 8, st) == b"C" and not any(st.values())
    assert J.subsequence(g, b"7", 3, 1, st) == b"" and st["n_inverted"] == 1


def test_header_declares_and_capi_exports():
    import ctypes as C
    import capi
    head = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "parasuite_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ps_fetch_sequences\s*\(", head) and "ps_fetch_stats" in head
    assert "ps_fetch_sequences" in capi.EXPORTS and hasattr(capi.lib(), "ps_fetch_sequences")
    names = [k for k, _ in capi.FetchStats._fields_]
    assert names[:len(J.INT_KEYS)] == list(J.INT_KEYS) and names[len(J.INT_KEYS):] == ["n_pieces", "s_total", "s_read", "s_index", "s_kernels", "s_write"]
    assert C.sizeof(capi.FetchStats) == 8 * 15


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
@pytest.mark.parametrize("bed", [False, True])
def test_library_fails_loudly_without_device(tmp_path, bed):
    import capi
    fa, sites = tmp_path / "g.fa", tmp_path / "sites.tsv"
    fa.write_bytes(GENOME)
    sites.write_bytes(CASES["bed_chr_prefix" if bed else "holes_both_strands"][0])
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_fetch_sequences(str(fa), str(sites), str(tmp_path / "out.txt"), bed)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["g.fa", "sites.tsv"]
