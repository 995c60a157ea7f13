"""ValidateBenchmarkStatisticsPARCLIP.calculateBenchmarkStatistics (ValidateBenchmarkStatisticsPARCLIP.java:43-242) as
tests/java_benchmark.py restates it, against answers worked out by hand on hand-built SAM + FASTQ pairs.  The GPU entry point
ps_benchmark_reads is held to the same bytes and counters in tests/test_gpu_benchmark.py, which imports the cases from here."""
import os
import re

import numpy as np
import pytest

import java_benchmark as J
from test_capi_cpu import ROOT, _no_gpu

CONTIGS = ("c1", "c2")


def header(contigs=CONTIGS):
    return "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:100000\n" % c for c in contigs)


def name(chrom="c1", start="1000", end="1049", bound="1-1:0"):
    """a read name in the simulator's format: gene|transcript|contig|start|end|bound-cluster:read"""
    return "SEQ_ID:g0|t0|%s|%s|%s|%s" % (chrom, start, end, bound)


def rec(qname, flag, chrom, pos, cigar):
    n = 50 if cigar == "*" else sum(int(x) for x, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")
    return "%s\t%d\t%s\t%d\t37\t%s\t*\t0\t0\t%s\t%s\n" % (qname, flag, chrom, pos, cigar, "A" * n, "I" * n)


def fastq(names, end="\n"):
    return "".join("@%s%sACGT%s+%sIIII%s" % (n, end, end, end, end) for n in names).encode()


def text(matched, processed, reads, precision, recall, accuracy):
    return ("matched correctly:\t%d\nreadsProcessed:\t%d\nall reads:\t%d\nprecision:\t%s\nrecall:\t%s\naccuracy:\t%s"
            % (matched, processed, reads, precision, recall, accuracy)).encode()


def counters(**kw):
    st = dict.fromkeys(J.INT_KEYS, 0)
    st.update(kw)
    return st


def case(contigs, pairs, exp_text, **cnt):
    """pairs: (read name, SAM record) in file order; the FASTQ holds the same names"""
    return header(contigs) + "".join(r for _, r in pairs), fastq([n for n, _ in pairs]), exp_text, counters(**cnt)


P, N = name(), name(bound="0-1:0")          # truth c1:1000-1049, bound / not bound
CASES = {}

# The window (:145-147): start - 5 <= alignment start and end + 5 >= alignment end, truth 1000-1049.
#   r0 bound, c1:1000 50M (end 1049): TP        r1 not bound, the same place: TN      r2 bound, on c2: names differ
#   r3 start 995 = 1000 - 5: TP                 r4 start 994: outside
#   r5 1005 50M, end 1054 = 1049 + 5: TP        r6 1006 50M, end 1055: outside
# FASTQ: 6 positives, 1 negative.  TP 3, TN 1, FP 6 - 3 = 3, FN 1 - 1 = 0: precision 3/6, recall 3/3, accuracy 4/7 (0.5714286 as a float)
CASES["window"] = case(CONTIGS, [(P, rec(P, 0, "c1", 1000, "50M")), (N, rec(N, 16, "c1", 1000, "50M")), (P, rec(P, 0, "c2", 1000, "50M")),
                                 (P, rec(P, 0, "c1", 995, "50M")), (P, rec(P, 0, "c1", 994, "50M")), (P, rec(P, 16, "c1", 1005, "50M")),
                                 (P, rec(P, 0, "c1", 1006, "50M"))],
                       text(4, 7, 7, "0.5", "1.0", "0.5714286"),
                       n_lines=28, n_reads=7, n_positives=6, n_negatives=1, n_records=7, n_processed=7, n_tp=3, n_tn=1, n_other_contig=1, n_outside=2)

# CIGAR and the end: r0 25M5D25M covers 55 bases, end 1054: TP; r1 25M6D25M ends at 1055: outside; r2 10S50M at 1005 ends at
# 1054 (the clip covers no reference; counted, the end would be 1064): TP; r3 a secondary record (flag 256) counts like any other: TP.
# 4 positives, TP 3, FP 1: precision 3/4, recall 3/3, accuracy 3/4
CASES["cigar"] = case(CONTIGS, [(P, rec(P, 0, "c1", 1000, "25M5D25M")), (P, rec(P, 0, "c1", 1000, "25M6D25M")), (P, rec(P, 0, "c1", 1005, "10S50M")),
                                (P, rec(P, 256, "c1", 1000, "50M"))],
                      text(3, 4, 4, "0.75", "1.0", "0.75"),
                      n_lines=16, n_reads=4, n_positives=4, n_records=4, n_processed=4, n_tp=3, n_outside=1)

# Flag 4 (alignment end 0): r0 keeps c1:1000, 995 <= 1000 and 1054 >= 0: TP; r1 keeps c1:900, 995 <= 900 fails: outside;
# r2 is '*' at 0, not bound: unplaced.  2 positives, 1 negative, TP 1, TN 0, FP 1, FN 1: precision 1/2, recall 1/2, accuracy 1/3
CASES["flag4"] = case(CONTIGS, [(P, rec(P, 4, "c1", 1000, "50M")), (P, rec(P, 20, "c1", 900, "50M")), (N, rec(N, 4, "*", 0, "*"))],
                      text(1, 3, 3, "0.5", "0.5", "0.33333334"),
                      n_lines=12, n_reads=3, n_positives=2, n_negatives=1, n_records=3, n_processed=3, n_tp=1, n_outside=1, n_unplaced=1)

# No contig starts with "chr": a truth name loses its "chr" (:136-138).  r0 chr1 -> 1 on contig 1: TP; r1 chr2 -> 2 on contig 1:
# names differ; r2 chrM -> M on contig M (not "chrM", so no chrMT): TP.  3 positives: 2/3, 2/2, 2/3
A, B, C = name("chr1"), name("chr2"), name("chrM")
CASES["chr_only_in_names"] = case(("1", "2", "M"), [(A, rec(A, 0, "1", 1000, "50M")), (B, rec(B, 0, "1", 1000, "50M")), (C, rec(C, 0, "M", 1000, "50M"))],
                                  text(2, 3, 3, "0.6666667", "1.0", "0.6666667"),
                                  n_lines=12, n_reads=3, n_positives=3, n_records=3, n_processed=3, n_tp=2, n_other_contig=1)

# The reverse: contig chr1, truth "1" gets "chr" (the flag is set by the record itself, :131-135): TN; truth "chr1" stays: TN.
# No positives: precision 0/0 NaN; FN 2 - 2 = 0, recall 0/0 NaN; accuracy 2/2
A, B = name("1", bound="0-1:0"), name("chr1", bound="0-1:1")
CASES["chr_only_in_contigs"] = case(("chr1",), [(A, rec(A, 0, "chr1", 1000, "50M")), (B, rec(B, 0, "chr1", 1000, "50M"))],
                                    text(2, 2, 2, "NaN", "NaN", "1.0"),
                                    n_lines=8, n_reads=2, n_negatives=2, n_records=2, n_processed=2, n_tn=2)

# The flag is sticky: r0 truth 1 on contig 1: TP; r1 truth 2 on chr2 sets it, chr2: TP; r2 truth 1 on contig 1 is now chr1: names differ
A, B = name("1"), name("2")
CASES["sticky_chr"] = case(("1", "chr2"), [(A, rec(A, 0, "1", 1000, "50M")), (B, rec(B, 0, "chr2", 1000, "50M")), (A, rec(A, 0, "1", 1000, "50M"))],
                           text(2, 3, 3, "0.6666667", "1.0", "0.6666667"),
                           n_lines=12, n_reads=3, n_positives=3, n_records=3, n_processed=3, n_tp=2, n_other_contig=1)

# chrM becomes chrMT (:141-143): on contig chrM truth M -> chrM -> chrMT and truth chrM -> chrMT both miss; on contig chrMT truth
# M, chrM, chrMT and MT (-> chrMT) all hit.  6 positives, TP 4: 4/6, 4/4, 4/6
M = [name(t) for t in ("M", "chrM", "M", "chrM", "chrMT", "MT")]
CASES["mitochondrion"] = case(("chrM", "chrMT"), [(M[k], rec(M[k], 0, "chrM" if k < 2 else "chrMT", 1000, "50M")) for k in range(6)],
                              text(4, 6, 6, "0.6666667", "1.0", "0.6666667"),
                              n_lines=24, n_reads=6, n_positives=6, n_records=6, n_processed=6, n_tp=4, n_other_contig=2)

# The bound class is field 5 before its first '-': "2" nothing; "-1-3" is "" (split gives "", "1", "3"): nothing; field 5 empty
# before a seventh field: "": nothing; "1": TP; "0-7": TN.  All five lie in the window.  1 positive, 1 negative: 1/1, 1/1, 2/2
Bn = [name(bound=b) for b in ("2", "-1-3", "|x", "1", "0-7")]
CASES["bound_classes"] = case(CONTIGS, [(b, rec(b, 0, "c1", 1000, "50M")) for b in Bn],
                              text(2, 5, 5, "1.0", "1.0", "1.0"),
                              n_lines=20, n_reads=5, n_positives=1, n_negatives=1, n_records=5, n_processed=5, n_tp=1, n_tn=1, n_other_bound=3)

# Integer.parseInt: "+1000" is 1000: TP; "-3" .. "+7" around c1:1 5M (-8 <= 1, 12 >= 5): TP; start -2147483648 is valid and
# start - 5 wraps to 2147483643 > 1000: outside; end 2147483647 + 5 wraps to -2147483644 < 1049: outside.  4 positives: 2/4, 2/2, 2/4
Nn = [name(start="+1000"), name(start="-3", end="+7"), name(start="-2147483648"), name(end="2147483647")]
CASES["numbers"] = case(CONTIGS, [(Nn[0], rec(Nn[0], 0, "c1", 1000, "50M")), (Nn[1], rec(Nn[1], 0, "c1", 1, "5M")), (Nn[2], rec(Nn[2], 0, "c1", 1000, "50M")),
                                  (Nn[3], rec(Nn[3], 0, "c1", 1000, "50M"))],
                        text(2, 4, 4, "0.5", "1.0", "0.5"),
                        n_lines=16, n_reads=4, n_positives=4, n_records=4, n_processed=4, n_tp=2, n_outside=2)

# A number that does not parse ends the loop (:177): r0 TP, r1 is never counted and hides r2 (a TP); the file is written with
# readsProcessed 1.  The FASTQ pass reads no numbers: 3 positives.  TP 1, FP 2: 1/3, 1/1, 1/3
for key, bad in (("bad_number_too_large", name(start="2147483648")), ("bad_number_empty", name(end="")), ("bad_number_letters", name(start="12a"))):
    CASES[key] = case(CONTIGS, [(P, rec(P, 0, "c1", 1000, "50M")), (bad, rec(bad, 0, "c1", 1000, "50M")), (P, rec(P, 0, "c1", 1000, "50M"))],
                      text(1, 1, 3, "0.33333334", "1.0", "0.33333334"),
                      n_lines=12, n_reads=3, n_positives=3, n_records=3, n_processed=1, n_tp=1, bad_number_record=2)

# The same with a short name behind the bad number: the loop has ended before the Java could die on it.  The FASTQ has good names.
SHORT = "SEQ_ID:g0|t0|c1|1000|1049|"          # the trailing empty field is dropped: five fields
BAD = name(start="x")
CASES["bad_number_before_short_name"] = (header() + rec(P, 0, "c1", 1000, "50M") + rec(BAD, 0, "c1", 1000, "50M") + rec(SHORT, 0, "c1", 1000, "50M"),
                                         fastq([P, P, P]), text(1, 1, 3, "0.33333334", "1.0", "0.33333334"),
                                         counters(n_lines=12, n_reads=3, n_positives=3, n_records=3, n_processed=1, n_tp=1, bad_number_record=2))

# Line ends: "\r\n", bare "\r", and no end after the last line: 8 lines, one positive, one negative; TP and TN: 1/1, 1/1, 2/2
CASES["line_ends"] = (header() + rec(P, 0, "c1", 1000, "50M") + rec(N, 0, "c1", 1000, "50M"),
                      fastq([P], "\r\n") + fastq([N], "\r")[:-1], text(2, 2, 2, "1.0", "1.0", "1.0"),
                      counters(n_lines=8, n_reads=2, n_positives=1, n_negatives=1, n_records=2, n_processed=2, n_tp=1, n_tn=1))

# A quality line may start with "@SEQ_ID" (Phred 31 is '@'): it is counted like a header, here as a positive next to the one
# real read, a negative.  TN 1, TP 0, FP 1 - 0 = 1, FN 0: precision 0/1 = 0.0, recall 0/0 NaN, accuracy 1/2
CASES["quality_line_counts"] = (header() + rec(N, 0, "c1", 1000, "50M"),
                                ("@%s\nACGTACGTACGTACGTACGT\n+\n@SEQ_ID|a|b|c|d|1-xx\n" % N).encode(), text(1, 1, 1, "0.0", "NaN", "0.5"),
                                counters(n_lines=4, n_reads=1, n_positives=1, n_negatives=1, n_records=1, n_processed=1, n_tn=1))

# Nothing at all: every ratio is 0/0
CASES["empty"] = (header(), b"", text(0, 0, 0, "NaN", "NaN", "NaN"), counters())

# 2048 reads, one bound; its record is the only one: TP 1, FP 0, FN 2047: precision 1/1, recall 1/2048, accuracy 1/2048 = 4.8828125E-4
CASES["one_in_2048"] = (header() + rec(P, 0, "c1", 1000, "50M"), fastq([P] + [N] * 2047), text(1, 1, 2048, "1.0", "4.8828125E-4", "4.8828125E-4"),
                        counters(n_lines=8192, n_reads=2048, n_positives=1, n_negatives=2047, n_records=1, n_processed=1, n_tp=1))

# The mapping's names need not be the FASTQ's: no positives there but a TP here: FP -1, TP + FP = 0: precision 1/0 Infinity;
# FN 1, recall 1/2; accuracy 1/1
CASES["division_by_zero"] = (header() + rec(P, 0, "c1", 1000, "50M"), fastq([N]), text(1, 1, 1, "Infinity", "0.5", "1.0"),
                             counters(n_lines=4, n_reads=1, n_negatives=1, n_records=1, n_processed=1, n_tp=1))

# Where the Java dies: (SAM, FASTQ, what the message names)
DASHES = name(bound="--")
ERRORS = {
    "short_name_in_mapping": (header() + rec(P, 0, "c1", 1000, "50M") + rec(SHORT, 0, "c1", 1000, "50M"), fastq([P, P]), "record 2"),
    "short_name_before_bad_number": (header() + rec(P, 0, "c1", 1000, "50M") + rec(SHORT, 0, "c1", 1000, "50M") + rec(BAD, 0, "c1", 1000, "50M"),
                                     fastq([P, P, P]), "record 2"),
    "dashes_checked_before_numbers": (header() + rec(name(start="x", bound="--"), 0, "c1", 1000, "50M"), fastq([P]), "record 1"),   # :118 runs before :127
    "short_name_in_fastq": (header() + rec(P, 0, "c1", 1000, "50M"), fastq([P, SHORT]), "line 5"),
    "dashes_in_fastq": (header() + rec(P, 0, "c1", 1000, "50M"), fastq([DASHES]), "line 1"),
    "short_quality_line": (header() + rec(P, 0, "c1", 1000, "50M"), ("@%s\nACGTACGTACG\n+\n@SEQ_ID|a|b\n" % P).encode(), "line 4"),
    "lines_not_a_multiple_of_4": (header() + rec(P, 0, "c1", 1000, "50M"), fastq([P]) + b"@x\n", "5 lines"),
}


@pytest.mark.parametrize("key", sorted(CASES))
def test_hand_worked_cases(key):
    sam, fq, exp_text, exp_st = CASES[key]
    got_text, st = J.benchmark(sam, fq)
    assert got_text == exp_text
    assert {k: st[k] for k in J.INT_KEYS} == exp_st
    assert st["n_processed"] == st["n_tp"] + st["n_tn"] + st["n_unplaced"] + st["n_other_contig"] + st["n_outside"] + st["n_other_bound"]
    ratios = [J.float_to_string(np.float32(st[k])) for k in J.FLOAT_KEYS]
    assert ratios == [l.split("\t")[1] for l in exp_text.decode().split("\n")[3:]]


@pytest.mark.parametrize("key", sorted(ERRORS))
def test_where_the_java_dies(key):
    sam, fq, what = ERRORS[key]
    with pytest.raises(J.BenchmarkError, match=what):
        J.benchmark(sam, fq)


def test_java_primitives():
    assert J.java_split(b"a|b||", b"|") == [b"a", b"b"] and J.java_split(b"", b"|") == [b""] and J.java_split(b"||", b"|") == []
    assert J.java_split(b"|a", b"|") == [b"", b"a"] and J.java_split(b"-1-3", b"-") == [b"", b"1", b"3"] and J.java_split(b"--", b"-") == []
    assert [J.parse_int(s) for s in (b"+7", b"-3", b"007", b"-2147483648", b"2147483647")] == [7, -3, 7, -2 ** 31, 2 ** 31 - 1]
    for s in (b"", b"+", b"-", b"12a", b" 1", b"1 ", b"2147483648", b"-2147483649", b"--1", b"1.0"):
        with pytest.raises(J.NumberFormatException):
            J.parse_int(s)
    assert J.read_lines(b"") == [] and J.read_lines(b"a") == [b"a"] and J.read_lines(b"a\n") == [b"a"]
    assert J.read_lines(b"a\r\nb\rc\n\nd") == [b"a", b"b", b"c", b"", b"d"] and J.read_lines(b"\r\r\n\n") == [b"", b"", b""]
    assert J.i32(2 ** 31) == -2 ** 31 and J.i32(-2 ** 31 - 5) == 2 ** 31 - 5


def test_float_to_string():
    f = lambda a, b: J.float_to_string(J.java_float_div(a, b))
    assert [f(1, 3), f(2, 3), f(1, 2048), f(1, 1), f(0, 5), f(0, 0), f(1, 0), f(-1, 0)] == \
        ["0.33333334", "0.6666667", "4.8828125E-4", "1.0", "0.0", "NaN", "Infinity", "-Infinity"]
    assert [f(1, 1000), f(1, 1001), f(-1, 4), f(3, -7), f(9999999, 1), f(10000000, 1), f(16777217, 1), f(123456789, 1)] == \
        ["0.001", "9.99001E-4", "-0.25", "-0.42857143", "9999999.0", "1.0E7", "1.6777216E7", "1.2345679E8"]


def test_header_declares_and_capi_exports():
    import capi
    head = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "parasuite_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ps_benchmark_reads\s*\(", head) and "ps_benchmark_stats" in head
    assert "ps_benchmark_reads" in capi.EXPORTS and hasattr(capi.lib(), "ps_benchmark_reads")
    assert [k for k, _ in capi.BenchmarkStats._fields_] == list(J.INT_KEYS + J.FLOAT_KEYS)


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_library_fails_loudly_without_device(tmp_path):
    import capi
    sam, fq = tmp_path / "m.sam", tmp_path / "r.fq"
    sam.write_text(CASES["window"][0])
    fq.write_bytes(CASES["window"][1])
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_benchmark_reads(str(sam), str(tmp_path / "out.stats"), str(fq))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["m.sam", "r.fq"]
