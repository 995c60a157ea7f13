"""ValidateBenchmarkStatisticsPARCLIP.calculateBenchmarkStatistics (the toolkit's utils/benchmarking/
ValidateBenchmarkStatisticsPARCLIP.java:43-242) restated in plain Python, one line and one record at a time as the Java walks
them: test infrastructure, the yardstick ps_benchmark_reads is held to (tests/test_benchmark_cpu.py works its answers out by
hand against this file, tests/test_gpu_benchmark.py holds the library to it).  No JVM is at hand, so this is the Java as it
is written, read line by line, not pinned to the jar.

benchmark(sam_text, fastq_bytes) returns (the bytes of the statistics file, the counters of ps_benchmark_stats).  Where the Java
dies -- an uncaught ArrayIndexOutOfBounds on a short name, System.exit on a line count that is no multiple of 4 -- this raises
BenchmarkError, as include/parasuite_hip.h has the library fail.  getAlignmentEnd follows the library's rule (parasuite_hip.h,
ps_combine_genome_transcript): start + reference length of the CIGAR - 1, and 0 for a record with flag 4."""
import re

import numpy as np

INT_KEYS = ("n_lines", "n_reads", "n_positives", "n_negatives", "n_records", "n_processed", "n_tp", "n_tn", "n_unplaced",
            "n_other_contig", "n_outside", "n_other_bound", "bad_number_record")
FLOAT_KEYS = ("precision", "recall", "accuracy")


class BenchmarkError(Exception):
    pass


class NumberFormatException(Exception):
    pass


def i32(x):
    """a Java int: 32 bits, wraps"""
    return (x + 2 ** 31) % 2 ** 32 - 2 ** 31


def java_split(s, sep):
    """String.split with a one-character pattern: trailing empty strings are dropped; a string without a match is itself"""
    parts = s.split(sep)
    if len(parts) == 1:
        return parts
    while parts and parts[-1] == b"":
        parts.pop()
    return parts


def parse_int(s):
    """Integer.parseInt on ASCII: one optional sign, at least one digit, int range"""
    if not re.fullmatch(rb"[+-]?[0-9]+", s):
        raise NumberFormatException(s)
    v = int(s)
    if not -2 ** 31 <= v <= 2 ** 31 - 1:
        raise NumberFormatException(s)
    return v


def read_lines(data):
    """BufferedReader.readLine until null: a line ends at \\n, \\r or \\r\\n; no empty line after a final line end"""
    lines = re.split(rb"\r\n|\n|\r", data)
    if lines[-1] == b"":                                 # nothing behind the last line end (or nothing at all)
        lines.pop()
    return lines


def float_to_string(v):
    """Float.toString (JDK 19+): the shortest decimal that reads back as the same float; d.d.. for 1e-3 <= |v| < 1e7, else d.d..E<n>"""
    v = np.float32(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    if v == 0:
        return "-0.0" if np.signbit(v) else "0.0"
    mant, exp = np.format_float_scientific(abs(v), unique=True, trim="-").split("e")
    digits, e10 = mant.replace(".", "").rstrip("0") or "0", int(exp)
    sign = "-" if v < 0 else ""
    if np.float32(1e-3) <= abs(v) < np.float32(1e7):
        if e10 >= 0:
            ip = digits[:e10 + 1].ljust(e10 + 1, "0")
            return sign + ip + "." + (digits[e10 + 1:] or "0")
        return sign + "0." + "0" * (-e10 - 1) + digits
    return sign + digits[0] + "." + (digits[1:] or "0") + "E" + str(e10)


def java_float_div(a, b):
    """(float) a / b with Java ints a, b: both become floats, IEEE division (0/0 NaN, x/0 an infinity)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(a) / np.float32(b)


def ref_length(cigar):
    return 0 if cigar == "*" else sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MDN=X")


def sam_records(sam_text):
    """(QNAME bytes, flag, reference name, alignment start, alignment end) per alignment line, in file order"""
    out, body = [], False
    for line in sam_text.split("\n"):
        line = line.rstrip("\r")
        if not line or (not body and line.startswith("@")):
            continue
        body = True
        f = line.split("\t")
        flag, pos = int(f[1]), int(f[3])
        out.append((f[0].encode(), flag, f[2], pos, 0 if flag & 4 else i32(pos + ref_length(f[5]) - 1)))
    return out


def bound_class(fields, what):
    """splittedHeader[5].split("-")[0] (:84, :118); either index can be out of bounds"""
    if len(fields) < 6:
        raise BenchmarkError("%s has fewer than six '|' fields" % what)
    first = java_split(fields[5], b"-")
    if not first:
        raise BenchmarkError("%s: field 5 is made of '-' only" % what)
    return first[0]


def benchmark(sam_text, fastq):
    st = dict.fromkeys(INT_KEYS, 0)
    # :78-103
    positives = negatives = 0
    lines = read_lines(fastq)
    for k, line in enumerate(lines):
        if line.startswith(b"@SEQ_ID"):
            b = bound_class(java_split(line, b"|"), "line %d" % (k + 1))
            if b == b"1":
                positives += 1
            elif b == b"0":
                negatives += 1
    if len(lines) % 4:
        raise BenchmarkError("%d lines: not a multiple of 4" % len(lines))
    st.update(n_lines=len(lines), n_reads=len(lines) // 4, n_positives=positives, n_negatives=negatives)
    # :105-163
    recs = sam_records(sam_text)
    st["n_records"] = len(recs)
    processed = tp = tn = 0
    starts_with_chr = False
    try:
        for k, (name, flag, chrom, aln_start, aln_end) in enumerate(recs):
            f = java_split(name, b"|")
            bound = bound_class(f, "record %d" % (k + 1))      # :113-118, all before the numbers are parsed
            read_chr = f[2]
            read_start, read_end = parse_int(f[3]), parse_int(f[4])
            chrom = chrom.encode()
            if chrom.startswith(b"chr"):
                starts_with_chr = True
            if starts_with_chr and not read_chr.startswith(b"chr"):
                read_chr = b"chr" + read_chr
            elif not starts_with_chr and read_chr.startswith(b"chr"):
                read_chr = read_chr[3:]
            if read_chr == b"chrM":
                read_chr = b"chrMT"
            same = read_chr == chrom
            inside = i32(read_start - 5) <= aln_start and i32(read_end + 5) >= aln_end
            if same and inside and bound == b"1":
                tp += 1
            elif same and inside and bound == b"0":
                tn += 1
            else:                                        # the library's breakdown: the first reason that applies
                st["n_unplaced" if chrom == b"*" else "n_other_contig" if not same else "n_outside" if not inside else "n_other_bound"] += 1
            processed += 1
    except NumberFormatException:                        # :177: caught outside the loop, the writer still runs
        st["bad_number_record"] = processed + 1
    st.update(n_processed=processed, n_tp=tp, n_tn=tn)
    # :165-166, :200-225
    fp, fn = i32(positives - tp), i32(negatives - tn)
    precision, recall = java_float_div(tp, i32(tp + fp)), java_float_div(tp, i32(tp + fn))
    accuracy = java_float_div(i32(tp + tn), i32(positives + negatives))
    st.update(precision=float(precision), recall=float(recall), accuracy=float(accuracy))
    text = ("matched correctly:\t%d\nreadsProcessed:\t%d\nall reads:\t%d\nprecision:\t%s\nrecall:\t%s\naccuracy:\t%s"
            % (i32(tp + tn), processed, len(lines) // 4, float_to_string(precision), float_to_string(recall), float_to_string(accuracy)))
    return text.encode(), st


def same_stats(got, exp):
    """None, or the first field in which two stats dicts differ (NaN equals NaN; floats compared as the float32 they are)"""
    if set(got) != set(INT_KEYS + FLOAT_KEYS):
        return "fields: %s" % sorted(got)
    for k in INT_KEYS:
        if int(got[k]) != exp[k]:
            return "%s: %r != %r" % (k, got[k], exp[k])
    for k in FLOAT_KEYS:
        a, b = np.float32(got[k]), np.float32(exp[k])
        if not ((np.isnan(a) and np.isnan(b)) or a == b):
            return "%s: %r != %r" % (k, got[k], exp[k])
    return None
