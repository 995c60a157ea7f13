"""The record table (csrc/ps_bam.h: RecTable, flatten_records) and the Java rules (csrc/ps_java.h), without a device.
tests/rec_table_check.cpp is built from ps_bam.cpp by the host compiler with AddressSanitizer and UBSan and runs as a plain
executable; it prints the table's columns, which are compared here with values worked out from the SAM text."""
import gzip
import os
import struct
import subprocess
import zlib

import pytest

from test_capi_cpu import ROOT

CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
CIGAR, SEQ, NAMES, QUAL = 1, 2, 8, 4            # kRecCigar, kRecSeq, kRecNames, kRecQual
ALL = CIGAR | SEQ | QUAL | NAMES
HEADER = "@HD\tVN:1.6\tSO:queryname\n@SQ\tSN:chrA\tLN:100000\n@SQ\tSN:chrB\tLN:500\n"
REFS = ["chrA", "chrB"]
# name, flag, reference, POS (1-based), MAPQ, CIGAR, SEQ, QUAL
RECORDS = [
    ("a", 0, "chrA", 1, 30, "1M", "A", "I"),                        # a 1-character name; l_seq 1: one padding nibble, one padding QUAL byte
    ("r2", 16, "chrA", 10, 30, "2M", "AC", "*"),                    # l_seq 2, QUAL absent: 0xFF 0xFF
    ("r3", 0, "chrB", 7, 20, "1S2M", "ACG", "!#5"),                 # l_seq 3
    ("x" * 254, 0, "chrB", 100, 0, "2M1I1M1D3N2M", "ACGTNA", "IIIIII"),   # the longest name BAM holds
    ("noseq", 0, "chrA", 5, 3, "4M", "*", "*"),                     # l_seq 0
    ("nocigar", 4, "*", 0, 0, "*", "ACGT", "IJKL"),                 # unplaced: ref -1, pos -1, n_cig 0
    ("r6", 16 + 1024, "chrA", 999, 60, "2=1X", "TTt", "ABC"),
    ("last", 0, "chrB", 500, 1, "1M", "N", "*"),                    # l_seq 1, QUAL absent: 0xFF and the padding 0xFF
]


def sam_text(records):
    return HEADER + "".join("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\n" % r for r in records)


def expected(records, columns, rows=None, sort_order="queryname"):
    """the lines rec_table_check prints, from the SAM fields alone (SAMv1 4.2: CIGAR words len << 4 | op of MIDNSHP=X, bases as
    nibbles of =ACMGRSVTWYHKDBN with the first base in the high nibble, QUAL as Phred values or 0xFF throughout); offsets count
    what the rows taken hold: seq_off in bases, rounded up to even per record"""
    rows = range(len(records)) if rows is None else rows
    lines, cig_off, seq_off, name_off = [], 0, 0, 0
    for i in rows:
        name, flag, rname, pos1, _, cigar, seq, qual = records[i]
        l_seq = 0 if seq == "*" else len(seq)
        words, num = [], ""
        for ch in "" if cigar == "*" else cigar:
            if ch.isdigit():
                num += ch
            else:
                words.append(int(num) << 4 | "MIDNSHP=X".index(ch))
                num = ""
        nib = ["=ACMGRSVTWYHKDBN".index(c.upper()) for c in seq] if l_seq else []
        nib += [0] * (l_seq & 1)
        packed = bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(nib), 2))
        q = (b"\xff" * l_seq if qual == "*" else bytes(ord(c) - 33 for c in qual)) + b"\xff" * (l_seq & 1)
        part = ["%d %d %d %d" % (REFS.index(rname) if rname != "*" else -1, pos1 - 1, flag, l_seq)]
        part.append("%d %d %s" % (cig_off, len(words), ",".join(map(str, words)) or "-") if columns & CIGAR else "-")
        part.append("%d %s %s" % (seq_off, (packed.hex() or "-") if columns & SEQ else "-", (q.hex() or "-") if columns & QUAL else "-")
                    if columns & (SEQ | QUAL) else "-")
        part.append("%d %d %s" % (name_off, len(name), name) if columns & NAMES else "-")
        lines.append(" | ".join(part))
        cig_off += len(words)
        seq_off += len(nib)
        name_off += len(name)
    head = ["n %d" % len(lines), "sort_order %s" % sort_order, "refs chrA:100000 chrB:500",
            "sizes %d %d %d %d" % (cig_off if columns & CIGAR else 0, seq_off // 2 if columns & SEQ else 0, seq_off if columns & QUAL else 0,
                                   name_off if columns & NAMES else 0)]
    return head + lines


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rec") / "rec_table_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g", "-Wall",
                           "-Werror", "-pthread", "-I", CSRC, os.path.join(ROOT, "tests", "rec_table_check.cpp"), os.path.join(CSRC, "ps_bam.cpp"),
                           "-lz", "-o", out])
    return out


def _run(exe, *args, status=0):
    r = subprocess.run([exe] + [str(a) for a in args], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == status, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def _table(exe, path, columns=ALL, threads=1, rows=None, status=0):
    return _run(exe, "table", path, columns, threads, "-" if rows is None else ",".join(map(str, rows)), status=status)


def _sam_and_bam(tmp_path, records, stem):
    import capi
    sam, bam = str(tmp_path / (stem + ".sam")), str(tmp_path / (stem + ".bam"))
    with open(sam, "w") as f:
        f.write(sam_text(records))
    assert capi.ps_sam_to_bam(sam, bam, threads=2)["n_out"] == len(records)
    return sam, bam


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _sam_and_bam(tmp_path_factory.mktemp("recs"), RECORDS, "eight")


def test_the_headers_need_no_hip():
    """system headers only, none of HIP's; ps_bam.h also takes ps_outfiles.h, which is held to the same (and to ps_error.h)"""
    for name, own in (("ps_java.h", []), ("ps_bam.h", ['"ps_outfiles.h"']), ("ps_outfiles.h", ['"ps_error.h"']), ("ps_error.h", [])):
        text = open(os.path.join(CSRC, name)).read()
        includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
        assert includes and all("hip" not in i for i in includes) and [i for i in includes if not i.startswith("<")] == own, (name, includes)


@pytest.mark.parametrize("columns", [ALL, CIGAR | NAMES, CIGAR | SEQ, QUAL, 0])
def test_columns_from_sam_and_bam(exe, files, columns):
    """every column of the eight records, by hand; the same from SAM text and from BAM, on one thread and on three"""
    want = expected(RECORDS, columns)
    for path in files:
        for threads in (1, 3):
            assert _table(exe, path, columns, threads) == want, (path, threads)


def test_worked_by_hand(exe, files):
    """a few fields spelled out, so that expected() above is held to something too"""
    got = _table(exe, files[1])
    assert got[3] == "sizes 14 12 24 %d" % (1 + 2 + 2 + 254 + 5 + 7 + 2 + 4)
    assert got[4] == "0 0 0 1 | 0 1 16 | 0 10 28ff | 0 1 a"                          # A = 1 in the high nibble; 'I' = 40 = 0x28, then the padding
    assert got[5] == "0 9 16 2 | 1 1 32 | 2 12 ffff | 1 2 r2"
    assert got[6] == "1 6 0 3 | 2 2 20,32 | 4 1240 000214ff | 3 2 r3"                # 1S = 1 << 4 | 4
    assert got[8].startswith("0 4 0 0 | 10 1 64 | 14 - - | ")                        # no bases: nothing stored, the offset does not move
    assert got[9] == "-1 -1 4 4 | 11 0 - | 14 1248 28292a2b | 264 7 nocigar"
    assert got[11] == "1 499 0 1 | 13 1 16 | 22 f0 ffff | 273 4 last"


def test_row_subset(exe, files):
    rows = [1, 2, 3, 5, 6]                                                             # neither the first record nor the last
    for path in files:
        for threads in (1, 3):
            assert _table(exe, path, ALL, threads, rows) == expected(RECORDS, ALL, rows)


@pytest.mark.parametrize("n", [0, 1])
def test_zero_records_and_one(exe, tmp_path, n):
    for path in _sam_and_bam(tmp_path, RECORDS[:n], "few"):
        for threads in (1, 3):
            assert _table(exe, path, ALL, threads) == expected(RECORDS[:n], ALL)


def _bgzf(data):
    """data as BGZF blocks of at most 0xff00 bytes, then the end-of-file block (SAMv1 4.1)"""
    out = b""
    for at in list(range(0, len(data), 0xff00)) + [None]:
        chunk = b"" if at is None else data[at:at + 0xff00]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        out += struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return out


def _record_offsets(raw):
    """offsets of the records in an uncompressed BAM"""
    l_text, = struct.unpack_from("<I", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", raw, at)
        at += 8 + l_name
    offs = []
    while at < len(raw):
        offs.append(at)
        at += 4 + struct.unpack_from("<I", raw, at)[0]
    return offs


def test_records_across_bgzf_blocks(exe, tmp_path):
    """3,000 short records: the BAM's body is cut into blocks of 0xff00 bytes wherever that falls, here inside records"""
    records = [("q%d" % i, 16 * (i & 1), "chrA", i + 1, 30, "5M", "ACGTA"[i % 5:] + "ACGTA"[:i % 5], "IJKLM") for i in range(3000)]
    sam, bam = _sam_and_bam(tmp_path, records, "many")
    raw = open(bam, "rb").read()
    sizes, at = [], 0
    while at < len(raw):                                                               # block sizes: BSIZE of the BC field, ISIZE at the block's end
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", raw, at + bsize - 4)[0])
        at += bsize
    assert len([s for s in sizes if s]) >= 3
    starts, inside = set(_record_offsets(gzip.decompress(raw))), 0
    for k in range(1, len(sizes)):
        inside += 0 < sum(sizes[:k]) < sum(sizes) and sum(sizes[:k]) not in starts
    assert inside >= 2                                                                 # block boundaries that are no record boundaries
    want = expected(records, ALL)
    assert _table(exe, bam, ALL, 3) == want and _table(exe, sam, ALL, 3) == want and _table(exe, bam, ALL, 1) == want


def test_truncated_records(exe, files, tmp_path):
    """the last record ("last": 36 bytes, a name of 5 with its NUL, one CIGAR word, one byte of bases, one of QUAL) cut short by its
    block_size: inside the CIGAR it is corrupt whatever is asked for; behind the CIGAR only for who asks for bases or QUAL"""
    raw = gzip.decompress(open(files[1], "rb").read())
    last = _record_offsets(raw)[-1]
    for keep, columns, ok in ((36 + 5 + 2, CIGAR | NAMES, False), (36 + 5 + 2, 0, False), (36 + 5 + 4, CIGAR | NAMES, True), (36 + 5 + 4, SEQ, False),
                              (36 + 5 + 4 + 1, SEQ, True), (36 + 5 + 4 + 1, QUAL, False)):
        path = str(tmp_path / "cut.bam")
        with open(path, "wb") as f:
            f.write(_bgzf(raw[:last] + struct.pack("<I", keep - 4) + raw[last + 4:last + keep]))
        if ok:
            assert _table(exe, path, columns, 3) == expected(RECORDS, columns)
        else:
            assert _table(exe, path, columns, 3, status=2) == ["error: corrupt record 8"]


def test_java_fp_to_string(exe):
    """Double.toString: the strings pinned in test_error_profile.py::test_java_double_to_string; Float.toString: those of
    test_benchmark_cpu.py::test_float_to_string"""
    doubles = ((0.99, "0.99"), (1e-4, "1.0E-4"), (2.1e-5, "2.1E-5"), (5.9e-4, "5.9E-4"), (0.001, "0.001"), (1.0, "1.0"), (0.0, "0.0"), (1e7, "1.0E7"),
               (9999999.0, "9999999.0"), (0.12, "0.12"), (1.0 / 3.0, "0.3333333333333333"), (float("nan"), "NaN"), (123456.5, "123456.5"))
    assert _run(exe, "double", *[repr(v) for v, _ in doubles]) == [s for _, s in doubles]
    floats = (((1, 3), "0.33333334"), ((2, 3), "0.6666667"), ((1, 2048), "4.8828125E-4"), ((1, 1), "1.0"), ((0, 5), "0.0"), ((0, 0), "NaN"),
              ((1, 0), "Infinity"), ((-1, 0), "-Infinity"), ((1, 1000), "0.001"), ((1, 1001), "9.99001E-4"), ((-1, 4), "-0.25"), ((3, -7), "-0.42857143"),
              ((9999999, 1), "9999999.0"), ((10000000, 1), "1.0E7"), ((16777217, 1), "1.6777216E7"), ((123456789, 1), "1.2345679E8"))
    assert _run(exe, "float_div", *[x for ab, _ in floats for x in ab]) == [s for _, s in floats]


def test_java_parse_int(exe):
    """Integer.parseInt(String): an optional single '+' or '-', then one or more decimal digits and nothing else; the value must lie
    in [-2^31, 2^31 - 1], however many digits spell it (leading zeros count for nothing); everything else is a NumberFormatException"""
    cases = (("+7", 7), ("-0", 0), ("2147483647", 2 ** 31 - 1), ("2147483648", None), ("-2147483648", -2 ** 31), ("00000000001", 1), ("", None), ("-", None),
             ("1x", None))
    assert _run(exe, "parse_int", *[s for s, _ in cases]) == ["NumberFormatException" if v is None else str(v) for _, v in cases]
