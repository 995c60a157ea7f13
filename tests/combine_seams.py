"""Inputs that put ps_combine_genome_transcript on the seams of its own layout (csrc/ps_combine.hip: one lane per placed
transcript record in blocks of 256, a scan over the per-record CIGAR word counts, one lane per name group that walks its whole
group, 4096 lifted records per assembling worker), shared by tests/test_combine_seams_cpu.py (the inputs have the properties
claimed, by the restatement tests/java_combine.py alone) and tests/test_gpu_combine_seams.py (the library gives the
restatement's records):

  C1  the exon walk: four small transcripts on both strands, an <l>M record for every start and length up to two bases past
      the transcript's end; on one of them also clipped, inserted, deleted, own-N, flag-4, flag-16 and flag-256 records
  C2  k_cb_lift<0> -> scan -> k_cb_lift<1>: 48 exons of 1-3 bases under a name of several hundred bytes, records of 3, 33, 93
      and 95 CIGAR words between records of none, with the 95-word record first, last, and an unlocated record last
  C3  k_cb_heads, k_cb_groups: n in {1, 255, 256, 257, 512, 513} placed records, groups and name pairs on the block seam
      255 | 256, a group that ends at n - 1, records without reference first, last and in the seam
  C4  k_cb_groups: seven groups of 600 records of one name, one per way the Java's lists decide a group
  C5  k_cb_revcomp: lengths 0, 1, 2, 3, 63, 64, 65, 255, 256, 257 with all sixteen base codes at both ends
  C6  nothing to do: no record, no placed record (n == 0), no located record (no CIGAR word at all)
  C7  the sections above in one file, C1 again under further prefixes until more than 8192 records are lifted: two full
      shares of 4096 for the host's record assembly

Every section returns (genome SAM text, transcript SAM text).  Exon positions have five digits, so that the Java's string
sort of the bounds is the numeric one, and every exon has end >= start after it; exon() asserts both.  Test infrastructure,
not product code."""
import random

import java_combine as J
from test_combine_cpu import GENOME_RECS, g_header, rd, t_header

GENOME = g_header() + GENOME_RECS                                             # chr1, chr2, chrMT, chrM: no chr9


def exon(gene, chrom, strand, base, lengths, introns=()):
    """the transcript name Gene|Transcript|Chr|starts|ends|strand of exons of `lengths` bases, `introns` bases apart, from `base`"""
    assert len(introns) == len(lengths) - 1 and min(lengths) >= 1
    starts, ends, at = [], [], base
    for i, n in enumerate(lengths):
        starts.append(at)
        ends.append(at + n - 1)
        at += n + (introns[i] if i < len(introns) else 0)
    assert all(10000 <= x <= 99999 for x in starts + ends), (gene, starts[0], ends[-1])
    s, e = sorted(map(str, starts)), sorted(map(str, ends))
    assert s == list(map(str, starts)) and e == list(map(str, ends))         # the string sort is the numeric sort
    assert all(int(b) >= int(a) for a, b in zip(s, e))
    return "%s|T%s|%s|%s|%s|%s" % (gene, gene, chrom, ";".join(s), ";".join(e), strand)


def _bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _texts(transcripts, body):
    return GENOME, t_header(tuple(transcripts)) + body


def _tag(i):
    return "XI:i:%d" % i


# ---- C1: every phase of the walk

C1_SHAPES = (("k1", 20000, (1, 2, 1, 3, 5), (1, 2, 7, 1)), ("k2", 21000, (4,), ()), ("k3", 22000, (1,) * 6, (1,) * 5),
             ("k4", 23000, (3, 64, 2), (5, 9)))
C1_BLOCKS = tuple((key, strand) for key, _, _, _ in C1_SHAPES for strand in ("1", "-1"))
C1_TOTAL = {key: sum(lengths) for key, _, lengths, _ in C1_SHAPES}


def c1_transcript(key, strand):
    _, base, lengths, introns = [s for s in C1_SHAPES if s[0] == key][0]
    return exon("C%s%s" % (key, "f" if strand == "1" else "r"), "1", strand, base, lengths, introns)


def c1_spans(key):
    """every (alignment start, reference length) that ends at most two bases past the transcript"""
    total = C1_TOTAL[key]
    return [(a, l) for a in range(1, total + 3) for l in range(1, total + 2 - a + 2)]


def _c1_block(key, strand, prefix, rng):
    """(transcript, SAM lines); a record's name says what it is: <prefix><key><f|r>_<start>_<length>_<kind>"""
    t = c1_transcript(key, strand)
    stem = "%s%s%s" % (prefix, key, "f" if strand == "1" else "r")
    out = []

    def add(a, l, kind, flag, cigar, n_read):
        out.append(rd("%s_%d_%d_%s" % (stem, a, l, kind), flag, t, a, cigar, seq=_bases(rng, n_read), tags="NM:i:0"))

    for a, l in c1_spans(key):
        add(a, l, "m", 0, "%dM" % l, l)
        if key != "k1" or l < 3:
            continue
        add(a, l, "clip", 0, "1S%dM" % l, l + 1)
        add(a, l, "ins", 0, "1M1I%dM" % (l - 1), l + 1)
        add(a, l, "del", 0, "1M1D%dM" % (l - 2), l - 1)
        if l >= 4:
            add(a, l, "ownn", 0, "1M2N%dM" % (l - 3), l - 2)
        for flag in (4, 16, 256):
            add(a, l, "f%d" % flag, flag, "%dM" % l, l)
    return t, out


def _c1(prefix="", blocks=C1_BLOCKS, seed=1):
    rng = random.Random(seed)
    parts = [_c1_block(key, strand, prefix, rng) for key, strand in blocks]
    return [t for t, _ in parts], "".join("".join(lines) for _, lines in parts)


def c1(prefix=""):
    return _texts(*_c1(prefix))


# ---- C2: records of many CIGAR words

_rng2 = random.Random(2)
C2_LENGTHS = tuple(_rng2.randint(1, 3) for _ in range(48))
C2_INTRONS = tuple(_rng2.randint(1, 4) for _ in range(47))
C2_T = {"1": exon("C2f", "1", "1", 40000, C2_LENGTHS, C2_INTRONS), "-1": exon("C2r", "1", "-1", 40000, C2_LENGTHS, C2_INTRONS)}
C2_PLUS = exon("C2p", "1", "+", 41000, (100,))                               # strand "+": nothing is located
C2_ORDERS = ("first", "last", "unlocated_last")
C2_SPANS = ((5, 2), (3, 17), (0, 47), (0, 48))                               # (first exon of the walk, exons spanned)
assert len(C2_T["1"]) > 500


def _c2(order, strand, prefix=""):
    rng = random.Random(20)
    walk = C2_LENGTHS if strand == "1" else C2_LENGTHS[::-1]                 # the exons in the order the walk passes them
    stem = "%sc2%s_%s" % (prefix, "f" if strand == "1" else "r", order)

    def spanning(first, k, tag):
        a, l = sum(walk[:first]) + 1, sum(walk[first:first + k])
        return rd("%s_x%d%s" % (stem, k, tag), 0, C2_T[strand], a, "%dM" % l, seq=_bases(rng, l), tags="NM:i:0")

    def unlocated(i):
        return rd("%s_u%d" % (stem, i), 0, C2_PLUS, 11, "20M", tags="NM:i:0")

    base = [spanning(5, 2, ""), unlocated(1), spanning(3, 17, ""), unlocated(2), spanning(0, 47, ""), unlocated(3)]
    long = spanning(0, 48, "")
    lines = {"first": [long] + base + [spanning(7, 2, "b")], "last": base + [long], "unlocated_last": [long] + base}[order]
    return [C2_T[strand], C2_PLUS], "".join(lines)


def c2(order, strand, prefix=""):
    return _texts(*_c2(order, strand, prefix))


# ---- C3: block seams of the heads and the groups

C3_ONE = exon("C3f", "1", "1", 30000, (1000,))
C3_REV = exon("C3r", "1", "-1", 30000, (1000,))
C3_N = (1, 255, 256, 257, 512, 513)
C3_LAYOUTS = ("single", "head255")
C3_PAIRS = ("last_byte", "first_byte", "prefix", "long254", "returns")
# name groups per (n, layout), by hand: one per record, less the records that join a group.  The last three records share a
# name where that leaves the seam alone (n = 255: 252-254; 512: 509-511; 513: 510-512, across the block seam 511 | 512): -2.
# "head255": records 255-258 share a name, as far as they exist: n = 257: -1, n >= 259: -3.
C3_GROUPS = {(1, "single"): 1, (1, "head255"): 1, (255, "single"): 253, (255, "head255"): 253, (256, "single"): 256, (256, "head255"): 256,
             (257, "single"): 257, (257, "head255"): 256, (512, "single"): 510, (512, "head255"): 507, (513, "single"): 511, (513, "head255"): 508}


def c3_cases():
    """(n, layout, pair): the pairs differ only where a record 256 exists"""
    return [(n, layout, pair) for n in C3_N for layout in C3_LAYOUTS for pair in C3_PAIRS
            if n > 256 or (pair == C3_PAIRS[0] and (n == 256 or layout == C3_LAYOUTS[0]))]


def c3_pair(pair, prefix=""):
    """two names that the head test must tell apart"""
    if pair == "last_byte":
        return prefix + "seam_a", prefix + "seam_b"
    if pair == "first_byte":
        return prefix + "a_seam", prefix + "b_seam"                       # with a prefix: the first byte behind it
    if pair == "prefix":
        return prefix + "x", prefix + "xy"
    if pair == "long254":
        stem = prefix + "L" * (253 - len(prefix))
        return stem + "a", stem + "b"                                      # 254 bytes, the longest name a BAM record holds
    assert pair == "returns"
    return prefix + "back", prefix + "other"                              # ... and "back" again: two groups of that name


def c3_names(n, layout, pair, prefix=""):
    names = ["%sr%04d" % (prefix, j) for j in range(n)]
    p0, p1 = c3_pair(pair, prefix)
    if layout == "single":                                                  # groups of one record at 255 and at 256
        put = {255: p0, 256: p1}
        if pair == "returns":
            put[257] = p0
    else:                                                                   # the head in lane 255, its members in the next block
        put = {254: p0, 255: p1, 256: p1, 257: p1, 258: p1}
        if pair == "returns":
            put[259] = p0
    for j, name in put.items():
        if j < n:
            names[j] = name
    if n >= 3 and (n - 3 > 259 or n - 1 <= 254):                            # a group that ends at n - 1
        names[n - 3:] = [prefix + "tail"] * 3
    return names


def _c3(n, layout, pair, prefix=""):
    names = c3_names(n, layout, pair, prefix)
    star = lambda name: rd(name, 4, "*", 0, "*", tags="NM:i:0")
    lines, head = [star(names[0])], 0
    for j, name in enumerate(names):
        if j and name != names[j - 1]:
            head = j
        if j == 256:
            lines.append(star(name))                                        # neither breaks nor starts a group, shifts no index
        # a group's records lift to one start; with flag 0 throughout the last one goes out, with 0x100 on the others the head
        flag = 256 if j != head and head % 2 else 0
        lines.append(rd(name, flag, C3_REV if head % 3 == 0 else C3_ONE, 1 + (head * 7) % 900, "20M", tags=_tag(j)))
    lines.append(star(names[-1]))
    return [C3_ONE, C3_REV], "".join(lines)


def c3(n, layout, pair, prefix=""):
    return _texts(*_c3(n, layout, pair, prefix))


# ---- C4: groups of 600

C4_SIZE = 600
C4_ABSENT = exon("C4x", "9", "1", 30000, (1000,))                            # the exons of C3_ONE on a contig the genome lacks
C4_PLUS = exon("C4p", "1", "+", 30000, (1000,))
C4_VARIANTS = "abcdefg"
# what goes out of each group: the index of the emitted record (its XI tag), or the counter that takes the group
C4_EXPECT = {"a": 0,                          # every record has 0x100: entry 0
             "b": 599,                        # the only record without 0x100 is the last
             "c": 400,                        # records 100 and 400 are without 0x100: the index stored last
             "d": 599,                        # as b with records 1, 4, 7, ... unlocated: list entry 399 is record 599
             "e": "n_groups_ambiguous",       # as a, the last record one base on
             "f": "n_no_contig",              # the primary record, 300, names a transcript on chr9; the others chr1
             "g": 0}                          # the primary record, 300, is unlocated and stores nothing: entry 0


def _c4(prefix="", variants=C4_VARIANTS):
    lines = []
    for v in variants:
        primary = {"a": (), "b": (599,), "c": (100, 400), "d": (599,), "e": (), "f": (300,), "g": (300,)}[v]
        for i in range(C4_SIZE):
            t = C3_ONE
            if (v == "d" and i % 3 == 1) or (v == "g" and i == 300):
                t = C4_PLUS
            if v == "f" and i == 300:
                t = C4_ABSENT
            pos = 11 + 40 * C4_VARIANTS.index(v) + (1 if v == "e" and i == C4_SIZE - 1 else 0)
            lines.append(rd("%sc4%s" % (prefix, v), 0 if i in primary else 256, t, pos, "20M", tags=_tag(i)))
    return [C3_ONE, C4_ABSENT, C4_PLUS], "".join(lines)


def c4(prefix="", variants=C4_VARIANTS):
    return _texts(*_c4(prefix, variants))


# ---- C5: reverse complement

C5_T = exon("C5r", "1", "-1", 50000, (400,))
C5_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)


def c5_seq(n):
    """the first sixteen bases cycle through the sixteen codes, the last sixteen run the cycle backwards (they win where both meet)"""
    rng = random.Random(500 + n)
    s = list(_bases(rng, n))
    for i in range(min(16, n)):
        s[i] = J.SEQ16[i]
    for i in range(min(16, n)):
        s[n - 1 - i] = J.SEQ16[i]
    return "".join(s)


def _c5(prefix=""):
    lines = []
    for k, n in enumerate(C5_LENGTHS):
        seq = c5_seq(n) if n else "*"
        q = "*" if k % 2 == 0 or not n else "".join(chr(35 + i % 60) for i in range(n))
        lines.append("%sc5_%d\t0\t%s\t%d\t23\t%dM\t*\t0\t0\t%s\t%s\t%s\n" % (prefix, n, C5_T, 3 + k, n or 20, seq, q, _tag(n)))
    return [C5_T], "".join(lines)


def c5(prefix=""):
    return _texts(*_c5(prefix))


# ---- C6: nothing to do

C6_KINDS = ("no_record", "no_placed_record", "no_located_record")


def c6(kind):
    star = "".join(rd("s%d" % i, 4, "*", 0, "*", tags="NM:i:0") for i in range(3))
    if kind == "no_record":
        return _texts([C3_ONE], "")
    if kind == "no_placed_record":
        return _texts([C3_ONE], star)
    assert kind == "no_located_record"
    return _texts([C4_PLUS], "".join(rd("u%d" % (i // 2), 0, C4_PLUS, 11 + i, "20M", tags=_tag(i)) for i in range(300)) + star)


# ---- C7: everything in one file

C7_LIFTED, C7_MAX_RECORDS = 8192, 15000
C7_C3 = ((1, "single", "last_byte"), (255, "single", "last_byte"), (256, "head255", "last_byte"), (257, "single", "long254"),
         (512, "head255", "returns"), (513, "single", "prefix"))


def _n_lifted(transcripts, body):
    return J.combine(J.parse_sam(GENOME), J.parse_sam(t_header(tuple(transcripts)) + body))[3]["n_lifted"]


def _c7():
    parts = [_c1("s1_")]
    parts += [_c2(order, strand, "s2_") for order in C2_ORDERS for strand in ("1", "-1")]
    parts += [_c3(n, layout, pair, "s3%d_" % i) for i, (n, layout, pair) in enumerate(C7_C3)]
    parts += [_c4("s4_"), _c5("s5_")]
    lifted = sum(_n_lifted(t, body) for t, body in parts)                   # no name crosses a part: the counts add up
    rep = 0
    while lifted < C7_LIFTED:                                               # C1 again, one transcript at a time
        parts.append(_c1("s1%c_" % (97 + rep), (C1_BLOCKS[rep % len(C1_BLOCKS)],), seed=100 + rep))
        lifted += _n_lifted(*parts[-1])
        rep += 1
    transcripts = []
    for t, _ in parts:
        transcripts += [x for x in t if x not in transcripts]
    return transcripts, "".join(body for _, body in parts)


_C7 = []


def c7():
    if not _C7:
        _C7.append(_texts(*_c7()))
    return _C7[0]
