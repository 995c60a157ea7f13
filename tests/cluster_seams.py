"""Inputs that put ps_pileup_clusters on the seams of its own layout (csrc/ps_clusters.hip), shared by
tests/test_cluster_seams_cpu.py (the inputs have the properties claimed, by the restatement alone) and
tests/test_gpu_cluster_seams.py (the library writes the restatement's bytes):

  A1  k_cl_sitefreq: chunks of 56 crosslinked clusters, blocks of 64 ranks; n in {1, 55, 56, 57, 112, 113} crosslinked
      clusters of which one has 65 kept sites (a second block of ranks, table of 128 buckets), first, in the middle or last;
      one file whose first 56 written clusters are not crosslinked
  A2  k_cl_reduce: windows of 64, 65, 128 and 129 positions with sites at offsets 0, 63, 64, 127, 128; ties across the
      64-position step decided by bucket and by first insertion; a known SNP on offset 64
  A3  k_cl_sum: 8 and 9 sites in one bucket of the 16-bucket table, and the same sites in the 32-bucket table
  A4  k_cl_fix: records that are locally out of order under an SO:coordinate header, where the running maximum and the
      Java's recurrence disagree
  A5  k_cl_classify: 65,535 and 65,536 aligned bases, a record past its contig's end, SEQ '*', read indices 50 and 51

Everything is built here from seeded generators over a reference this module makes itself: "ACG" letters at random with T
exactly where a case asks for one.  Test infrastructure, not product code."""
import random

L_S, L_2 = 60000, 65600


def _contig(n, seed):
    rng = random.Random(seed)
    return bytearray(rng.choice(b"ACG") for _ in range(n))


_REF = {"chrS": _contig(L_S, 11), "c2": _contig(L_2, 12)}
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrS\tLN:%d\n@SQ\tSN:c2\tLN:%d\n" % (L_S, L_2)


def _set_t(chrom, positions):
    for p in positions:
        _REF[chrom][p - 1] = ord("T")


def rd(name, chrom, pos, n, sites=(), flag=0):
    """an <n>M record whose SEQ copies the reference, with C at the reference positions `sites` (each holds a T)"""
    seq = bytearray(_REF[chrom][pos - 1:pos - 1 + n])
    assert len(seq) == n, (name, pos, n)
    for s in sites:
        assert pos <= s < pos + n and _REF[chrom][s - 1] == ord("T"), (name, s)
        seq[s - pos] = ord("C")
    return "%s\t%d\t%s\t%d\t37\t%dM\t*\t0\t0\t%s\t*\n" % (name, flag, chrom, pos, n, seq.decode())


def vcf(positions, chrom="S"):
    """T>C records at chrS positions (CHROM without "chr", as SNPCalling strips it)"""
    return ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n" + "".join("%s\t%d\t.\tT\tC\n" % (chrom, p) for p in positions)).encode()


# ---- A1: rank and chunk seams of .sitefrequency.tsv

A1_BASE, A1_STRIDE, A1_SLOTS = 1000, 200, 171
A1_N = (1, 55, 56, 57, 112, 113)
A1_PLACES = ("first", "middle", "last")
for _s in range(A1_SLOTS):                                                    # 65 T per slot: offsets 5..69 of its 75 bases
    _set_t("chrS", range(A1_BASE + A1_STRIDE * _s + 5, A1_BASE + A1_STRIDE * _s + 70))


def a1_patterns(n, place, seed=0):
    """per cluster [(T index 0..64, reads that convert it: 1 or 2 of 2)]: 1-3 sites, 3 in every 56th cluster (so the first
    of each staged chunk has a rank >= 1), exactly one in cluster 1, and 65 in the cluster `place` names"""
    rng = random.Random(1000 * n + seed)
    pats = []
    for c in range(n):
        k = 3 if c % 56 == 0 else 1 if c == 1 else rng.randint(1, 3)
        pats.append([(o, rng.choice((1, 2))) for o in sorted(rng.sample(range(65), k))])
    pats[{"first": 0, "middle": n // 2, "last": n - 1}[place]] = [(o, rng.choice((1, 2))) for o in range(65)]
    return pats


def _a1_cluster(slot, pat):
    """two 75M reads, the second 0..5 bases further on; both cover every T of the slot"""
    b = A1_BASE + A1_STRIDE * slot
    sites = lambda need: [b + 5 + o for o, k in pat if k >= need]
    return rd("s%da" % slot, "chrS", b, 75, sites(1)) + rd("s%db" % slot, "chrS", b + slot % 6, 75, sites(2))


def _a1_weak(slot):
    """six 75M reads with one T->C in one of them: fraction 1/6 < 0.2, a written cluster that is not crosslinked"""
    b = A1_BASE + A1_STRIDE * slot
    return rd("w%da" % slot, "chrS", b, 75, [b + 5 + slot % 65]) + "".join(rd("w%d%s" % (slot, x), "chrS", b, 75) for x in "bcdef")


def _sentinel(slot):                                                          # the last cluster is never written
    return rd("z", "chrS", A1_BASE + A1_STRIDE * slot, 10)


def a1_sam(n, place, swap=False, lead=0):
    """`lead` weak clusters, then n crosslinked ones; swap: the first two crosslinked clusters trade their sites"""
    pats = a1_patterns(n, place)
    if swap:
        pats[0], pats[1] = pats[1], pats[0]
    return (HEADER + "".join(_a1_weak(s) for s in range(lead)) + "".join(_a1_cluster(lead + c, p) for c, p in enumerate(pats))
            + _sentinel(lead + n))


A1_CASES = [(n, place) for n in A1_N for place in A1_PLACES if n > 1 or place == "first"]
A1_LEAD = (57, "last", 56)                                                    # n, place, lead

# ---- A2: window seams of k_cl_reduce

A2_BASE, A2_STRIDE = 36000, 400                                               # multiples of 16: bucket = window offset & 15
A2_OFFSETS = (0, 63, 64, 127, 128)


def _a2_cluster(tag, lo, W, long_sets, conv0):
    """two 10M reads at lo (the first conv0 of them convert offset 0), then one (W - 2)M read at lo + 2 per entry of
    long_sets, converting those window offsets: the window is [lo, lo + W - 1]"""
    _set_t("chrS", [lo + o for o in A2_OFFSETS + (5, 30, 48) if o < W])
    out = "".join(rd("%s_s%d" % (tag, i), "chrS", lo, 10, [lo] if i < conv0 else []) for i in range(2))
    return out + "".join(rd("%s_l%d" % (tag, i), "chrS", lo + 2, W - 2, sorted(lo + o for o in s)) for i, s in enumerate(long_sets))


def _a2_build():
    """(SAM text, VCF bytes, [(tag, window lo, W, expected best offset)])"""
    specs = []
    for W in (64, 65, 128, 129):                                              # one winner (every read converts it) per offset
        offs = [o for o in A2_OFFSETS if o < W]
        for win in offs:
            rest = {o for o in offs if o and o != win}
            one = {win} if win else set()
            specs.append(("w%d_best%d" % (W, win), 0, W, [rest | one, one, one], 2 if win == 0 else 1, win))
    # 63 and 64 tie at 3/3: lane 63 of the first step against lane 0 of the second; the larger bucket wins
    specs.append(("tie_bucket_63", 0, 129, [{63, 64, 127, 128}, {63, 64}, {63, 64}], 1, 63))      # buckets 15 and 0
    specs.append(("tie_bucket_64", 1, 129, [{63, 64, 127, 128}, {63, 64}, {63, 64}], 1, 64))      # buckets 0 and 1
    # 48 and 64 tie at 2/3 in one bucket: the site first seen by the later record wins
    specs.append(("tie_first_48", 0, 129, [{64, 127}, {48}, {48, 64}], 1, 48))
    specs.append(("tie_first_64", 0, 129, [{48, 127}, {64}, {48, 64}], 1, 64))
    # offset 64 is a known SNP with the largest fraction: kept fractions and sites compact differently from there on
    specs.append(("snp_64", 0, 129, [{63, 64, 127, 128}, {64, 128}, {64}], 1, 128))
    text, expect, snps = HEADER, [], []
    for i, (tag, shift, W, long_sets, conv0, win) in enumerate(specs):
        lo = A2_BASE + A2_STRIDE * i + shift
        text += _a2_cluster(tag, lo, W, long_sets, conv0)
        expect.append((tag, lo, W, win))
        if tag == "snp_64":
            snps.append(lo + 64)
    return text + rd("z", "chrS", A2_BASE + A2_STRIDE * len(specs), 10), vcf(snps), expect


A2_SAM, A2_VCF, A2_EXPECT = _a2_build()
assert A2_BASE + A2_STRIDE * (len(A2_EXPECT) + 1) <= 45000

# ---- A3: more than 8 sites in one bucket of the final table

A3_P, A3_13 = 46005, 45003                                                    # sites A3_P + 16 k; 13 adjacent sites before them
_set_t("chrS", [A3_P + 16 * k for k in range(9)] + list(range(A3_13, A3_13 + 13)))


def a3_sam(n_sites, after_13=False, after_plain=False):
    """after_13: a 13-site cluster first (the table grows to 32 buckets); after_plain: a cluster without sites first"""
    first = rd("t13", "chrS", A3_13 - 3, 20, range(A3_13, A3_13 + 13)) if after_13 else rd("t0", "chrS", A3_13 - 3, 10) if after_plain else ""
    return HEADER + first + rd("b%d" % n_sites, "chrS", A3_P - 3, 140, [A3_P + 16 * k for k in range(n_sites)]) + rd("z", "chrS", 47000, 10)


A3_SNP_VCF = vcf([A3_P + 16 * k for k in range(3)])                           # three of the nine sites, all in the first 64-position step, are known SNPs

# ---- A4: rule 2 where the records are locally out of order


def scan_opens(recs):
    """the device's first answer (k_cl_open): record j opens iff the running maximum of the ends of its reference, taken
    over the records before it, lies less than 5 beyond its start.  recs: (reference, start, end) in file order"""
    out, ref, M = [], None, 0
    for r, s, e in recs:
        o = r != ref or M - s < 5
        M = e if r != ref else max(M, e)
        ref = r
        out.append(o)
    return out


def java_opens(recs):
    """PileupClusters.java:175-176 with :346-357 and :416-499: clusterEnd is the opener's end, raised by members"""
    out, ref, c = [], None, 0
    for r, s, e in recs:
        o = r != ref or c - s < 5
        c = e if o else max(c, e)
        ref = r
        out.append(o)
    return out


def sorted_rules_agree(n_records=6, width=12, spans=range(1, 7)):
    """every coordinate-sorted sequence of up to n_records records with starts in [0, width) and the given spans, as the
    set of states (last start, running maximum, clusterEnd) they reach: both rules only look at that state and the next
    record, so checking every step out of every reachable state covers every such sequence.  Returns (states, steps)."""
    states, seen, steps = {(s, s + n - 1, s + n - 1) for s in range(width) for n in spans}, 0, 0
    for _ in range(n_records - 1):
        nxt = set()
        for s0, M, c in states:
            for s in range(s0, width):
                for n in spans:
                    e = s + n - 1
                    o_scan, o_java = M - s < 5, c - s < 5
                    if o_scan != o_java:
                        return None
                    steps += 1
                    nxt.add((s, max(M, e), e if o_java else max(c, e)))
        seen += len(states)
        states = nxt
    return seen + len(states), steps


A4_T = {"chrS": (50110, 50121, 50127, 50129, 50131, 50133, 50135, 50139, 50310, 50331, 50333, 50335), "c2": (110, 131, 133, 135)}
for _c, _ps in A4_T.items():
    _set_t(_c, _ps)
A4_RECORDS = [          # (reference, start, length); the comments give the Java's clusterEnd c and the running maximum M
    ("chrS", 50100, 41),    # opens; c = M = 50140
    ("chrS", 50137, 1),     # M - start = 3: opens for both, ends below M: c = 50137
    ("chrS", 50130, 3),     # joins for both (c - start = 7); c stays
    ("chrS", 50134, 3),     # c - start = 3: the Java opens, M - start = 6: the scan does not; c = 50136
    ("chrS", 50131, 10),    # joins (c - start = 5) although it starts before its opener, and raises c to 50140
    ("chrS", 50137, 1),     # opens for both and ends below M again: the second stretch follows the first
    ("chrS", 50134, 2),     # Java opens, c = 50135
    ("chrS", 50132, 2),     # Java opens, c = 50133
    ("chrS", 50130, 2),     # Java opens, c = 50131
    ("chrS", 50128, 2),     # Java opens, c = 50129
    ("chrS", 50120, 4),     # joins (c - start = 9)
    ("chrS", 50126, 2),     # Java opens, c = 50127
    ("chrS", 50300, 41),    # far beyond M: opens for both, in step again; c = M = 50340
    ("chrS", 50337, 1),     # opens below M
    ("chrS", 50334, 2),     # Java opens
    ("chrS", 50332, 2),     # Java opens
    ("chrS", 50330, 2),     # Java opens; the stretch ends at the change of reference
    ("c2", 100, 41),
    ("c2", 137, 1),         # opens below M
    ("c2", 134, 2),         # Java opens
    ("c2", 132, 2),         # Java opens
    ("c2", 130, 2),         # Java opens
    ("c2", 128, 2),         # Java opens; the stretch runs to the last record
]


def a4_sam():
    out = HEADER
    for i, (c, s, n) in enumerate(A4_RECORDS):
        out += rd("u%d" % i, c, s, n, [p for p in A4_T[c] if s <= p < s + n and (p + i) % 3])
    return out


A4_SPANS = [(c, s, s + n - 1) for c, s, n in A4_RECORDS]

# ---- A5: the edges of k_cl_classify

A5_SITES = (32752, 40000, 40016)                                              # read indices 32751, 39999, 40015; all in bucket 0 of 16
_set_t("c2", A5_SITES)
_set_t("chrS", (52050, 52051))
A5_LONG_OK = HEADER + rd("long", "c2", 1, 65535, A5_SITES) + rd("z", "c2", 65590, 10)
A5_LONG_BAD = HEADER + rd("long", "c2", 1, 65536, A5_SITES) + rd("z", "c2", 65590, 10)
A5_PAST_END = HEADER + rd("a", "chrS", 100, 10) + "past\t0\tchrS\t%d\t37\t10M\t*\t0\t0\tACGACGACGA\t*\n" % (L_S - 8) + rd("z", "c2", 100, 10)
A5_NO_SEQ = HEADER + rd("a", "chrS", 100, 10) + "noseq\t0\tchrS\t200\t37\t10M\t*\t0\t0\t*\t*\n" + rd("z", "chrS", 300, 10)
A5_INDEX_50_51 = HEADER + rd("i", "chrS", 52000, 60, (52050, 52051)) + rd("z", "chrS", 52200, 10)

REF = {k: bytes(v) for k, v in _REF.items()}                                  # every T is set: the reference as the tests use it
FA = "".join(">%s\n%s" % (n, "".join(s[i:i + 80].decode() + "\n" for i in range(0, len(s), 80))) for n, s in REF.items())
