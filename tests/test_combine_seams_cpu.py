"""The inputs of tests/combine_seams.py have the properties their names claim, shown with the plain restatement
tests/java_combine.py alone, and the restatement's walk is pinned to a genome-position list made straight from the exon
table; tests/test_gpu_combine_seams.py then holds ps_combine_genome_transcript to the restatement's records on the same inputs.
The literals 256 (records or groups per block of every kernel) and 4096 (lifted records per assembling worker) are the
library's own: test_kernel_constants reads them from the sources.  Every comparison is exact."""
import os
import re

import pytest

import combine_seams as S
import java_combine as J

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "para-suite_amd", "csrc")


def combine(texts):
    """(the genomic records, the lifted records, the stats) of a section"""
    genome = J.parse_sam(texts[0])
    _, _, recs, st = J.combine(genome, J.parse_sam(texts[1]))
    assert J.same_records(recs[:len(genome[2])], genome[2]) is None
    return genome[2], recs[len(genome[2]):], st


def xi(rec):
    return int([t for t in rec["tags"] if t.startswith("XI:i:")][0][5:])


def test_kernel_constants():
    """the seam tests are written for one lane per record in blocks of 256 and for one assembling worker per 4096 lifted records"""
    text = open(os.path.join(CSRC, "ps_combine.hip")).read()
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\((\d+)\)\s+)?(k_cb_\w+)", text)
    assert kernels == [("256", k) for k in ("k_cb_lift", "k_cb_heads", "k_cb_groups", "k_cb_revcomp")], "update the seam tests: %r" % kernels
    launches = re.findall(r"hipLaunchKernelGGL\((k_cb_\w+)(?:<\w+>)?, dim3\((.*?)\), dim3\((\d+)\), 0, s,", text)
    assert launches == [(k, "blocks_for((size_t)n)", "256") for k in ("k_cb_lift", "k_cb_lift", "k_cb_heads", "k_cb_groups", "k_cb_revcomp")], \
        "update the seam tests: %r" % launches
    per = re.findall(r"inline unsigned blocks_for\(size_t n, unsigned per = (\d+)\)", open(os.path.join(CSRC, "ps_dev.h")).read())
    assert per == ["256"], "update the seam tests: %r" % per
    rule = re.findall(r"const int W = std::max\(1, std::min<int>\(threads, \(int\)\(out_rec\.size\(\) / (\d+)\) \+ 1\)\);", text)
    assert rule == ["4096"] and S.C7_LIFTED == 2 * 4096, "update the seam tests: %r" % rule


# ---- C1

@pytest.fixture(scope="module")
def c1():
    return combine(S.c1())


def test_restatement_against_exon_map(c1):
    """the <l>M records that lie inside their transcript: walking the lifted CIGAR from the lifted start visits exactly the
    genome positions of the transcript's bases a .. a + l - 1, taken from a list of the exons' positions (reversed on -1)"""
    _, lifted, _ = c1
    by_name = {r["name"]: r for r in lifted}
    assert len(by_name) == len(lifted)
    checked = 0
    for key, strand in S.C1_BLOCKS:
        f = S.c1_transcript(key, strand).split("|")
        bounds = sorted(zip(map(int, f[3].split(";")), map(int, f[4].split(";"))))
        genome = [p for s, e in bounds for p in range(s, e + 1)]
        assert len(genome) == S.C1_TOTAL[key]
        transcript = genome if strand == "1" else genome[::-1]
        for a, l in S.c1_spans(key):
            if a + l - 1 > S.C1_TOTAL[key]:
                continue
            r = by_name["%s%s_%d_%d_m" % (key, "f" if strand == "1" else "r", a, l)]
            at, visited = r["pos"] + 1, []
            for n, op in J.cigar_ops(r["cigar"]):
                assert op in "MN", r
                if op == "M":
                    visited += range(at, at + n)
                at += n
            want = transcript[a - 1:a + l - 1]
            assert visited == (want if strand == "1" else want[::-1]), (r["name"], r["pos"] + 1, r["cigar"])
            assert r["flag"] == (0 if strand == "1" else 16) and len(r["seq"]) == l
            checked += 1
    assert checked == 5048


def test_c1_every_phase_is_present(c1):
    _, lifted, st = c1
    n_spans = sum(len(S.c1_spans(key)) for key, _ in S.C1_BLOCKS)
    assert n_spans == 2 * (105 + 21 + 36 + 2556) and st["n_transcript"] == st["n_groups"] == n_spans + 2 * (6 * 78 + 66) == 6504
    assert st["n_missed_indel_splice"] > 0 and st["n_unlocated"] > 0 and st["n_spliced"] > 0
    assert any(r["cigar"] == "*" for r in lifted)
    assert st["n_lifted"] == len(lifted) == st["n_groups"] - st["n_unlocated"] and st["n_groups_ambiguous"] == st["n_no_contig"] == 0
    kinds = {r["name"].rsplit("_", 1)[1] for r in lifted}
    assert kinds == {"m", "clip", "ins", "del", "ownn", "f4", "f16", "f256"}
    assert any(r["name"].endswith("_ownn") and r["cigar"].count("N") > 1 for r in lifted)      # the own N, then the junctions'
    # starts and ends past the transcript are there, on each strand
    for key, strand in S.C1_BLOCKS:
        total, stem = S.C1_TOTAL[key], key + ("f" if strand == "1" else "r")
        names = {r["name"] for r in lifted}
        assert "%s_%d_1_m" % (stem, total + 1) not in names and "%s_%d_1_m" % (stem, total) in names
        assert ("%s_%d_3_m" % (stem, total) in names) == (strand == "1")                        # runs out past the last exon


# ---- C2

@pytest.mark.parametrize("strand", ["1", "-1"])
@pytest.mark.parametrize("order", S.C2_ORDERS)
def test_c2_long_words(order, strand):
    texts = S.c2(order, strand)
    _, lifted, st = combine(texts)
    words = [J.cigar_ops(r["cigar"]) for r in lifted]
    assert sorted({len(w) for w in words}) == [3, 33, 93, 95]
    longest = max(words, key=len)
    assert [op for _, op in longest] == ["M", "N"] * 47 + ["M"]
    assert [n for n, op in longest if op == "M"] == list(S.C2_LENGTHS) and [n for n, op in longest if op == "N"] == list(S.C2_INTRONS)
    placed = [l.split("\t") for l in texts[1].split("\n") if l and l[0] != "@"]
    located = {r["name"] for r in lifted}
    assert st["n_unlocated"] == 3 and len(placed[0][2]) > 500
    first, last = placed[0][0], placed[-1][0]
    assert (first.endswith("_x48"), last.endswith("_x48"), last in located) == \
        {"first": (True, False, True), "last": (False, True, True), "unlocated_last": (True, False, False)}[order]
    assert [i for i, f in enumerate(placed) if f[0] not in located][0] in (1, 2)             # records of no word between the others


# ---- C3

@pytest.mark.parametrize("n,layout,pair", S.c3_cases())
def test_c3_groups_on_the_block_seam(n, layout, pair):
    names = S.c3_names(n, layout, pair)
    _, lifted, st = combine(S.c3(n, layout, pair))
    assert st["n_transcript"] - st["n_unplaced"] == n and st["n_unplaced"] == (3 if n > 256 else 2)
    assert st["n_groups"] == S.C3_GROUPS[n, layout] == st["n_lifted"] and st["n_unlocated"] == 0
    # the record that goes out of every group, from the names alone: with flag 0 throughout the last one, else the head
    heads = [j for j in range(n) if j == 0 or names[j] != names[j - 1]]
    ends = [h - 1 for h in heads[1:]] + [n - 1]
    assert [xi(r) for r in lifted] == [h if h % 2 else e for h, e in zip(heads, ends)]
    assert ends[-1] == n - 1 and (n - 1 not in heads or n in (1, 256, 257))
    if n > 256:
        a, b = S.c3_pair(pair)
        j = 255 if layout == "single" else 254
        assert (names[j], names[j + 1]) == (a, b) and a != b
        assert {"last_byte": len(a) == len(b) and a[:-1] == b[:-1], "first_byte": len(a) == len(b) and a[1:] == b[1:],
                "prefix": b == a + "y" and a == "x", "long254": len(a) == len(b) == 254 and a[:253] == b[:253],
                "returns": n == 257 or names[j + (2 if layout == "single" else 5)] == a}[pair]
        if layout == "single":
            assert 255 in heads and 256 in heads and 257 in heads + [n]
        else:
            assert 255 in heads and not set(range(256, min(n, 259))) & set(heads)


# ---- C4

def test_c4_long_groups():
    _, lifted, st = combine(S.c4())
    assert st["n_groups"] == 7 and st["n_transcript"] == 7 * 600 and st["n_unlocated"] == 200 + 1
    got = {r["name"][2]: xi(r) for r in lifted}
    assert got == {v: e for v, e in S.C4_EXPECT.items() if isinstance(e, int)} and len(lifted) == 5
    assert st["n_groups_ambiguous"] == 1 and st["n_no_contig"] == 1
    for v, e in S.C4_EXPECT.items():                                         # and each variant alone
        _, one, st1 = combine(S.c4(variants=v))
        if isinstance(e, int):
            assert [xi(r) for r in one] == [e] and st1["n_groups_ambiguous"] + st1["n_no_contig"] == 0
        else:
            assert one == [] and st1[e] == 1 and st1["n_groups"] == 1


# ---- C5

def test_c5_reverse_complement():
    _, lifted, st = combine(S.c5())
    assert [xi(r) for r in lifted] == list(S.C5_LENGTHS) and st["n_strand_flipped"] == 10
    comp = str.maketrans("ACGT", "TGCA")                                     # every other code keeps its value
    for k, (n, r) in enumerate(zip(S.C5_LENGTHS, lifted)):
        src = S.c5_seq(n)
        assert len(src) == n and n not in range(4, 32)
        if n >= 32:
            assert src[:16] == J.SEQ16 and src[-16:] == J.SEQ16[::-1]
        else:
            assert src == J.SEQ16[:n][::-1]                                  # the backward cycle takes the whole read
        assert r["seq"] == (src[::-1].translate(comp) if n else "*") and r["flag"] == 16
        assert (r["qual"] == "*") == (n > 0 and k % 2 == 0) and (n > 0 or r["qual"] == "")
    assert [r["seq"] for r in lifted[1:4]] == ["=", "=T", "=TG"]           # of "=", "A=" and "CA="


# ---- C6

@pytest.mark.parametrize("kind", S.C6_KINDS)
def test_c6_nothing_to_do(kind):
    _, lifted, st = combine(S.c6(kind))
    assert lifted == [] and st["n_lifted"] == 0
    placed = st["n_transcript"] - st["n_unplaced"]
    assert (st["n_transcript"], placed, st["n_unlocated"], st["n_groups"]) == \
        {"no_record": (0, 0, 0, 0), "no_placed_record": (3, 0, 0, 0), "no_located_record": (303, 300, 300, 150)}[kind]


# ---- C7

def test_c7_many_workers():
    texts = S.c7()
    _, lifted, st = combine(texts)
    assert st["n_lifted"] == len(lifted) >= 8192 and st["n_transcript"] < S.C7_MAX_RECORDS
    names = [r["name"] for r in lifted]                                     # no group merged: one name twice, the one that returns
    assert sorted(n for n in set(names) if names.count(n) > 1) == ["s34_back"] and names.count("s34_back") == 2
    assert max(len(J.cigar_ops(r["cigar"])) for r in lifted) == 95 and st["n_groups_ambiguous"] == 1 and st["n_no_contig"] == 1
    assert max(len(r["name"]) for r in lifted) == 254
    assert {t: min(t, st["n_lifted"] // 4096 + 1) for t in (1, 2, 3, 8)} == {1: 1, 2: 2, 3: 3, 8: 3}
