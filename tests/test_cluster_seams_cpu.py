"""The inputs of tests/cluster_seams.py have the properties their names claim, shown with the plain restatement
tests/java_pileupclusters.py alone; tests/test_gpu_cluster_seams.py then holds ps_pileup_clusters to the restatement's bytes
on the same inputs.  The literals 56 (clusters per staged chunk of k_cl_sitefreq), 224 (records per chunk of k_qual_sd) and
64 (ranks, positions or lanes per block or step) are the kernels' own: test_kernel_constants reads them from the sources."""
import os
import re

import pytest

import cluster_seams as S
import java_pileupclusters as J

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "para-suite_amd", "csrc")


def lines(b):
    return b.decode().split("\n")[:-1]


def test_kernel_constants():
    """the seam tests are written for chunks of 7 * 32 = 224 records and 7 * 8 = 56 clusters"""
    found = {}
    for name in ("ps_clusters.hip", "ps_profile.hip"):
        text = open(os.path.join(CSRC, name)).read()
        found.update((k, int(v)) for k, v in re.findall(r"\b(kSdLoaders|kSdPer|kSfLoaders|kSfPer)\s*=\s*(\d+)", text))
    assert found == dict(kSdLoaders=7, kSdPer=32, kSfLoaders=7, kSfPer=8), "update the seam tests: %r" % found
    assert found["kSdLoaders"] * found["kSdPer"] == 224 and found["kSfLoaders"] * found["kSfPer"] == 56


# ---- A1

@pytest.mark.parametrize("n,place", S.A1_CASES)
def test_a1_ranks_and_chunks(n, place):
    f, st, info = J.cluster(S.a1_sam(n, place), S.REF, None, 1)
    assert st["n_crosslinked"] == n and st["n_clusters_written"] == n and st["n_ccr"] == n
    assert len(lines(f[".sitefrequency.tsv"])) == 65 and info["max_cap"] == 128          # a second block of 64 ranks
    sites = [int(l.split("\t")[7]) for l in lines(f[""])[1:]]
    assert max(sites) == 65 and sites.index(65) == {"first": 0, "middle": n // 2, "last": n - 1}[place]
    assert all(1 <= k <= 3 for k in sites if k != 65)                                    # most ranks: "no k-th fraction"
    if n > 1:                                                                            # the first cluster is the doubled one
        g, gst, _ = J.cluster(S.a1_sam(n, place, swap=True), S.REF, None, 1)
        assert gst["n_crosslinked"] == n and g[".sitefrequency.tsv"] != f[".sitefrequency.tsv"]
        assert lines(g[".sitefrequency.tsv"])[0] == lines(f[".sitefrequency.tsv"])[0]   # rank 0 is not doubled
    for c in range(56, n, 56):                                                           # the first cluster of a later chunk has a rank 1
        assert sites[c] >= 3


def test_a1_leading_clusters_not_crosslinked():
    n, place, lead = S.A1_LEAD
    f, st, _ = J.cluster(S.a1_sam(n, place, lead=lead), S.REF, None, 1)
    out = [l.split("\t") for l in lines(f[""])[1:]]
    assert len(out) == lead + n and st["n_crosslinked"] == n == 57 and lead == 56
    assert all(o[7] == "1" and float(o[8]) < 0.2 for o in out[:lead]) and all(float(o[8]) >= 0.2 for o in out[lead:])
    assert len(lines(f[".sitefrequency.tsv"])) == 65
    # the crosslinked clusters alone give the same ranks: the weak ones take no part
    alone, _, _ = J.cluster(S.a1_sam(n, place), S.REF, None, 1)
    assert alone[".sitefrequency.tsv"] == f[".sitefrequency.tsv"]


# ---- A2

def test_a2_windows_and_ties():
    f, st, info = J.cluster(S.A2_SAM, S.REF, S.A2_VCF, 1)
    out = [l.split("\t") for l in lines(f[""])[1:]]
    assert len(out) == len(S.A2_EXPECT) == 19
    assert [(int(o[2]), int(o[3]) - int(o[2]) + 1) for o in out] == [(lo, W) for _, lo, W, _ in S.A2_EXPECT]
    assert sorted({W for _, _, W, _ in S.A2_EXPECT}) == [64, 65, 128, 129]
    assert info["best_sites"] == [lo + win for _, lo, _, win in S.A2_EXPECT]
    assert info["max_cap"] == 16
    by_tag = {tag: (lo, win) for tag, lo, _, win in S.A2_EXPECT}
    # the bucket ties: offsets 63 and 64 in buckets 15 / 0 and 0 / 1; the first-insertion ties: 48 and 64 in one bucket
    lo = by_tag["tie_bucket_63"][0]
    assert (J.bucket(lo + 63, 16), J.bucket(lo + 64, 16)) == (15, 0)
    lo = by_tag["tie_bucket_64"][0]
    assert (J.bucket(lo + 63, 16), J.bucket(lo + 64, 16)) == (0, 1)
    for tag in ("tie_first_48", "tie_first_64"):
        lo = by_tag[tag][0]
        assert J.bucket(lo + 48, 16) == J.bucket(lo + 64, 16)
    assert info["ties_hashmap"] == 2              # tie_bucket_63 and tie_first_48: neither the largest nor the last inserted wins
    # the SNP: the site with the largest fraction is removed, the next one is the anchor
    assert st["n_snp_hits"] == 1
    snp = out[[t for t, _, _, _ in S.A2_EXPECT].index("snp_64")]
    assert snp[7] == "5" and snp[8] == J.jd(((2 / 3 + 1 / 2) + 1 / 3) + 1 / 3)      # five sites, four kept fractions
    no_vcf, _, i2 = J.cluster(S.A2_SAM, S.REF, None, 1)
    assert i2["best_sites"][-1] == by_tag["snp_64"][0] + 64 and no_vcf[""] != f[""]


# ---- A3

def test_a3_ninth_site_leaves_the_model():
    f8, st8, i8 = J.cluster(S.a3_sam(8), S.REF, None, 1)
    assert lines(f8[""])[1].split("\t")[7] == "8" and i8["max_cap"] == 16 and st8["n_order_unmodelled"] == 0
    assert len({J.bucket(S.A3_P + 16 * k, 16) for k in range(9)}) == 1
    with pytest.raises(J.FixtureError):
        J.cluster(S.a3_sam(9), S.REF, None, 1)
    with pytest.raises(J.FixtureError):
        J.cluster(S.a3_sam(9, after_plain=True), S.REF, S.A3_SNP_VCF, 1)
    assert all(S.A3_P + 16 * k - (S.A3_P - 3) < 64 for k in range(3))                    # the three known SNPs: first step of the window
    # after a 13-site cluster the table has 32 buckets and the nine sites fall into two of them
    assert sorted(J.bucket(S.A3_P + 16 * k, 32) for k in range(9)).count(J.bucket(S.A3_P, 32)) == 5
    for n in (8, 9):
        f, st, info = J.cluster(S.a3_sam(n, after_13=True), S.REF, None, 1)
        assert info["max_cap"] == 32 and [l.split("\t")[7] for l in lines(f[""])[1:]] == ["13", str(n)]


# ---- A4

def test_a4_sorted_input_never_desynchronises_the_rules():
    """on coordinate-sorted input the running maximum opens exactly where the Java's clusterEnd does"""
    res = S.sorted_rules_agree(6, 12, range(1, 7))
    assert res is not None and res[1] > 10000
    # the state walk against plain enumeration, for every sorted sequence of three records
    n = 0
    for a in range(12):
        for b in range(a, 12):
            for c in range(b, 12):
                for sa in range(1, 7):
                    for sb in range(1, 7):
                        for sc in range(1, 7):
                            recs = [("r", a, a + sa - 1), ("r", b, b + sb - 1), ("r", c, c + sc - 1)]
                            assert S.scan_opens(recs) == S.java_opens(recs)
                            n += 1
    assert n == 364 * 216
    # and the rules do differ once the order is broken: the example of the issue
    recs = [("r", 100, 140), ("r", 137, 137), ("r", 134, 136)]
    assert S.scan_opens(recs) == [True, True, False] and S.java_opens(recs) == [True, True, True]


def test_a4_out_of_order_stretches():
    scan, java = S.scan_opens(S.A4_SPANS), S.java_opens(S.A4_SPANS)
    differ = [i for i in range(len(scan)) if scan[i] != java[i]]
    assert len(differ) >= 10 and all(java[i] and not scan[i] for i in differ)
    refs = [r for r, _, _ in S.A4_SPANS]
    last_chrS = max(i for i, r in enumerate(refs) if r == "chrS")
    assert last_chrS in differ                                  # a stretch that ends at a reference change
    assert len(refs) - 1 in differ                              # a stretch that runs to the last record
    # two stretches back to back: a record that opens below the running maximum for both rules, inside a stretch
    starts = [i for i in range(1, len(scan)) if scan[i] and refs[i] == refs[i - 1] and S.A4_SPANS[i][2] < max(e for r, _, e in S.A4_SPANS[:i] if r == refs[i])]
    assert any(b > a and not any(scan[a + 1:b]) and any(i in differ for i in range(a + 1, b)) for a in starts for b in starts)
    unsorted = [i for i in range(1, len(refs)) if refs[i] == refs[i - 1] and S.A4_SPANS[i][1] < S.A4_SPANS[i - 1][1]]
    assert unsorted
    f, st, _ = J.cluster(S.a4_sam(), S.REF, None, 1)
    assert st["n_clusters"] == sum(java) and st["n_clusters_written"] == sum(java) - 1
    out = [l.split("\t") for l in lines(f[""])[1:]]
    assert ["50134", "50140"] in [o[2:4] for o in out]          # a member that starts before its opener raises the end
    assert st["n_ccr"] >= 5


# ---- A5

def test_a5_long_record_and_read_index_flags():
    f, st, info = J.cluster(S.A5_LONG_OK, S.REF, None, 1)
    assert len({J.bucket(p, 16) for p in S.A5_SITES}) == 1 and min(S.A5_SITES) - 1 < 32768 <= sorted(S.A5_SITES)[1] - 1
    # all three sites tie at 1/1 in one bucket: the last inserted, read index 40015, wins; a key that lost bit 15 of the
    # read index, or took it for a sign, would not change the order of 39999 and 40015 but would put 32751 last
    assert info["best_sites"] == [40016] and st["n_t2c_beyond_51"] == 3
    assert lines(f[""])[1].split("\t")[2:4] == ["1", "65535"]
    for text, msg in ((S.A5_LONG_BAD, None), (S.A5_PAST_END, "past the end"), (S.A5_NO_SEQ, "without SEQ")):
        if msg is None:                                         # the restatement has no 65,536 limit: the library's own
            assert J.cluster(text, S.REF, None, 1)[1]["n_kept"] == 2
        else:
            with pytest.raises(ValueError, match=msg):
                J.cluster(text, S.REF, None, 1)
    f, st, _ = J.cluster(S.A5_INDEX_50_51, S.REF, None, 1)
    assert st["n_t2c_beyond_51"] == 1 and lines(f[".sitepositions.tsv"]) == ["0.0"] * 50 + ["1.0"]
