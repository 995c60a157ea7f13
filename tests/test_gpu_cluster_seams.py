"""ps_pileup_clusters on the seams of its own layout: the inputs of tests/cluster_seams.py (what each one reaches is shown in
tests/test_cluster_seams_cpu.py), all six files and the stats byte for byte equal to the plain-Python restatement
tests/java_pileupclusters.py, from SAM and from ps_sam_to_bam's BAM."""
import os

import pytest

import cluster_seams as S
from test_gpu_pileup_clusters import _check, bam_to_sam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seams(workdir):
    import capi
    d = os.path.join(workdir, "cl_seams")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "r.fa")
    open(fa, "w").write(S.FA)
    capi.ps_index(fa)
    return d, fa


def _key(text):
    return [[f[i] for i in (0, 1, 2, 3, 5, 9)] for f in (l.split("\t") for l in text.split("\n") if l and l[0] != "@")]


def _both(seams, name, text, vcf=None, min_cov=1):
    """the restatement against the library on the SAM text and on its BAM; returns the stats"""
    import capi
    d, fa = seams
    vcf_path = None
    if vcf:
        vcf_path = os.path.join(d, name + ".vcf")
        open(vcf_path, "wb").write(vcf)
    sam, bam = os.path.join(d, name + ".sam"), os.path.join(d, name + ".bam")
    open(sam, "w").write(text)
    st_sam, info = _check(sam, fa, text, S.REF, vcf_path, min_cov, os.path.join(d, name + "_s"), os.path.join(d, name + "_s"))
    capi.ps_sam_to_bam(sam, bam, 0, True, False, 4)
    assert _key(bam_to_sam(bam)) == _key(text)                               # sorted already: the sort keeps the order
    st_bam, _ = _check(bam, fa, text, S.REF, vcf_path, min_cov, os.path.join(d, name + "_b"), os.path.join(d, name + "_b"))
    assert st_sam == st_bam
    return st_sam, info


# ---- A1

@pytest.mark.parametrize("n,place", S.A1_CASES)
def test_a1_ranks_and_chunks(seams, n, place):
    st, info = _both(seams, "a1_%d_%s" % (n, place), S.a1_sam(n, place))
    assert st["n_crosslinked"] == n and info["max_cap"] == 128 and st["n_order_unmodelled"] == 0


def test_a1_swapped_first_cluster(seams):
    """the doubled cluster is the first crosslinked one of the file, not the first of a chunk"""
    for n in (57, 113):
        _both(seams, "a1_%d_swap" % n, S.a1_sam(n, "middle", swap=True))


def test_a1_leading_clusters_not_crosslinked(seams):
    n, place, lead = S.A1_LEAD
    st, _ = _both(seams, "a1_lead", S.a1_sam(n, place, lead=lead))
    assert st["n_crosslinked"] == n and st["n_clusters_written"] == n + lead


# ---- A2

def test_a2_windows_and_ties(seams):
    st, info = _both(seams, "a2", S.A2_SAM, S.A2_VCF)
    assert info["best_sites"] == [lo + win for _, lo, _, win in S.A2_EXPECT] and st["n_snp_hits"] == 1
    _both(seams, "a2_no_vcf", S.A2_SAM)                                       # offset 64 kept: the anchor of the last cluster moves


# ---- A3

def _a3_nine(seams, name, text, vcf, n_clusters):
    """nine sites in one of 16 buckets: the restatement refuses (test_cluster_seams_cpu), the library counts the cluster"""
    import capi
    d, fa = seams
    sam, out = os.path.join(d, name + ".sam"), os.path.join(d, name + "_s")
    open(sam, "w").write(text)
    vcf_path = None
    if vcf:
        vcf_path = os.path.join(d, name + ".vcf")
        open(vcf_path, "wb").write(vcf)
    st = capi.ps_pileup_clusters(sam, fa, out, vcf_path, 1, out)
    print("n_order_unmodelled", name, st["n_order_unmodelled"])
    assert st["n_order_unmodelled"] == 1
    assert (st["n_clusters"], st["n_kept"], st["n_clusters_written"]) == (n_clusters, n_clusters, n_clusters - 1)
    line = open(out, "rb").read().decode().split("\n")[n_clusters - 1].split("\t")
    assert line[2:4] == [str(S.A3_P - 3), str(S.A3_P + 136)] and line[5:8] == ["1", "9", "9"]
    return st


def test_a3_unmodelled_bucket_with_known_snps(seams):
    """the sites of a bucket count, known SNP or not: three of the nine are removed from the fractions in the first step of
    the window, so from there on the kept fractions are compacted at another offset than the sites' buckets"""
    st = _a3_nine(seams, "a3_9_snp", S.a3_sam(9, after_plain=True), S.A3_SNP_VCF, 3)
    assert st["n_snp_hits"] == 3


def test_a3_the_unmodelled_bucket(seams):
    st8, _ = _both(seams, "a3_8", S.a3_sam(8))
    assert st8["n_order_unmodelled"] == 0
    _a3_nine(seams, "a3_9", S.a3_sam(9), None, 2)
    # after a 13-site cluster the table has 32 buckets, and the same nine sites are modelled again
    for n in (8, 9):
        st, info = _both(seams, "a3_13_%d" % n, S.a3_sam(n, after_13=True))
        print("n_order_unmodelled a3_13_%d" % n, st["n_order_unmodelled"])
        assert st["n_order_unmodelled"] == 0 and info["max_cap"] == 32


# ---- A4

def test_a4_out_of_order_stretches(seams):
    """locally out-of-order records under an SO:coordinate header: the library opens clusters where the Java would
    (k_cl_fix walks each stretch).  SAM only: ps_sam_to_bam would sort the records."""
    d, fa = seams
    text = S.a4_sam()
    sam = os.path.join(d, "a4.sam")
    open(sam, "w").write(text)
    st, _ = _check(sam, fa, text, S.REF, None, 1, os.path.join(d, "a4_s"), os.path.join(d, "a4_s"))
    assert st["n_clusters"] == sum(S.java_opens(S.A4_SPANS)) > sum(S.scan_opens(S.A4_SPANS))
    _check(sam, fa, text, S.REF, None, 2, os.path.join(d, "a4_s2"), os.path.join(d, "a4_s2"))


# ---- A5

def test_a5_65535_aligned_bases(seams):
    st, info = _both(seams, "a5_long", S.A5_LONG_OK)
    assert info["best_sites"] == [40016] and st["n_t2c_beyond_51"] == 3


def test_a5_read_indices_50_and_51(seams):
    d, _ = seams
    st, _ = _both(seams, "a5_idx", S.A5_INDEX_50_51)
    assert st["n_t2c_beyond_51"] == 1
    assert open(os.path.join(d, "a5_idx_s.sitepositions.tsv")).read().split("\n")[50] == "1.0"


@pytest.mark.parametrize("name,text,msg", [("long", S.A5_LONG_BAD, "65536 bases or more"), ("past", S.A5_PAST_END, "past the end"),
                                           ("noseq", S.A5_NO_SEQ, "no SEQ")], ids=["long", "past", "noseq"])
def test_a5_errors_write_nothing(seams, name, text, msg):
    import capi
    d, fa = seams
    sam = os.path.join(d, "err5_%s.sam" % name)
    open(sam, "w").write(text)
    with pytest.raises(capi.PsError, match=msg):
        capi.ps_pileup_clusters(sam, fa, os.path.join(d, "err5_%s.out" % name), None, 1, os.path.join(d, "err5_%s" % name))
    assert [f for f in os.listdir(d) if f.startswith("err5_%s" % name)] == ["err5_%s.sam" % name]
