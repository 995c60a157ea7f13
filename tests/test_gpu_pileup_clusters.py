"""ps_pileup_clusters on the GPU: all six files of PileupClusters.calculateReadPileups (PileupClusters.java:62-673) and the
stats, byte for byte equal to the plain-Python restatement tests/java_pileupclusters.py, from SAM and from sorted BAM."""
import gzip
import os
import struct

import numpy as np
import pytest

import java_pileupclusters as J
from test_pileup_clusters_cpu import CASES, FA, REF

pytestmark = pytest.mark.gpu


def _paths(out, site_prefix):
    return {k: out + k for k in J.OUT_FILES} | {k: site_prefix + k for k in J.SITE_FILES}


def _read(paths):
    return {k: open(p, "rb").read() for k, p in paths.items()}


def _check(mapping, fa, sam_text, ref, vcf_path, min_cov, out, site_prefix=None):
    """run the library and the restatement on the same records; return (stats, restatement info)"""
    import capi
    vcf = open(vcf_path, "rb").read() if vcf_path else None
    exp, est, info = J.cluster(sam_text, ref, vcf, min_cov)
    st = capi.ps_pileup_clusters(mapping, fa, out, vcf_path, min_cov, site_prefix)
    got = _read(_paths(out, site_prefix or mapping))
    for k in exp:
        assert got[k] == exp[k], (out, k, got[k][:2000], exp[k][:2000])
    assert st == est, (st, est)
    return st, info


_SAM_FLAGS = "MIDNSHP=X"


def bam_to_sam(path):
    """SAM text (header, and the fields the restatement reads) of a BAM file, in file order"""
    d = gzip.decompress(open(path, "rb").read())
    l_text = struct.unpack_from("<i", d, 4)[0]
    text = d[8:8 + l_text].rstrip(b"\0").decode()
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", d, at)[0]; at += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", d, at)[0]
        names.append(d[at + 4:at + 4 + ln - 1].decode()); at += 8 + ln
    out = [text if text.endswith("\n") or not text else text + "\n"]
    while at < len(d):
        bs, rid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", d, at + 0)
        p = at + 36
        name = d[p:p + l_name - 1].decode(); p += l_name
        cig = struct.unpack_from("<%dI" % n_cig, d, p); p += 4 * n_cig
        cigar = "".join("%d%s" % (c >> 4, _SAM_FLAGS[c & 15]) for c in cig) or "*"
        seq = "".join("=ACMGRSVTWYHKDBN"[(d[p + i // 2] >> (4 * (1 - i % 2))) & 15] for i in range(l_seq)) or "*"
        out.append("%s\t%d\t%s\t%d\t0\t%s\t*\t0\t0\t%s\t*\n" % (name, flag, names[rid] if rid >= 0 else "*", pos + 1, cigar, seq))
        at += 4 + bs
    return "".join(out)


@pytest.fixture(scope="module")
def hand(workdir):
    import capi
    d = os.path.join(workdir, "pc_hand")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "r.fa")
    open(fa, "w").write(FA)
    capi.ps_index(fa)
    return d, fa


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_cases(hand, name):
    import capi
    d, fa = hand
    text, vcf, mc = CASES[name]
    vcf_path = None
    if vcf:
        vcf_path = os.path.join(d, name + ".vcf")
        open(vcf_path, "wb").write(vcf)
    sam = os.path.join(d, name + ".sam")
    open(sam, "w").write(text)
    bam = os.path.join(d, name + ".bam")
    capi.ps_sam_to_bam(sam, bam, 0, True, False, 4)
    key = lambda t: [[f[i] for i in (0, 1, 2, 3, 5, 9)] for f in (l.split("\t") for l in t.split("\n") if l and l[0] != "@")]
    assert key(bam_to_sam(bam)) == key(text)                                # the hand-built records are sorted already
    for m in sorted({mc, 0, 2}):
        st_sam, _ = _check(sam, fa, text, REF, vcf_path, m, os.path.join(d, "%s_s%d" % (name, m)), os.path.join(d, "%s_s%d" % (name, m)))
        st_bam, _ = _check(bam, fa, text, REF, vcf_path, m, os.path.join(d, "%s_b%d" % (name, m)), os.path.join(d, "%s_b%d" % (name, m)))
        assert st_sam == st_bam
    # site_prefix None: next to the mapping file
    capi.ps_pileup_clusters(sam, fa, os.path.join(d, name + "_default"), vcf_path, mc)
    for k in J.SITE_FILES:
        assert open(sam + k, "rb").read() == open(os.path.join(d, "%s_s%d%s" % (name, mc, k)), "rb").read()


# ---- end to end: clustered PAR-CLIP reads, mapped and sorted by the library

def clustered_reads(contigs, n_loci, reads_per_locus, seed, read_len=(50, 50)):
    """PAR-CLIP-like loci: per locus a transcript strand, up to 4 T->C sites converted with SITE_FREQ[k], 2-10 (or given)
    reads of which about one in six comes from the other strand, sequencing errors from EXAMPLE_PROFILE.  Returns FASTQ text
    and the sites (contig, 1-based position) of every locus."""
    import simulate as S
    rng = np.random.default_rng(seed)
    codes = [S.contig_codes(asc) for _, asc in contigs]
    prof = np.cumsum(S.EXAMPLE_PROFILE, axis=1)
    fq, sites, n = [], [], 0
    lo_len, hi_len = read_len
    while len(sites) < n_loci:
        ci = int(rng.integers(len(contigs)))
        cc = codes[ci]
        a = int(rng.integers(12000, cc.size - 400))
        span = int(rng.integers(60, 120))
        if (cc[a:a + span + hi_len] > 3).any():
            continue
        strand = int(rng.integers(2))
        tgt = 3 if strand == 0 else 0                                       # reference T (forward) or A (reverse)
        cand = np.flatnonzero(cc[a + 10:a + span - 10] == tgt) + a + 10
        k_sites = min(cand.size, int(rng.integers(0, 5)))
        chosen = rng.choice(cand, size=k_sites, replace=False) if k_sites else np.array([], dtype=np.int64)
        sites.append([(contigs[ci][0], int(p) + 1) for p in chosen])
        lo_r, hi_r = reads_per_locus
        for _ in range(int(rng.integers(lo_r, hi_r + 1))):
            L = int(rng.integers(lo_len, hi_len + 1))
            s = a + int(rng.integers(0, max(1, span - L // 2)))
            rs = strand if rng.random() > 1 / 6 else 1 - strand
            seg = cc[s:s + L].copy()
            seg = (prof[seg] < rng.random(L)[:, None]).sum(axis=1).clip(0, 3).astype(np.uint8)
            for k, p in enumerate(chosen):
                if s <= p < s + L and rs == strand and rng.random() < S.SITE_FREQ[k]:
                    seg[p - s] = 1 if strand == 0 else 2                    # C on the forward strand, G (read C) on the reverse
            txt = "".join("ACGT"[b] for b in seg)
            if rs == 1:
                txt = txt[::-1].translate(str.maketrans("ACGT", "TGCA"))
            fq.append("@r%d\n%s\n+\n%s\n" % (n, txt, "I" * L))
            n += 1
    return "".join(fq), sites


def _vcf(rows):
    """VCF text of (CHROM, POS, REF, ALT) rows"""
    body = "".join("%s\t%d\t.\t%s\t%s\t50\tPASS\t.\n" % r for r in sorted(rows))
    return ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + body).encode()


def _snp_rows(sites, rng):
    """about a fifth of the true sites as T>C (CHROM without "chr"), and distractors: the next position, a first ALT that is
    not C, another REF, a symbolic ALT"""
    rows = []
    for c, p in sorted({x for ss in sites for x in ss}):
        c, u = c[3:], rng.random()
        rows.append((c, p, "T", "C") if u < 0.2 else (c, p + 1, "T", "C") if u < 0.3 else (c, p, "T", "A,C") if u < 0.4 else
                    (c, p, "G", "C") if u < 0.5 else (c, p, "T", "<CNV>") if u < 0.55 else (c, p, "TT", "CT") if u < 0.6 else None)
    return [r for r in rows if r]


def _map_sorted(fa, fq_text, prefix):
    import capi
    fq = prefix + ".fq"
    open(fq, "w").write(fq_text)
    bam = prefix + ".bam"
    capi.ps_map_to_bam(8, "0.04", None, None, fa, fq, bam, min_mapq=0, sort_by_coordinate=True, write_index=False)
    return bam


def test_end_to_end_example_genome(example, workdir):
    import __graft_entry__ as ge
    import capi
    mod = ge.load_package()
    fa = example["fa"]
    if not all(os.path.exists(fa + e) for e in (".bwt", ".sa", ".pac", ".ann")):
        capi.ps_index(fa)
    ref = J.read_fasta(fa)
    fq, sites = clustered_reads(example["genome"], 3000, (2, 10), seed=4711)
    prefix = os.path.join(workdir, "pc_e2e")
    bam = _map_sorted(fa, fq, prefix)
    text = bam_to_sam(bam)
    rng = np.random.default_rng(9)
    vcf_plain = prefix + ".vcf"
    open(vcf_plain, "wb").write(_vcf(_snp_rows(sites, rng)))
    vcf_gz = prefix + ".vcf.gz"
    open(vcf_gz, "wb").write(gzip.compress(open(vcf_plain, "rb").read()))
    st, info = _check(bam, fa, text, ref, vcf_plain, 1, prefix + "_p.clusters", prefix + "_p")
    print("e2e stats", st, "ties", info["ties_hashmap"], "max cap", info["max_cap"])
    assert info["ties_hashmap"] >= 20
    assert st["n_crosslinked"] >= 10 and st["n_double_stranded"] > 0 and st["n_snp_hits"] > 0 and st["n_ccr"] > 0
    assert st["n_order_unmodelled"] == 0 and st["n_ccr_clipped"] == 0
    st_gz, _ = _check(bam, fa, text, ref, vcf_gz, 1, prefix + "_g.clusters", prefix + "_g")
    assert st_gz == st
    got_p = _read(_paths(prefix + "_p.clusters", prefix + "_p"))
    assert _read(_paths(prefix + "_g.clusters", prefix + "_g")) == got_p
    # a second call writes the same bytes; the mirror class writes them next to the mapping
    capi.ps_pileup_clusters(bam, fa, prefix + "_p2.clusters", vcf_plain, 1, prefix + "_p2")
    assert _read(_paths(prefix + "_p2.clusters", prefix + "_p2")) == got_p
    st_m = mod.mapping.PileupClusters().calculateReadPileups(bam, fa, prefix + "_m.clusters", vcf_plain, 1)
    assert st_m == st
    assert _read(_paths(prefix + "_m.clusters", bam)) == got_p


def test_deep_clusters(mid, workdir):
    import capi
    fa = mid["fa"]
    if not all(os.path.exists(fa + e) for e in (".bwt", ".sa", ".pac", ".ann")):
        capi.ps_index(fa)
    ref = J.read_fasta(fa)
    fq, sites = clustered_reads(mid["genome"], 100, (200, 1000), seed=815)
    prefix = os.path.join(workdir, "pc_deep")
    bam = _map_sorted(fa, fq, prefix)
    text = bam_to_sam(bam)
    vcf = prefix + ".vcf"
    open(vcf, "wb").write(_vcf(_snp_rows(sites, np.random.default_rng(3))))
    st, info = _check(bam, fa, text, ref, vcf, 5, prefix + ".clusters", prefix)
    print("deep stats", st, "max cap", info["max_cap"])
    assert info["max_cap"] >= 64 and st["n_crosslinked"] > 0


def ragged_sam(seed):
    """60 loci of 20-60 reads of 36-75 bases on a 20 kbp contig, both strands, T->C at 8 % of the transcript's T (so some
    at read index >= 51), one in ten reads with a deleted base, one in twenty soft-clipped; sorted SAM text and the contig"""
    import random
    rng = random.Random(seed)
    contig = "".join(rng.choice("ACGT") for _ in range(20000))
    recs = []
    for locus in range(60):
        a = 300 + locus * 320 + rng.randrange(0, 100)
        for _ in range(rng.randint(20, 60)):
            L = rng.randint(36, 75)
            pos = a + rng.randrange(0, 60)
            seq = list(contig[pos - 1:pos - 1 + L])
            rev = rng.random() < 0.4
            for i in range(L):
                if rev and seq[i] == "A" and rng.random() < 0.08:
                    seq[i] = "G"
                elif not rev and seq[i] == "T" and rng.random() < 0.08:
                    seq[i] = "C"
            cig = "%dM" % L
            if rng.random() < 0.1:                                          # one deleted reference base
                c = rng.randint(3, L - 4)
                seq = seq[:c] + list(contig[pos - 1 + c + 1:pos - 1 + L + 1])[:L - c]
                cig = "%dM1D%dM" % (c, L - c)
            elif rng.random() < 0.05:                                       # soft clip
                seq = ["A", "A"] + seq[:L - 2]
                cig = "2S%dM" % (L - 2)
            recs.append((pos, "g%d\t%d\tchrR\t%d\t37\t%s\t*\t0\t0\t%s\t*\n" % (len(recs), 16 if rev else 0, pos, cig, "".join(seq))))
    recs.sort(key=lambda x: x[0])
    return "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrR\tLN:20000\n" + "".join(l for _, l in recs), contig


def test_ragged_reads(workdir):
    import capi
    d = os.path.join(workdir, "pc_ragged")
    os.makedirs(d, exist_ok=True)
    text, contig = ragged_sam(5150)
    fa = os.path.join(d, "g.fa")
    open(fa, "w").write(">chrR\n" + contig + "\n")
    capi.ps_index(fa)
    sam = os.path.join(d, "m.sam")
    open(sam, "w").write(text)
    st, _ = _check(sam, fa, text, {"chrR": contig.encode()}, None, 3, os.path.join(d, "out"), os.path.join(d, "out"))
    assert st["n_t2c_beyond_51"] > 0 and st["n_crosslinked"] > 0


def test_errors_write_nothing(hand):
    import capi
    d, fa = hand
    text = CASES["basic"][0]
    uns = os.path.join(d, "err_unsorted.sam")
    open(uns, "w").write(text.replace("SO:coordinate", "SO:unsorted"))
    with pytest.raises(capi.PsError, match="SO:unsorted"):
        capi.ps_pileup_clusters(uns, fa, os.path.join(d, "err_u.out"), None, 1, os.path.join(d, "err_u"))
    unk = os.path.join(d, "err_contig.sam")
    open(unk, "w").write(text.replace("@SQ\tSN:c2", "@SQ\tSN:c9").replace("\tchr1\t80\t", "\tc9\t80\t"))
    with pytest.raises(capi.PsError, match="reference"):
        capi.ps_pileup_clusters(unk, fa, os.path.join(d, "err_c.out"), None, 1, os.path.join(d, "err_c"))
    assert not [f for f in os.listdir(d) if f.startswith("err_") and not f.endswith(".sam")]


def test_a_failure_on_the_fourth_file_leaves_none(hand):
    """<out>.report is taken by a directory: the call fails after every count was taken, and none of the other five files is left"""
    import capi
    d, fa = hand
    sam, out, sp = (os.path.join(d, n) for n in ("late.sam", "late.out", "late_sites"))
    open(sam, "w").write(CASES["basic"][0])
    os.mkdir(out + ".report")
    with pytest.raises(capi.PsError, match="cannot rename"):
        capi.ps_pileup_clusters(sam, fa, out, None, 1, sp)
    assert sorted(f for f in os.listdir(d) if f.startswith("late")) == ["late.out.report", "late.sam"]
    assert os.path.isdir(out + ".report") and os.listdir(out + ".report") == []
    os.rmdir(out + ".report")
    capi.ps_pileup_clusters(sam, fa, out, None, 1, sp)                      # and with the name free, all six, no temporary
    assert sorted(f for f in os.listdir(d) if f.startswith("late")) == sorted(["late.sam"] + [os.path.basename(p) for p in _paths(out, sp).values()])
    with pytest.raises(capi.PsError, match="would overwrite the input"):
        capi.ps_pileup_clusters(sam, fa, sam, None, 1, sp)
    assert open(sam).read() == CASES["basic"][0]
