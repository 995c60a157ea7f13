"""ps_error_profile_full on the GPU: all six files of ErrorProfiling.inferErrorProfile (ErrorProfiling.java:100-631), byte for
byte equal to the plain-Python restatement tests/java_errorprofile.py, from SAM and from BAM, in each file's own order."""
import os
import random

import pytest

import java_errorprofile as J
from test_error_profile_full_cpu import FA, ML, ORDER_SEED, RECORDS, order_records, sam_text

pytestmark = pytest.mark.gpu


def _read(prefix):
    return {k: open(prefix + k, "rb").read() for k in J.FILES}


def _index(path, text):
    import capi
    open(path, "w").write(text)
    capi.ps_index(path)
    return J.read_fasta(path)


def test_hand_built_records(workdir):
    import capi
    d = os.path.join(workdir, "epf_hand")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "r.fa")
    ref = _index(fa, FA)
    sam = os.path.join(d, "m.sam")
    open(sam, "w").write(sam_text(RECORDS))
    for iq in (False, True):
        exp, est = J.infer(sam_text(RECORDS), ref, ML, iq)
        out = os.path.join(d, "q%d" % iq)
        st = capi.ps_error_profile_full(sam, fa, ML, out, iq)
        got = _read(out)
        for k in J.FILES:
            assert got[k] == exp[k], (iq, k, got[k], exp[k])
        assert st == est
        assert st["n_without_qual"] == 1 and st["n_qual_beyond_read"] == 2 and st["n_indel_reads"] == 3
    assert open(os.path.join(d, "q0.qualities"), "rb").read() == b""
    # the mapper's two files are the bytes ps_error_profile writes; out_prefix None: the mapping file's name
    capi.ps_error_profile(sam, fa, ML, os.path.join(d, "plain"))
    for k in (".errorprofile", ".indelprofile"):
        assert open(os.path.join(d, "plain" + k), "rb").read() == open(os.path.join(d, "q1" + k), "rb").read()
    capi.ps_error_profile_full(sam, fa, ML, None, True)
    assert _read(sam) == _read(os.path.join(d, "q1"))


def _bam_order(sam_path):
    """the records of a SAM file in the order of ps_sam_to_bam's coordinate sort (stable; no reference last)"""
    text = open(sam_path).read().split("\n")
    hdr = [l for l in text if l.startswith("@")]
    recs = [l for l in text if l and not l.startswith("@")]
    sq = {l.split("\t")[1][3:]: i for i, l in enumerate(l for l in hdr if l.startswith("@SQ"))}
    key = lambda l: (sq.get(l.split("\t")[2], 1 << 32), int(l.split("\t")[3]) - 1)
    return "\n".join(hdr) + "\n" + "".join(l + "\n" for l in sorted(recs, key=key))


def test_first_pass_sam_bam_and_mirror(mid, workdir):
    import __graft_entry__ as ge
    import capi
    import simulate as S
    mod = ge.load_package()
    sim = S.simulate_reads(mid["genome"], n_reads=50000, read_len=50, seed=93, indel_scale=400, n_frac=0.002)
    fq = os.path.join(workdir, "epf.fq")
    S.write_fastq(fq, sim)
    fa = mid["fa"]
    first = os.path.join(workdir, "epf_first")
    mod.mapping.BWAMapping().executeMapping(8, fa, fq, first, 10, "2")
    sam = first + ".sam"
    recs = [l for l in open(sam).read().split("\n") if l and not l.startswith("@")]
    gapped_rev = sum(1 for l in recs if ("I" in l.split("\t")[5] or "D" in l.split("\t")[5]) and int(l.split("\t")[1]) & 16)
    gapped_fwd = sum(1 for l in recs if ("I" in l.split("\t")[5] or "D" in l.split("\t")[5]) and not int(l.split("\t")[1]) & 16)
    assert gapped_rev > 10 and gapped_fwd > 10
    ref = J.read_fasta(fa)
    exp_sam, st_sam = J.infer(open(sam).read(), ref, 101, True)
    st = capi.ps_error_profile_full(sam, fa, 101, os.path.join(workdir, "epf_sam"), True)
    got_sam = _read(os.path.join(workdir, "epf_sam"))
    assert got_sam == exp_sam and st == st_sam
    capi.ps_sam_to_bam(sam, first + ".bam", 0, True, True, 8)
    st_bam = capi.ps_error_profile_full(first + ".bam", fa, 101, os.path.join(workdir, "epf_bam"), True)
    got_bam = _read(os.path.join(workdir, "epf_bam"))
    for k in (".errorprofile", ".indelprofile", ".errorprofile.vcf", ".qualityPerMismatch", ".indels"):
        assert got_bam[k] == got_sam[k], k
    exp_bam, _ = J.infer(_bam_order(sam), ref, 101, True)
    assert got_bam[".qualities"] == exp_bam[".qualities"]
    assert st_bam == st
    capi.ps_error_profile(sam, fa, 101, os.path.join(workdir, "epf_plain"))
    for k in (".errorprofile", ".indelprofile"):
        assert open(os.path.join(workdir, "epf_plain" + k), "rb").read() == got_sam[k]
    ep, ip = mod.mapping.ErrorProfiling(sam, fa, 101).inferErrorProfile(True, False)
    assert (ep, ip) == (sam + ".errorprofile", sam + ".indelprofile")
    assert _read(sam) == exp_sam


def test_file_order_is_honoured(workdir):
    import capi
    d = os.path.join(workdir, "epf_order")
    os.makedirs(d, exist_ok=True)
    contig, a, b = order_records(ORDER_SEED)
    fa = os.path.join(d, "s.fa")
    ref = _index(fa, ">s1\n" + contig + "\n")
    hdr = "@SQ\tSN:s1\tLN:400\n"
    quals = []
    for name, recs in (("a", a), ("b", b)):
        sam = os.path.join(d, name + ".sam")
        open(sam, "w").write(sam_text(recs, hdr))
        exp, _ = J.infer(sam_text(recs, hdr), ref, 40, True)
        capi.ps_error_profile_full(sam, fa, 40, os.path.join(d, name), True)
        got = _read(os.path.join(d, name))
        assert got == exp, name
        quals.append(got[".qualities"])
    assert quals[0] != quals[1]                   # a histogram or a reordered sum cannot give both


def test_ragged_reads_and_too_long(workdir):
    import capi
    d = os.path.join(workdir, "epf_ragged")
    os.makedirs(d, exist_ok=True)
    rng = random.Random(4242)
    contig = "".join(rng.choice("ACGT") for _ in range(2000))
    fa = os.path.join(d, "g.fa")
    ref = _index(fa, ">g1\n" + contig + "\n")
    recs = []
    for r in range(3000):
        L = rng.randint(18, 75)
        pos = rng.randrange(1, 2000 - 80)
        seq = list(contig[pos - 1:pos - 1 + L])
        for _ in range(rng.randint(0, 3)):
            seq[rng.randrange(L)] = rng.choice("ACGTN")
        cig = "%dM" % L
        kind = rng.random()
        if kind < 0.1:                                               # one inserted base
            c = rng.randint(3, L - 4)
            seq = seq[:c] + [rng.choice("ACGT")] + seq[c:L - 1]
            cig = "%dM1I%dM" % (c, L - 1 - c)
        elif kind < 0.2:                                             # one deleted reference base
            c = rng.randint(3, L - 4)
            seq = seq[:c] + list(contig[pos - 1 + c + 1:pos - 1 + L + 1])[:L - c]
            cig = "%dM1D%dM" % (c, L - c)
        qual = "*" if rng.random() < 0.02 else "".join(chr(33 + rng.randint(2, 41)) for _ in range(len(seq)))
        recs.append(("g%d" % r, 16 if rng.random() < 0.5 else 0, "g1", pos, cig, "".join(seq), qual))
    hdr = "@SQ\tSN:g1\tLN:2000\n"
    sam = os.path.join(d, "m.sam")
    open(sam, "w").write(sam_text(recs, hdr))
    exp, est = J.infer(sam_text(recs, hdr), ref, 250, True)
    st = capi.ps_error_profile_full(sam, fa, 250, os.path.join(d, "ok"), True)
    assert _read(os.path.join(d, "ok")) == exp and st == est
    # one record longer than max_read_len: the error of ps_error_profile, and no file of either call
    long_sam = os.path.join(d, "long.sam")
    open(long_sam, "w").write(sam_text(recs + [("big", 0, "g1", 1, "300M", contig[:300], "I" * 300)], hdr))
    with pytest.raises(capi.PsError) as e1:
        capi.ps_error_profile(long_sam, fa, 250, os.path.join(d, "long_plain"))
    with pytest.raises(capi.PsError) as e2:
        capi.ps_error_profile_full(long_sam, fa, 250, os.path.join(d, "long_full"), True)
    assert str(e1.value) == str(e2.value)
    assert not [f for f in os.listdir(d) if f.startswith("long_")]


def test_a_failure_on_the_last_file_leaves_none(workdir):
    """<prefix>.qualities is taken by a directory: the call fails after every count was taken and none of the six files is left"""
    import capi
    d = os.path.join(workdir, "epf_late")
    os.makedirs(d, exist_ok=True)
    fa, sam, out = (os.path.join(d, n) for n in ("r.fa", "m.sam", "late"))
    _index(fa, FA)
    open(sam, "w").write(sam_text(RECORDS))
    os.mkdir(out + ".qualities")
    with pytest.raises(capi.PsError, match="cannot rename"):
        capi.ps_error_profile_full(sam, fa, ML, out, True)
    assert [f for f in os.listdir(d) if f.startswith("late")] == ["late.qualities"] and os.listdir(out + ".qualities") == []
    os.rmdir(out + ".qualities")
    capi.ps_error_profile_full(sam, fa, ML, out, True)                       # and with the name free, all six, no temporary
    assert sorted(f for f in os.listdir(d) if f.startswith("late")) == sorted("late" + k for k in J.FILES)
    named = os.path.join(d, "named.errorprofile")                            # a mapping under the name the profile would get
    open(named, "w").write(sam_text(RECORDS))
    for call in (capi.ps_error_profile, capi.ps_error_profile_full):
        with pytest.raises(capi.PsError, match="would overwrite the input"):
            call(named, fa, ML, named[:-len(".errorprofile")])
    assert open(named).read() == sam_text(RECORDS) and [f for f in os.listdir(d) if f.startswith("named")] == ["named.errorprofile"]
