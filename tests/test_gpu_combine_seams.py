"""ps_combine_genome_transcript on the seams of its own layout: the inputs of tests/combine_seams.py (what each one reaches is
shown in tests/test_combine_seams_cpu.py), record for record and counter for counter what the plain-Python restatement
tests/java_combine.py gives, from SAM and from ps_sam_to_bam's BAM, and the same bytes whatever the number of threads."""
import gzip
import os

import pytest

import combine_seams as S
import java_combine as J
from test_gpu_combine import _check_index, _stats_equal, _write

pytestmark = pytest.mark.gpu


def inflated(path):
    return gzip.decompress(open(path, "rb").read())


def _both(d, texts, from_bam=False, name="c", **kw):
    """the library on a section's two files against the restatement on their text; returns (output file, stats, records)"""
    import capi
    from test_bam import read_bam
    d = str(d)
    g, t, out = _write(os.path.join(d, name + "_g.sam"), texts[0]), _write(os.path.join(d, name + "_t.sam"), texts[1]), os.path.join(d, name + ".bam")
    exp_text, exp_refs, exp, exp_st = J.combine(J.parse_sam(texts[0]), J.parse_sam(texts[1]))
    if from_bam:
        for p in (g, t):
            capi.ps_sam_to_bam(p, p[:-3] + "bam")
        g, t = g[:-3] + "bam", t[:-3] + "bam"
    st = capi.ps_combine_genome_transcript(g, t, out, **kw)
    text, refs, recs, _ = read_bam(out)
    assert text == exp_text and refs == exp_refs
    assert J.same_records(recs, exp) is None, J.same_records(recs, exp)
    _stats_equal(st, exp_st, out)
    return out, st, recs


def _same_bytes_for_any_threads(d, texts, name):
    one, _, _ = _both(d, texts, name=name + "_1", threads=1)
    three, _, _ = _both(d, texts, name=name + "_3", threads=3)
    assert inflated(one) == inflated(three)


def test_c1_every_phase_of_the_walk(tmp_path):
    _, st, _ = _both(tmp_path, S.c1())
    assert st["n_missed_indel_splice"] > 0 and st["n_unlocated"] > 0 and st["n_spliced"] > 0 and st["n_lifted"] > 4096


@pytest.mark.parametrize("from_bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("strand", ["1", "-1"])
@pytest.mark.parametrize("order", S.C2_ORDERS)
def test_c2_long_words(tmp_path, order, strand, from_bam):
    _, st, recs = _both(tmp_path, S.c2(order, strand), from_bam)
    assert max(len(J.cigar_ops(r["cigar"])) for r in recs) == 95 and st["n_unlocated"] == 3


@pytest.mark.parametrize("from_bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("n", S.C3_N)
def test_c3_groups_on_the_block_seam(tmp_path, n, from_bam):
    for i, case in enumerate(c for c in S.c3_cases() if c[0] == n):
        _, st, _ = _both(tmp_path, S.c3(*case), from_bam, name="c3_%d" % i)
        assert st["n_groups"] == S.C3_GROUPS[case[:2]] == st["n_lifted"], case
        if not from_bam:
            _same_bytes_for_any_threads(tmp_path, S.c3(*case), "c3t_%d" % i)


@pytest.mark.parametrize("from_bam", [False, True], ids=["sam", "bam"])
def test_c4_long_groups(tmp_path, from_bam):
    _, st, _ = _both(tmp_path, S.c4(), from_bam)
    assert (st["n_groups"], st["n_lifted"], st["n_groups_ambiguous"], st["n_no_contig"]) == (7, 5, 1, 1)
    for v in S.C4_VARIANTS:                                                   # each group alone: its head in lane 0, its end at n - 1
        _both(tmp_path, S.c4(variants=v), from_bam, name="c4" + v)
    if not from_bam:
        _same_bytes_for_any_threads(tmp_path, S.c4(), "c4t")


def test_c5_reverse_complement(tmp_path):
    _, st, _ = _both(tmp_path, S.c5())
    assert st["n_strand_flipped"] == len(S.C5_LENGTHS)


@pytest.mark.parametrize("kind", S.C6_KINDS)
def test_c6_nothing_to_do(tmp_path, kind):
    texts = S.c6(kind)
    _, st, recs = _both(tmp_path, texts, name="c6")
    assert st["n_lifted"] == 0 and J.same_records(recs, J.parse_sam(texts[0])[2]) is None      # the genomic records alone
    assert sorted(os.listdir(str(tmp_path))) == ["c6.bam", "c6_g.sam", "c6_t.sam"]             # and no temporary file


@pytest.fixture(scope="module")
def c7(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("c7"))
    texts = S.c7()
    return d, texts, _write(os.path.join(d, "g.sam"), texts[0]), _write(os.path.join(d, "t.sam"), texts[1])


def test_c7_many_workers(c7):
    """more than 2 * 4096 lifted records: 1, 2, 3 and (of 8 threads) 3 workers assemble them, and the file is the same"""
    d, texts, _, _ = c7
    outs = []
    for threads in (1, 2, 3, 8):
        out, st, _ = _both(d, texts, name="w%d" % threads, threads=threads)     # the restatement's records, in order
        assert st["n_lifted"] >= 8192
        outs.append(inflated(out))
    assert outs[1] == outs[0] and outs[2] == outs[0] and outs[3] == outs[0]


def test_c7_sorted_and_indexed(c7):
    import capi
    from test_bam import read_bai, read_bam, reg2bins, voffset_to_u
    d, texts, g, t = c7
    u, s, su = (os.path.join(d, x) for x in ("u.bam", "s.bam", "su.bam"))
    capi.ps_combine_genome_transcript(g, t, u)
    st = capi.ps_combine_genome_transcript(g, t, s, sort_by_coordinate=True, write_index=True)
    exp_text, exp_refs, exp, exp_st = J.combine(J.parse_sam(texts[0]), J.parse_sam(texts[1]), True)
    text, refs, recs, _ = read_bam(s)
    assert text == exp_text and refs == exp_refs and J.same_records(recs, exp) is None, J.same_records(recs, exp)
    _stats_equal(st, exp_st, s)
    capi.ps_bam_sort(u, su)
    assert inflated(s) == inflated(su)
    _check_index(s, read_bam, read_bai, reg2bins, voffset_to_u, n_queries=8)
