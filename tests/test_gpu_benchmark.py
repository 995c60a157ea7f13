"""ps_benchmark_reads on the GPU: the hand-worked cases of tests/test_benchmark_cpu.py from SAM and from BAM, byte for byte
and counter for counter what the restatement tests/java_benchmark.py gives; generated inputs around the wave and block
sizes; one FASTQ counted in pieces of every awkward size; and a mapping made by ps_map, scored here, by the restatement and
by simulate.score_truth."""
import os

import pytest

import java_benchmark as J
from test_benchmark_cpu import CASES, ERRORS, fastq, header, name, rec

pytestmark = pytest.mark.gpu


def _write(path, data):
    with open(path, "wb" if isinstance(data, bytes) else "w") as f:
        f.write(data)
    return str(path)


def _run(tmp_path, sam_text, fq_bytes, from_bam=False):
    """the library on the two files -> (bytes of the statistics file, stats)"""
    import capi
    sam, fq, out = _write(tmp_path / "m.sam", sam_text), _write(tmp_path / "r.fq", fq_bytes), str(tmp_path / "out.stats")
    if from_bam:
        capi.ps_sam_to_bam(sam, sam[:-3] + "bam")
        sam = sam[:-3] + "bam"
    if os.path.exists(out):
        os.remove(out)
    st = capi.ps_benchmark_reads(sam, out, fq)
    return open(out, "rb").read(), st


def _same_as_restatement(tmp_path, sam_text, fq_bytes, from_bam=False):
    exp_text, exp_st = J.benchmark(sam_text, fq_bytes)
    got_text, st = _run(tmp_path, sam_text, fq_bytes, from_bam)
    assert got_text == exp_text
    assert J.same_stats(st, exp_st) is None, (J.same_stats(st, exp_st), st, exp_st)
    return st


@pytest.mark.parametrize("from_bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("key", sorted(CASES))
def test_hand_worked_cases(tmp_path, key, from_bam):
    sam_text, fq_bytes, exp_text, exp_st = CASES[key]
    got_text, st = _run(tmp_path, sam_text, fq_bytes, from_bam)
    assert got_text == exp_text                                          # the hand-worked answer
    assert {k: st[k] for k in J.INT_KEYS} == exp_st
    assert J.same_stats(st, J.benchmark(sam_text, fq_bytes)[1]) is None  # the ratios too


@pytest.mark.parametrize("from_bam", [False, True], ids=["sam", "bam"])
@pytest.mark.parametrize("key", sorted(ERRORS))
def test_errors_write_nothing(tmp_path, key, from_bam):
    import capi
    sam_text, fq_bytes, what = ERRORS[key]
    sam, fq = _write(tmp_path / "m.sam", sam_text), _write(tmp_path / "r.fq", fq_bytes)
    if from_bam:
        capi.ps_sam_to_bam(sam, sam[:-3] + "bam")
        os.remove(sam)
        sam = sam[:-3] + "bam"
    with pytest.raises(capi.PsError, match=what):
        capi.ps_benchmark_reads(sam, str(tmp_path / "out.stats"), fq)
    assert sorted(p.name for p in tmp_path.iterdir()) == [os.path.basename(sam), "r.fq"]


def test_gzip_reads_are_refused(tmp_path):
    import gzip
    import capi
    sam, fq = _write(tmp_path / "m.sam", CASES["window"][0]), _write(tmp_path / "r.fq.gz", gzip.compress(CASES["window"][1]))
    with pytest.raises(capi.PsError, match="gzip"):
        capi.ps_benchmark_reads(sam, str(tmp_path / "out.stats"), fq)
    assert not os.path.exists(str(tmp_path / "out.stats"))


def generated(n, bad_at=None, chr_at=64):
    """n records by a fixed pattern -- i % 4: TP, TN, one base outside the window, the other contig -- on contigs "1" and "2"; the
    record at chr_at lies on "chr3", the first name with "chr", after which every truth name gets "chr" and only records on chr3
    (every fifth from there) can still hit; bad_at: the one record whose start does not parse"""
    sam, names = [header(("1", "2", "chr3"))], []
    for i in range(n):
        on_chr3 = i >= chr_at and (i - chr_at) % 5 == 0
        truth = "3" if on_chr3 else "1"
        s = 1000 + 3 * i
        nm = name(truth, "12a" if i == bad_at else str(s), str(s + 49), "%d-%d:%d" % ((i % 4 != 1), i // 16 + 1, i % 16))
        kind = i % 4
        contig = "chr3" if on_chr3 else ("2" if kind == 3 else "1")
        sam.append(rec(nm, 16 * (i % 2), contig, s + (6 if kind == 2 else 0), "50M"))
        names.append(nm)
    return "".join(sam), fastq(names)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1025])
def test_wave_and_block_edges(tmp_path, n):
    """one lane per record, 64 lanes per wave, 256 per block: every count and every index minimum across those edges"""
    st = _same_as_restatement(tmp_path, *generated(n))
    assert st["n_processed"] == n and st["bad_number_record"] == 0 and st["n_tp"] + st["n_tn"] > 0
    if n > 65:                                                           # (at 65 the one record on chr3 hits either way)
        none = _same_as_restatement(tmp_path, *generated(n, chr_at=n))   # without the "chr" contig more records hit
        assert none["n_tp"] + none["n_tn"] > st["n_tp"] + st["n_tn"]
    for bad_at in sorted({0, 63, 64, n - 1}):
        if bad_at < n:
            st = _same_as_restatement(tmp_path, *generated(n, bad_at), from_bam=bad_at == 64)
            assert st["n_processed"] == bad_at and st["bad_number_record"] == bad_at + 1 and st["n_records"] == n


def piece_fastq(n=200):
    """n reads, names of changing length, line ends "\\n", "\\r\\n" and "\\r" by turns, one quality line that starts "@SEQ_ID", no
    end after the last line"""
    out, names = [], []
    for i in range(n):
        nm = name("c1", str(1000 + 7 * i), str(1049 + 7 * i), "%d-%d:%d" % (i % 3 != 0, i + 1, i % 16)) + "x" * (i % 11)
        end = ("\n", "\r\n", "\r")[i % 3]
        qual = "@SEQ_ID|a|b|c|d|1-xx" if i == 100 else "I" * 20
        out.append("@%s%s%s%s+%s%s%s" % (nm, end, "ACGT" * 5, end, end, qual, end))
        names.append(nm)
    return "".join(out).rstrip("\r\n").encode(), names


def boundary_kinds(data, piece):
    """which kinds of place the piece boundaries of `data` fall on: inside a "@SEQ_ID" line, between "\\r" and "\\n", directly
    before a line start"""
    kinds, start = set(), 0                                               # start: where the line that holds b - 1 begins
    starts = [0] + [i + 1 for i in range(len(data) - 1) if data[i] == 10 or (data[i] == 13 and data[i + 1] != 10)]
    is_start = set(starts)
    for b in range(piece, len(data), piece):
        if data[b - 1] == 13 and data[b] == 10:
            kinds.add("between_cr_lf")
        elif b in is_start:
            kinds.add("before_line_start")
        else:
            start = max(s for s in starts if s < b)
            if data[start:start + 7] == b"@SEQ_ID" and data[b] not in (10, 13):
                kinds.add("inside_header")
    return kinds


def test_pieces_do_not_change_the_counts(tmp_path, monkeypatch):
    fq_bytes, names = piece_fastq()
    sam_text = header() + "".join(rec(nm, 0, "c1", 1000 + 7 * i, "50M") for i, nm in enumerate(names[:20]))
    exp_text, exp_st = J.benchmark(sam_text, fq_bytes)
    assert exp_st["n_reads"] == 200 and exp_st["n_positives"] == 134 and exp_st["n_negatives"] == 67   # 133 names and the quality line; 67 names
    for piece in (1, 7, 64, 4096, None):
        if piece is None:
            monkeypatch.delenv("PS_BENCH_PIECE")
        else:
            monkeypatch.setenv("PS_BENCH_PIECE", str(piece))
            if piece <= 64:
                assert boundary_kinds(fq_bytes, piece) == {"inside_header", "between_cr_lf", "before_line_start"}
        got_text, st = _run(tmp_path, sam_text, fq_bytes)
        assert got_text == exp_text and J.same_stats(st, exp_st) is None, (piece, J.same_stats(st, exp_st))


def test_mapped_reads_end_to_end(example, workdir, tmp_path):
    """simulate -> ps_map -> ps_benchmark_reads: the restatement's bytes and counters on the same SAM, and simulate.score_truth's
    count on the records it looks at (it passes over flag 4).  No accuracy is asked of the aligner: this pins the scorer."""
    import capi
    import simulate as S
    fa = example["fa"]
    if not os.path.exists(fa + ".bwt"):
        capi.ps_index(fa)
    fq, sam = os.path.join(workdir, "bench_reads.fq"), os.path.join(workdir, "bench_reads.sam")
    S.write_fastq(fq, S.simulate_reads(example["genome"], 2000, 50, seed=57, indel_scale=30))
    capi.ps_map(4, "2", None, None, fa, fq, sam)
    sam_text, fq_bytes = open(sam).read(), open(fq, "rb").read()
    st = _same_as_restatement(tmp_path, sam_text, fq_bytes)
    assert st["n_reads"] == 2000 and st["n_records"] == st["n_processed"] == 2000 and st["n_positives"] + st["n_negatives"] == 2000
    mapped_only = "".join(l for l in sam_text.splitlines(True) if l.startswith("@") or not int(l.split("\t")[1]) & 4)
    _, st_mapped = _run(tmp_path, mapped_only, fq_bytes)
    mapped, correct, total = S.score_truth(sam)
    assert st_mapped["n_records"] == mapped and st_mapped["n_tp"] + st_mapped["n_tn"] == correct and total == 2000


def test_mirror(tmp_path):
    import __graft_entry__ as ge
    mod = ge.load_package()
    sam_text, fq_bytes, exp_text, _ = CASES["flag4"]
    sam, fq, out = _write(tmp_path / "m.sam", sam_text), _write(tmp_path / "r.fq", fq_bytes), str(tmp_path / "o.stats")
    st = mod.mapping.ValidateBenchmarkStatisticsPARCLIP().calculateBenchmarkStatistics(sam, out, fq, True)
    assert open(out, "rb").read() == exp_text and st["n_tp"] == 1
    with pytest.raises(mod.mapping.ExternalCallErrorException, match="line 5"):
        mod.mapping.ValidateBenchmarkStatisticsPARCLIP().calculateBenchmarkStatistics(sam, out + "2", _write(tmp_path / "bad.fq", ERRORS["short_name_in_fastq"][1]))
    assert not os.path.exists(out + "2")
