"""ps_simulate_reads on the GPU: all five files byte for byte and every counter as tests/perl_simulator.py gives them, over
generated transcript sets around the wave and block sizes and the shortest transcript that can emit; the degenerate-parameter
checks of tests/test_simulator_cpu.py on the library's own output; determinism; every error, with nothing left behind; and the
FASTQ read back by ps_benchmark_reads."""
import functools
import os

import pytest

import perl_simulator as P
from test_simulator_cpu import (ALL_SITES, DEGENERATE, IDENTITY, LENGTHS, broken_inputs, check_degenerate, check_statistics, fasta_bytes,
                                make_transcripts, parse_clusters, parse_fastq, profiles)

pytestmark = pytest.mark.gpu

SUFFIXES = (".fastq", ".clusters", "_snps.vsf", ".log", ".err")
INPUT_NAMES = ("transcripts.fa", "error_profile.txt", "site_frequency.txt", "site_positions.txt", "qualities.txt", "indels.txt")


def run_library(tmp_path, fasta, prof, bound_prob, seed, **kw):
    """the library on the six inputs -> ({suffix: bytes}, stats)"""
    import capi
    paths = []
    for name, data in zip(INPUT_NAMES, [fasta] + list(prof)):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    prefix = str(tmp_path / "sim")
    for sfx in SUFFIXES:
        if os.path.exists(prefix + sfx):
            os.remove(prefix + sfx)
    st = capi.ps_simulate_reads(paths[0], prefix, *paths[1:], bound_prob, seed, **kw)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(INPUT_NAMES + tuple("sim" + s for s in SUFFIXES))
    return {sfx: open(prefix + sfx, "rb").read() for sfx in SUFFIXES}, st


def same_as_restatement(tmp_path, fasta, prof, bound_prob, seed, **kw):
    exp_files, exp_st = P.simulate(fasta, *prof, bound_prob, seed, **kw)
    files, st = run_library(tmp_path, fasta, prof, bound_prob, seed, **kw)
    for sfx in SUFFIXES:
        assert files[sfx] == exp_files[sfx], sfx
    assert {k: st[k] for k in P.INT_KEYS} == {k: exp_st[k] for k in P.INT_KEYS}
    assert st["avg_read_length"] == exp_st["avg_read_length"] and st["avg_reads_per_cluster"] == exp_st["avg_reads_per_cluster"]
    return files, st


@functools.lru_cache(maxsize=None)
def generated(n, seed=21):
    """n transcripts whose lengths go round LENGTHS -- 39, 40 and 41 around the shortest that can emit, up to 1,600 -- with 1 to 5
    exons and both strands; computed once"""
    return tuple(make_transcripts([LENGTHS[t % len(LENGTHS)] for t in range(n)], seed))


@pytest.mark.parametrize("n,select_read,bound_prob", [(2, 1.0, 0.6), (63, 1.0, 0.0), (64, 1.0, 1.0), (65, None, 0.6), (257, None, 0.6), (257, 1.0, 0.6)])
def test_bytes_match_the_restatement(tmp_path, n, select_read, bound_prob):
    """one lane per transcript, 64 lanes per wave, 256 per block; the last transcript is dropped, so 64 lanes are busy at n = 65"""
    transcripts = generated(13)[7:9] if n == 2 else generated(n)         # n = 2: lengths 400 and 1600, of which the 400 is simulated
    files, st = same_as_restatement(tmp_path, fasta_bytes(transcripts), profiles(), bound_prob, 5, select_read=select_read)
    assert st["n_transcripts"] == n and st["n_reads"] > 0 and st["n_selected"] <= n - 1
    if select_read == 1.0:
        assert st["n_selected"] == n - 1
    if n >= 63:
        assert st["n_clusters_skipped"] > 0                               # lengths 40 .. 52: positions below 10
        assert (st["n_t2c"] > 0) == (bound_prob > 0)


def test_one_long_transcript(tmp_path):
    """100 kb: the SNP pass spreads it over 25 blocks per cluster, and the plan kernel reads its text far from its start"""
    transcripts = make_transcripts([100000, 1600, 50], seed=33)
    files, st = same_as_restatement(tmp_path, fasta_bytes(transcripts), profiles(), 0.6, 8, select_read=1.0)
    assert st["n_snp_positions"] >= 101600 and st["n_snps_preselected"] > 500 and 0 < st["n_snps_reported"] < st["n_snps_preselected"]


def test_every_branch_of_the_loop(tmp_path):
    """rates turned up so that one small run takes every branch: characters that are no ACGT, SNPs on them and on bases,
    insertions (the repeated iteration) and deletions, T->C sites"""
    transcripts = make_transcripts([300] * 40, seed=34, alphabet="ACGTTN")
    indels = b"0.05\t0.15\n" * 31
    files, st = same_as_restatement(tmp_path, fasta_bytes(transcripts), profiles(indels=indels), 1.0, 77, select_read=1.0, snp_rate=0.2, snp_report=0.5)
    assert min(st[k] for k in ("n_non_acgt", "n_snps", "n_indels", "n_t2c", "n_errors", "n_snps_reported")) > 0
    reads = parse_fastq(files[".fastq"])
    assert any(len(r["seq"]) != len(r["qual"]) for r in reads)            # a SNP on a non-ACGT character: a quality without a base
    assert files[".err"].count(b"unrecognized base in ACGT_hash=N\n") == st["n_non_acgt"]


@pytest.mark.parametrize("t2c", [False, True], ids=["copies", "t2c"])
def test_degenerate_parameters(tmp_path, t2c):
    transcripts = make_transcripts(LENGTHS * 3, seed=5)
    prof = profiles(error_profile=IDENTITY, site_frequency=ALL_SITES) if t2c else profiles(error_profile=IDENTITY)
    files, st = run_library(tmp_path, fasta_bytes(transcripts), prof, 1.0 if t2c else 0.0, 11, **DEGENERATE)
    assert check_degenerate(files, transcripts, t2c) == st["n_reads"] > 300
    assert st["n_selected"] == len(transcripts) - 1 and st["n_errors"] == st["n_indels"] == st["n_snps"] == 0 and (st["n_t2c"] > 0) == t2c


def test_statistics_of_the_library(tmp_path):
    """the statistics check of the CPU tier on the library's own draws (the same inputs and seed)"""
    transcripts = make_transcripts([400] * 280, seed=12)
    files, st = run_library(tmp_path, fasta_bytes(transcripts), profiles(), 0.0, 2024, select_read=1.0, snp_rate=0.0, allow_indels=0)
    assert check_statistics(transcripts, files) == st["sum_read_length"]


def test_determinism(tmp_path):
    fa, prof = fasta_bytes(generated(65)), profiles()
    a, st_a = run_library(tmp_path, fa, prof, 0.6, 1234, select_read=1.0)
    b, st_b = run_library(tmp_path, fa, prof, 0.6, 1234, select_read=1.0)
    c, _ = run_library(tmp_path, fa, prof, 0.6, 1235, select_read=1.0)
    assert a == b and {k: st_a[k] for k in P.INT_KEYS} == {k: st_b[k] for k in P.INT_KEYS}
    assert all(a[s] != c[s] for s in (".fastq", ".clusters", "_snps.vsf", ".log"))
    d, _ = run_library(tmp_path, fa, prof, 0.6, 1234 + (1 << 40), select_read=1.0)   # the high half of the seed counts
    assert a[".fastq"] != d[".fastq"]


@pytest.mark.parametrize("key", sorted(broken_inputs()))
def test_errors_leave_nothing(tmp_path, key):
    import capi
    fa, replace, what = broken_inputs()[key]
    with pytest.raises(capi.PsError, match=what) as ei:
        run_library(tmp_path, fa, profiles(**replace), 0.5, 1)
    if key.startswith("short_") and key != "short_exons":
        assert key[len("short_"):] + ".txt" in str(ei.value)              # the file is named
    if key == "only_one_transcript":
        assert "transcripts.fa" in str(ei.value)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(INPUT_NAMES)


def test_missing_file_and_missing_directory(tmp_path):
    import capi
    fa = fasta_bytes(generated(13))
    with pytest.raises(capi.PsError, match="nowhere.txt"):
        capi.ps_simulate_reads(str(tmp_path / "nowhere.txt"), str(tmp_path / "sim"), *[str(tmp_path / "nowhere.txt")] * 5, 0.5, 1)
    files, _ = run_library(tmp_path, fa, profiles(), 0.5, 1, select_read=1.0)
    paths = [str(tmp_path / nm) for nm in INPUT_NAMES]
    with pytest.raises(capi.PsError, match="cannot write"):
        capi.ps_simulate_reads(paths[0], str(tmp_path / "no_such_dir" / "sim"), *paths[1:], 0.5, 1, select_read=1.0)
    assert not os.path.exists(str(tmp_path / "no_such_dir"))


def test_benchmark_reads_the_names(tmp_path):
    """simulate -> ps_benchmark_reads with a mapping that holds no record: every name parses, every read is a positive or a
    negative, and the positives are the reads of the clusters that .clusters marks 1"""
    import capi
    transcripts = generated(65)
    files, st = run_library(tmp_path, fasta_bytes(transcripts), profiles(), 0.6, 99, select_read=1.0)
    sam = tmp_path / "empty.sam"
    sam.write_text("@HD\tVN:1.4\n@SQ\tSN:c0\tLN:100000\n")
    bm = capi.ps_benchmark_reads(str(sam), str(tmp_path / "bench.stats"), str(tmp_path / "sim.fastq"))
    assert bm["n_reads"] == st["n_reads"] and bm["n_records"] == 0
    assert bm["n_positives"] + bm["n_negatives"] == bm["n_reads"]
    bound_of, seen = {}, {}
    for ln in parse_clusters(files[".clusters"]):                         # the k-th line of a chromosome is the names' cluster k
        k = seen[ln["chrom"]] = seen.get(ln["chrom"], 0) + 1
        bound_of[(ln["chrom"], k)] = ln["bound"]
    reads = parse_fastq(files[".fastq"])
    assert bm["n_positives"] == sum(bound_of[(r["chrom"], r["cluster"])] for r in reads)
    assert 0 < bm["n_positives"] < bm["n_reads"] and all(r["bound"] == bound_of[(r["chrom"], r["cluster"])] for r in reads)
