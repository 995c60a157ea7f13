"""CPU tier of the `simulate` mode: tests/perl_simulator.py, the plain-Python restatement of the toolkit's read simulator that
ps_simulate_reads must match byte for byte -- its random stream against known answers, its output under degenerate parameters
against truth that this file works out on its own (generated transcripts, exon maps built here), the Perl's quirks one small
case each, and the statistics of its draws against the profile files.  tests/test_gpu_simulate.py runs the same checks on the
library's output."""
import math
import os
import random
import re

import pytest

import perl_simulator as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


PROFILE_FILES = ("example.errorprofile", "example.sitefrequency", "example.sitepositions", "example.qualities", "example.indels")
IDENTITY = b"1\t0\t0\t0\n0\t1\t0\t0\n0\t0\t1\t0\n0\t0\t0\t1\n"
ALL_SITES = b"1.0\n" * 4


def profiles(**replace):
    """the five profile files in argument order; error_profile= / site_frequency= / ... replace one"""
    keys = ("error_profile", "site_frequency", "site_positions", "qualities", "indels")
    return [replace.get(k, golden(f)) for k, f in zip(keys, PROFILE_FILES)]


DEGENERATE = dict(select_read=1.0, snp_rate=0.0, allow_indels=0)      # with an identity error profile: reads are copies


# ---- transcripts whose truth this file knows

class Transcript:
    def __init__(self, gene, chrom, seq, exons, strand):
        self.gene, self.chrom, self.seq, self.exons, self.strand = gene, chrom, seq, exons, strand
        self.positions = [p for s, e in sorted(exons) for p in range(s, e + 1)]   # the genomic position of every transcript index
        if strand == -1:
            self.positions.reverse()
        self.index_of = {p: i for i, p in enumerate(self.positions)}

    def fasta(self, width=60):
        head = ">%s|tr_%s|%s|%s|%s|%d" % (self.gene, self.gene, self.chrom, ";".join(str(s) for s, _ in self.exons),
                                          ";".join(str(e) for _, e in self.exons), self.strand)
        return head + "\n" + "".join(self.seq[i:i + width] + "\n" for i in range(0, len(self.seq), width))


def make_transcripts(lengths, seed, alphabet="ACGT"):
    """one transcript per length, each on a chromosome of its own ("c<t>"), 1 to 5 exons (t % 5 + 1) listed in shuffled order,
    strands by turns; the exons hold exactly the sequence"""
    rng, out = random.Random(seed), []
    for t, n in enumerate(lengths):
        n_exons = min(t % 5 + 1, max(1, n // 8))
        cuts = sorted(rng.sample(range(1, n), n_exons - 1)) if n_exons > 1 else []
        exons, at = [], 1000 + 17 * t
        for a, b in zip([0] + cuts, cuts + [n]):
            exons.append((at, at + (b - a) - 1))
            at += (b - a) + rng.randrange(50, 500)
        rng.shuffle(exons)
        out.append(Transcript("g%d" % t, "c%d" % t, "".join(rng.choice(alphabet) for _ in range(n)), exons, 1 if t % 2 == 0 else -1))
    return out


def fasta_bytes(transcripts):
    return "".join(t.fasta() for t in transcripts).encode()


NAME = re.compile(r"@SEQ_ID:>([^|]*)\|([^|]*)\|([^|]*)\|(-?\d+)\|(-?\d+)\|([01])-(\d+):(\d+)\Z")


def parse_fastq(data):
    """-> [dict(gene, chrom, a, b, bound, cluster, i, seq, qual)]"""
    lines = data.decode("latin-1").split("\n")
    assert lines[-1] == "" and len(lines) % 4 == 1
    out = []
    for k in range(0, len(lines) - 1, 4):
        m = NAME.match(lines[k])
        assert m, lines[k]
        assert lines[k + 2] == "+"
        out.append(dict(gene=m.group(1), chrom=m.group(3), a=int(m.group(4)), b=int(m.group(5)), bound=int(m.group(6)),
                        cluster=int(m.group(7)), i=int(m.group(8)), seq=lines[k + 1], qual=lines[k + 3]))
    return out


def parse_clusters(data):
    out = []
    for line in data.decode().splitlines():
        name, chrom, s, e, bound = line.split("\t")
        assert name.startswith("cl_") and chrom.startswith("chr")
        out.append(dict(n=int(name[3:]), chrom=chrom[3:], start=int(s), end=int(e), bound=int(bound)))
    return out


def span(t, rd):
    """a read's [start, end) on the transcript, from the coordinates in its name and this file's own exon map"""
    if t.strand == 1:
        return t.index_of[rd["a"]], t.index_of[rd["b"]]
    return t.index_of[rd["b"] - 1], t.index_of[rd["a"] - 1]


def check_degenerate(files, transcripts, t2c=False):
    """the checks of the degenerate runs (identity error profile, no SNPs, no indels, every transcript selected), on the five
    files alone; t2c: bound_prob 1 and all site frequencies 1.0, else bound_prob 0.  Returns the number of reads looked at."""
    by_chrom = {t.chrom: t for t in transcripts}
    reads, lines = parse_fastq(files[".fastq"]), parse_clusters(files[".clusters"])
    assert reads and files[".err"] == b"" and files["_snps.vsf"].count(b"\n") == 1
    assert all(r["gene"] != transcripts[-1].gene for r in reads)          # the last transcript yields nothing
    per_cluster = {}
    for r in reads:
        t = by_chrom[r["chrom"]]
        assert r["gene"] == t.gene and r["bound"] == int(t2c)
        start, end = span(t, r)
        assert 0 < end - start <= 30 and len(r["seq"]) == len(r["qual"]) == end - start
        assert all(36 <= ord(q) <= 97 for q in r["qual"])                 # 33 + 3 .. 33 + 64
        wt = t.seq[start:end]
        if not t2c:
            assert r["seq"] == wt
        else:
            assert all(x == w or (w == "T" and x == "C") for x, w in zip(r["seq"], wt))
        per_cluster.setdefault((r["chrom"], r["cluster"]), []).append((start, end, r))
    # the k-th .clusters line of a chromosome is the cluster that the read names call k; it spans its reads exactly
    seen = {}
    for ln in lines:
        t = by_chrom[ln["chrom"]]
        k = seen[ln["chrom"]] = seen.get(ln["chrom"], 0) + 1
        assert ln["bound"] == int(t2c) and ln["start"] <= ln["end"]
        lo, hi = (t.index_of[ln["start"]], t.index_of[ln["end"]]) if t.strand == 1 else (t.index_of[ln["end"]], t.index_of[ln["start"]])
        for start, end, _ in per_cluster.get((ln["chrom"], k), []):
            assert lo <= start and end <= hi
    assert all(k <= seen.get(c, 0) for c, k in per_cluster)
    if t2c:
        n_sites = 0
        for (chrom, _), rs in per_cluster.items():
            t = by_chrom[chrom]
            sites = {s + j for s, e, r in rs for j in range(e - s) if r["seq"][j] != t.seq[s + j]}
            n_sites += len(sites)
            assert len(sites) <= 4
            assert all(max(s for s, _, _ in rs) <= p < min(e for _, e, _ in rs) for p in sites)
            for s, e, r in rs:                                            # rate 1.0: every read that covers a site shows it
                assert all(r["seq"][p - s] == "C" for p in sites if s <= p < e)
        assert n_sites > 0
    return len(reads)


LENGTHS = [39, 40, 41, 45, 52, 80, 131, 400, 1600, 77, 300, 64]


# ---- the random stream

def test_mixer_known_answers():
    # splitmix64 seeded with 0: its published first outputs are mix(1 * golden), mix(2 * golden), mix(3 * golden)
    assert P.run_key(0) == 0xE220A8397B1DCDAF
    assert P.mix(2 * P.GOLDEN & P.M64) == 0x6E789E6AA1B965F4 and P.mix(3 * P.GOLDEN & P.M64) == 0x06C45D188009454F
    assert P.mix(0) == 0
    # the key layout, spelled out: run -> transcript -> cluster << 32 | read -> slot
    run = P.run_key(7)
    unit = P.mix(P.mix(run ^ 5) ^ (2 << 32 | 9))
    assert P.unit_key(run, 5, 2, 9) == unit and P.draw32(unit, 130) == P.mix(unit ^ 130) >> 32
    assert (P.run_key(7), P.unit_key(run, 5, 2, 9), P.draw32(unit, 130)) == KNOWN_KEYS


KNOWN_KEYS = (0x63CBE1E459320DD7, 0x2B7649CDE9861523, 0x38E357FA)


def test_normal_known_answers():
    half, top = 1 << 31, (1 << 32) - 1
    assert P.normal_from_draws([half] * 12, 16.0, 10.0) == 16.0          # z = 0
    assert P.normal_from_draws([0] * 12, 16.0, 10.0) == -44.0            # z = -6
    assert P.normal_from_draws([top] * 12, 0.0, 1.0) == 6.0 - 12 * 2.0 ** -32
    assert P.normal_from_draws([half] * 11 + [half + (1 << 30)], 31.0, 4.0) == 32.0   # z = 1/4
    # a product and a sum that a fused multiply-add would round differently: 0.1 * 3 + 0.3
    z3 = [half + (1 << 32) // 4 * 1] * 12                                # z = 3
    assert P.normal_from_draws(z3, 0.3, 0.1) == 0.3 + 0.1 * 3.0 == 0.6000000000000001
    assert int(P.normal_from_draws([0] * 12, 2.5, 1.0)) == -3            # int() truncates toward zero
    assert P.ceil_rand(P.unit_key(P.run_key(1), 0, 0, 0), 1, 3) in (1, 2, 3) and P.ceil_rand(0, 0, -5) == 0


def test_perl_numbers():
    assert [P.perl_num(s) for s in ("3.8\r", " 2E-05", "0.5abc", "", "x1", ".5", "1.", "1e", "-4\t")] == [3.8, 2e-05, 0.5, 0.0, 0.0, 0.5, 1.0, 1.0, -4.0]
    assert [P.perl_str(v) for v in (1 / 3, 16.0, 0.216, 0.1 + 0.2, 22.5)] == ["0.333333333333333", "16", "0.216", "0.3", "22.5"]
    assert P._split_ws(" 0.1 0.2\r") == ["", "0.1", "0.2"] and P._split_ws("") == []


# ---- degenerate parameters: the output against truth worked out here

def degenerate_run(transcripts, t2c, seed=11):
    prof = profiles(error_profile=IDENTITY, site_frequency=ALL_SITES) if t2c else profiles(error_profile=IDENTITY)
    return P.simulate(fasta_bytes(transcripts), *prof, 1.0 if t2c else 0.0, seed, **DEGENERATE)


@pytest.mark.parametrize("t2c", [False, True], ids=["copies", "t2c"])
def test_degenerate_parameters(t2c):
    transcripts = make_transcripts(LENGTHS * 3, seed=5)
    files, st = degenerate_run(transcripts, t2c)
    assert check_degenerate(files, transcripts, t2c) == st["n_reads"] > 300
    assert st["n_selected"] == len(transcripts) - 1 and st["n_errors"] == st["n_indels"] == st["n_snps"] == 0
    assert (st["n_t2c"] > 0) == t2c


def hand_built(strand):
    """two exons, 1000..1049 and 2000..2059, and behind it the transcript that is never simulated"""
    rng = random.Random(3)
    seq = "".join(rng.choice("ACGT") for _ in range(110))
    return [Transcript("hand", "7", seq, [(2000, 2059), (1000, 1049)], strand), Transcript("last", "8", "ACGT" * 20, [(1, 80)], 1)]


@pytest.mark.parametrize("strand", [1, -1])
def test_hand_built_exon_map(strand):
    transcripts = hand_built(strand)
    files, st = degenerate_run(transcripts, False, seed=4)
    reads = parse_fastq(files[".fastq"])
    assert len(reads) == st["n_reads"] > 5
    for r in reads:
        seq = transcripts[0].seq
        assert seq.count(r["seq"]) == 1
        start = seq.find(r["seq"])
        end = start + len(r["seq"])

        def genomic(i):                                                   # by hand: index -> position, forward and reversed
            if strand == -1:
                i = 109 - i
            return 1000 + i if i < 50 else 2000 + (i - 50)
        assert (r["a"], r["b"]) == ((genomic(start), genomic(end)) if strand == 1 else (genomic(end) + 1, genomic(start) + 1))
    assert re.match(rb"cl_\d+\tchr7\t", files[".clusters"])


# ---- the quirks

def test_last_transcript_yields_nothing():
    transcripts = make_transcripts([200, 200], seed=1)
    files, st = degenerate_run(transcripts, False)
    assert st["n_transcripts"] == 2 and st["n_selected"] == 1 and {r["gene"] for r in parse_fastq(files[".fastq"])} == {"g0"}
    with pytest.raises(P.SimError, match="no read"):
        degenerate_run(transcripts[:1], False)


def test_skipped_cluster_takes_a_number_but_no_index():
    transcripts = make_transcripts([45] * 60, seed=2)                    # positions 1..15: nine of them are < 10
    files, st = degenerate_run(transcripts, False)
    lines, reads = parse_clusters(files[".clusters"]), parse_fastq(files[".fastq"])
    numbers = [ln["n"] for ln in lines]
    assert st["n_clusters_skipped"] > 0 and len(numbers) == st["n_clusters"] - st["n_clusters_skipped"]
    assert numbers == sorted(set(numbers)) and numbers[-1] <= st["n_clusters"] and numbers != list(range(1, len(numbers) + 1))
    per_chrom = {}
    for ln in lines:
        per_chrom[ln["chrom"]] = per_chrom.get(ln["chrom"], 0) + 1
    assert all(1 <= r["cluster"] <= per_chrom[r["chrom"]] for r in reads)   # the index counts only clusters with a line
    check_degenerate(files, transcripts)


def test_snp_lengthens_the_read():
    transcripts = make_transcripts([300] * 6, seed=4)
    files, st = P.simulate(fasta_bytes(transcripts), *profiles(error_profile=IDENTITY), 0.0, 9, select_read=1.0, snp_rate=1.0, allow_indels=0)
    by_chrom, extras = {t.chrom: t for t in transcripts}, 0
    for r in parse_fastq(files[".fastq"]):
        t = by_chrom[r["chrom"]]
        start, end = span(t, r)
        wt, k = t.seq[start:end], 0
        for w in wt:                                                      # [alternative,] base -- the alternative is never the base
            if r["seq"][k] != w:
                extras, k = extras + 1, k + 1
            assert r["seq"][k] == w
            k += 1
        assert k == len(r["seq"]) == len(r["qual"])
    assert extras == st["n_snps"] > 0 and st["n_snps_preselected"] == st["n_snp_positions"]
    vsf = files["_snps.vsf"].decode().splitlines()
    ids = [int(l.split("\t")[2][3:]) for l in vsf[1:]]
    assert len(ids) == st["n_snps_reported"] < st["n_snps_preselected"] and ids == sorted(ids) and ids[-1] <= st["n_snps_preselected"]
    for l in vsf[1:20]:
        chrom, pos, _, ref, alt = l.split("\t")[:5]
        t = by_chrom[chrom]
        assert t.seq[t.index_of[int(pos)]] == ref != alt and alt in "ACGT"


def test_read_left_out_keeps_its_number(monkeypatch):
    """end - start > 30 needs two draws 8 apart, which the fixtures' spread of 1 all but never gives: here the ends are drawn 8
    further out, so about half the reads are left out"""
    real = P.normal
    monkeypatch.setattr(P, "normal", lambda unit, slot, mean, sd: real(unit, slot, mean + 8.0 if sd == 1.0 and slot >= P.C_ENDS else mean, sd))
    transcripts = make_transcripts([5000] * 8, seed=6)
    files, st = degenerate_run(transcripts, False, seed=1)
    reads = parse_fastq(files[".fastq"])
    assert st["n_reads_skipped"] > 10 and st["n_reads"] == len(reads) > 10
    per_cluster = {}
    for r in reads:
        per_cluster.setdefault((r["chrom"], r["cluster"]), []).append(r["i"])
    assert all(v == sorted(set(v)) for v in per_cluster.values())
    assert any(v != list(range(v[0], v[0] + len(v))) for v in per_cluster.values())   # gaps: the numbers of the reads left out


def test_crlf_qualities():
    q = golden("example.qualities")
    assert q.count(b"\r\n") == 40
    transcripts = make_transcripts([200] * 5, seed=8)
    a = P.simulate(fasta_bytes(transcripts), *profiles(), 0.6, 3, select_read=1.0)
    b = P.simulate(fasta_bytes(transcripts), *profiles(qualities=q.replace(b"\r\n", b"\n")), 0.6, 3, select_read=1.0)
    assert a == b and len(set(a[0][".fastq"].split(b"\n")[3])) > 1


def test_non_acgt_base():
    transcripts = make_transcripts([120] * 4, seed=9, alphabet="ACGTN")
    files, st = degenerate_run(transcripts, False)
    entries = files[".err"].decode().split("\n")
    assert st["n_non_acgt"] == len(entries) // 3 > 0 and entries[-1] == ""
    by_gene = {t.gene: t for t in transcripts}
    for k in range(0, len(entries) - 1, 3):
        assert entries[k] == "unrecognized base in ACGT_hash=N"
        gene = entries[k + 1].split("|")[0]
        assert gene.startswith("Sequence_header=>") and entries[k + 2] == "Sequence=" + by_gene[gene[17:]].seq
    reads = parse_fastq(files[".fastq"])
    assert sum(r["seq"].count("N") for r in reads) == st["n_non_acgt"]   # identity rows: whichever row is drawn, a match copies the character
    # with the real profile a mismatch by k writes ACGT[k]: never the character, always a base
    files, st = P.simulate(fasta_bytes(transcripts), *profiles(error_profile=b"0 1 0 0\n0 0 1 0\n0 0 0 1\n1 0 0 0\n"), 0.0, 1, **DEGENERATE)
    by_chrom = {t.chrom: t for t in transcripts}
    for r in parse_fastq(files[".fastq"]):
        t = by_chrom[r["chrom"]]
        start, end = span(t, r)
        assert all(x == ("C" if w == "N" else "ACGT"[("ACGT".index(w) + 1) % 4]) for x, w in zip(r["seq"], t.seq[start:end]))


def broken_inputs():
    """{key: (fasta, profile replacements, what the message must name)}: every input that is an error, three transcripts each"""
    good = make_transcripts([100, 100, 100], seed=1)
    lines = fasta_bytes(good).split(b"\n")
    at = [k for k, l in enumerate(lines) if l.startswith(b">g1|")][0]
    f = lines[at].split(b"|")

    def with_header(fields):
        return b"\n".join(lines[:at] + [b"|".join(fields)] + lines[at + 1:])
    out = {"five_fields": (with_header(f[:5]), {}, "g1.*fields"),
           "exon_bound": (with_header(f[:3] + [f[3] + b"x"] + f[4:]), {}, "g1.*integer"),
           "short_exons": (b"\n".join(lines[:at + 1] + [b"ACGT"] + lines[at + 1:]), {}, "g1.*exons"),
           "only_one_transcript": (good[0].fasta().encode(), {}, "no read")}
    keys = ("error_profile", "site_frequency", "site_positions", "qualities", "indels")
    for key, n, name in zip(keys, (3, 3, 39, 30, 30), PROFILE_FILES):
        out["short_" + key] = (b"\n".join(lines), {key: b"".join(profiles()[keys.index(key)].splitlines(True)[:n])}, "%d lines" % n)
    return out


@pytest.mark.parametrize("key", sorted(broken_inputs()))
def test_errors_name_their_subject(key):
    fa, replace, what = broken_inputs()[key]
    with pytest.raises(P.SimError, match=what):
        P.simulate(fa, *profiles(**replace), 0.5, 1)


# ---- statistics of about 2 * 10^5 bases drawn with the fixture profiles

STAT_SEED = 2024


def stat_run():
    transcripts = make_transcripts([400] * 280, seed=12)
    files, st = P.simulate(fasta_bytes(transcripts), *profiles(), 0.0, STAT_SEED, select_read=1.0, snp_rate=0.0, allow_indels=0)
    return transcripts, files, st


def check_statistics(transcripts, files):
    """substitutions against the error profile's rows and the mean quality per read position against mean - 0.5 (int() cuts a
    normal value down to the integer below it), each within 5 standard errors computed from the observed n.  bound_prob 0, no
    SNPs and no indels, so that every read base stands over its transcript base"""
    rows = [[float(v) for v in l.split()] for l in golden("example.errorprofile").decode().splitlines()]
    qual = [[float(v) for v in l.split()] for l in golden("example.qualities").decode().splitlines()]
    by_chrom = {t.chrom: t for t in transcripts}
    subst = [[0] * 4 for _ in range(4)]
    qsum, qn = [0] * 31, [0] * 31
    for r in parse_fastq(files[".fastq"]):
        t = by_chrom[r["chrom"]]
        start, end = span(t, r)
        assert len(r["seq"]) == end - start
        for j, (x, w) in enumerate(zip(r["seq"], t.seq[start:end])):
            subst["ACGT".index(w)][("ACGT".index(x) - "ACGT".index(w)) % 4] += 1
            qsum[j] += ord(r["qual"][j]) - 33
            qn[j] += 1
    n_bases = sum(map(sum, subst))
    assert n_bases > 150000
    for b in range(4):
        n = sum(subst[b])
        for k in (1, 2, 3):
            p = rows[b][(b + k) % 4]
            print("subst", "ACGT"[b], k, subst[b][k], n * p, 5 * math.sqrt(n * p * (1 - p)))
            assert abs(subst[b][k] - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    for j in range(31):
        if qn[j]:
            mean, sd = qual[j]
            print("qual", j, qn[j], qsum[j] / qn[j], mean - 0.5)
            assert abs(qsum[j] / qn[j] - (mean - 0.5)) <= 5 * math.sqrt((sd * sd + 1 / 12) / qn[j])
    return n_bases


def test_statistics():
    transcripts, files, st = stat_run()
    assert check_statistics(transcripts, files) == st["sum_read_length"]


# ---- the library without a device

def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_library_fails_without_device(tmp_path):
    import capi
    paths = []
    for name, data in zip(("t.fa", "ep", "sf", "sp", "q", "i"), [fasta_bytes(make_transcripts([100, 100], seed=1))] + profiles()):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_simulate_reads(paths[0], str(tmp_path / "sim"), *paths[1:], 0.5, 1)
    assert len(list(tmp_path.iterdir())) == 6
