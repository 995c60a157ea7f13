"""Generated data for the `map -t` route (Main.java:363-416) and the check of lifted records against where the generator cut
the reads: shared by tests/test_combine_route_cpu.py (the oracle as the mapper, the restatement as the combiner) and
tests/test_gpu_combine.py (the library for every step).  Nothing is taken from the toolkit's example files.

A three-contig genome chr1..chr3; 88 transcripts per contig, each in a 1000-base window of its own (2-4 exons of 30-80 bases,
introns of 40-200), every other one on strand -1 (its sequence is the reverse complement of the exon concatenation); headers
Gene|Transcript|Chr|starts|ends|strand.  All exon coordinates have five digits, so the Java's string sort of the exon lists
(tests/java_combine.py) and the numeric order agree.  Reads of 36-50 bases are cut from the transcripts, either orientation,
four in ten with one substitution; most span one or two junctions, so the genome pass leaves them weak."""
import os
import re

import numpy as np

N_CONTIGS, PER_CONTIG, WINDOW, FIRST = 3, 88, 1000, 10500
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return b.translate(_COMP)[::-1]


def make_data(workdir, n_reads=6000, seed=0xC0B1):
    rng = np.random.default_rng(seed)
    genome = {"chr%d" % (c + 1): bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=FIRST + PER_CONTIG * WINDOW + 1000)])
              for c in range(N_CONTIGS)}
    transcripts = []          # (header, sequence as in the FASTA, genome coordinate of every base of the exon concatenation, chrom, strand)
    for c in range(N_CONTIGS):
        chrom = "chr%d" % (c + 1)
        for k in range(PER_CONTIG):
            at, starts, ends = FIRST + k * WINDOW + int(rng.integers(0, 40)), [], []
            for e in range(int(rng.integers(2, 5))):
                n = int(rng.integers(30, 81))
                starts.append(at); ends.append(at + n - 1)
                at += n + int(rng.integers(40, 201))
            assert 10000 <= starts[0] and ends[-1] <= 99999 and ends[-1] < FIRST + (k + 1) * WINDOW
            strand = -1 if (c * PER_CONTIG + k) & 1 else 1
            gpos = np.concatenate([np.arange(s, e + 1) for s, e in zip(starts, ends)])
            seq = b"".join(genome[chrom][s - 1:e] for s, e in zip(starts, ends))
            head = "GENE%d|TR%d_%d|%d|%s|%s|%d" % (c * PER_CONTIG + k, c + 1, k, c + 1, ";".join(map(str, starts)), ";".join(map(str, ends)), strand)
            transcripts.append((head, seq if strand == 1 else revcomp(seq), gpos, chrom, strand))
    g_fa, t_fa, fq = (os.path.join(workdir, x) for x in ("route_genome.fa", "route_transcripts.fa", "route_reads.fq"))
    with open(g_fa, "wb") as f:
        for name, seq in genome.items():
            f.write(b">" + name.encode() + b"\n" + b"".join(seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60)))
    with open(t_fa, "wb") as f:
        for head, seq, _, _, _ in transcripts:
            f.write(b">" + head.encode() + b"\n" + b"".join(seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60)))
    truth = {}
    with open(fq, "wb") as f:
        for r in range(n_reads):
            head, seq, gpos, chrom, strand = transcripts[int(rng.integers(0, len(transcripts)))]
            n = int(rng.integers(36, 51))
            o = int(rng.integers(0, len(seq) - n + 1))
            read = bytearray(seq[o:o + n])
            if rng.random() < 0.4:
                p = int(rng.integers(0, n))
                read[p] = b"ACGT"[(b"ACGT".index(read[p]) + int(rng.integers(1, 4))) % 4]
            read = bytes(read)
            if rng.random() < 0.5:
                read = revcomp(read)
            g = gpos[o:o + n] if strand == 1 else gpos[len(seq) - n - o:len(seq) - o]
            cuts = np.nonzero(np.diff(g) > 1)[0]
            cigar, a = "", 0
            for x in cuts:
                cigar += "%dM%dN" % (x + 1 - a, g[x + 1] - g[x] - 1)
                a = x + 1
            cigar += "%dM" % (n - a)
            name = "read%d" % r
            truth[name] = (chrom, int(g[0]), cigar, strand)
            f.write(b"@" + name.encode() + b"\n" + read + b"\n+\n" + bytes(40 + (i * 7 + r) % 30 for i in range(n)) + b"\n")
    return dict(genome=genome, genome_fa=g_fa, transcripts_fa=t_fa, fastq=fq, truth=truth, n_reads=n_reads,
                n_transcripts=len(transcripts))


def read_along(cigar, pos1):
    """genome coordinates (1-based) of the read bases of an M/N CIGAR"""
    out, g = [], pos1
    for n, op in re.findall(r"(\d+)([MN])", cigar):
        if op == "M":
            out += range(g, g + int(n))
        g += int(n)
    return out


def check_lifted(data, combined, transcript_recs):
    """check (b): every lifted record whose transcript hit is one M run lies where the generator cut the read, with the
    generator's M/N CIGAR, and its SEQ read along that CIGAR on the forward genome differs from the genome in at most NM
    bases.  combined = (text, refs, records) of the combined BAM; returns the counts the conditions are stated on."""
    _, refs, recs = combined[:3]
    t_by_name = {}
    for r in transcript_recs:
        assert r["name"] not in t_by_name            # bwa samse: one record per read
        t_by_name[r["name"]] = r
    n_lifted = n_checked = 0
    n_junction = {1: 0, -1: 0}
    for r in recs:
        t = t_by_name.get(r["name"])
        if t is None:
            continue
        n_lifted += 1
        if not re.fullmatch(r"\d+M", t["cigar"]):
            continue
        chrom, pos, cigar, strand = data["truth"][r["name"]]
        assert r["ref"] >= 0 and refs[r["ref"]][0] == chrom and r["pos"] + 1 == pos and r["cigar"] == cigar, (r, data["truth"][r["name"]])
        nm = [int(x[5:]) for x in r["tags"] if x.startswith("NM:i:")]
        assert len(nm) == 1
        g = data["genome"][chrom]
        along = read_along(cigar, pos)
        assert len(along) == len(r["seq"])
        assert sum(chr(g[p - 1]) != b for p, b in zip(along, r["seq"])) <= nm[0], (r, nm)
        n_checked += 1
        if "N" in cigar:
            n_junction[strand] += 1
    return dict(n_lifted=n_lifted, n_checked=n_checked, n_junction_fwd=n_junction[1], n_junction_rev=n_junction[-1])


def assert_conditions(c):
    """the conditions of check (b): conditions, not measurements -- a run with fewer fails"""
    assert c["n_junction_fwd"] >= 200 and c["n_junction_rev"] >= 200, c
    assert 2 * c["n_checked"] >= c["n_lifted"] > 0, c


def assert_at_most_once(data, recs):
    """check (c): every read of the input FASTQ appears in the combined BAM at most once"""
    seen = {}
    for r in recs:
        seen[r["name"]] = seen.get(r["name"], 0) + 1
    assert set(seen) <= set(data["truth"]) and max(seen.values()) == 1
