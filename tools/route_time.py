#!/usr/bin/env python3
"""route_time.py -- what the whole `map --refine -t` route costs call by call and as ONE call (measurement aid).

  python tools/route_time.py prepare DIR [--genome-bp 1000000000 --reads 4000000 --transcripts 3000]
        a simulate.big_genome, transcripts cut from it with the header format of tests/combine_route.py, the reads (two thirds
        from the genome with T->C conversions, one third from the transcripts), and both indexes (GPU)
  python tools/route_time.py run DIR --how steps     the route through ps_map_to_bam, ps_error_profile, ps_extract_weak_reads,
        ps_bam_sort, ps_bam_index, ps_combine_genome_transcript -- calls a build without ps_map_route has too (PARASUITE_LIB
        names such a build: the baseline is the commit before ps_map_route, never this tree's own steps)
  python tools/route_time.py run DIR --how call      ps_map_route

One run per process (a fresh process each time, in turn); PS_VERBOSE=1 stage lines go to stderr; the last line of stdout is
`route_time how=... seconds=...`."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "para-suite_amd")):
    sys.path.insert(0, p)

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def prepare(d, genome_bp, n_reads, n_transcripts):
    import capi
    import simulate as S
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0x520C7E)
    genome = S.big_genome(genome_bp, 8)
    g_fa, t_fa, fq = (os.path.join(d, x) for x in ("genome.fa", "transcripts.fa", "reads.fq"))
    S.write_fasta(g_fa, genome)
    print("genome written", flush=True)
    # transcripts: 2-4 exons of 30-80 bases, introns of 40-200, every other one on strand -1; all exon coordinates of a
    # transcript have the same number of digits, so the Java's string sort of the exon lists and the numeric order agree
    transcripts = []
    while len(transcripts) < n_transcripts:
        c = int(rng.integers(0, len(genome)))
        asc = genome[c][1]
        lo = 10 ** (len(str(asc.size - 2000)) - 1)
        at = int(rng.integers(lo, asc.size - 2000))
        starts, ends = [], []
        for _ in range(int(rng.integers(2, 5))):
            n = int(rng.integers(30, 81))
            starts.append(at); ends.append(at + n - 1)
            at += n + int(rng.integers(40, 201))
        seq = b"".join(asc[s - 1:e].tobytes() for s, e in zip(starts, ends)).upper()
        if b"N" in seq:
            continue
        k = len(transcripts)
        strand = -1 if k & 1 else 1
        head = "GENE%d|TR%d|%d|%s|%s|%d" % (k, k, c + 1, ";".join(map(str, starts)), ";".join(map(str, ends)), strand)
        transcripts.append((head, seq if strand == 1 else seq.translate(_COMP)[::-1]))
    with open(t_fa, "wb") as f:
        for head, seq in transcripts:
            f.write(b">" + head.encode() + b"\n" + seq + b"\n")
    print("transcripts written", flush=True)
    n_t = n_reads // 3
    sim = S.simulate_reads(genome, n_reads - n_t, 50, seed=0x520C7F, bound=0.6, min_len=36)
    S.write_fastq(fq, sim, names=["g%d" % i for i in range(n_reads - n_t)])
    with open(fq, "ab") as f:
        pick = rng.integers(0, len(transcripts), size=n_t); ln = rng.integers(36, 51, size=n_t); u = rng.random(n_t); rc = rng.random(n_t) < 0.5
        out = []
        for i in range(n_t):
            seq = transcripts[int(pick[i])][1]
            n = int(ln[i]); o = int(u[i] * (len(seq) - n + 1))
            read = seq[o:o + n]
            if rc[i]:
                read = read.translate(_COMP)[::-1]
            out.append(b"@t%d\n%s\n+\n%s\n" % (i, read, b"I" * n))
            if len(out) == 200000:
                f.write(b"".join(out)); out = []
        f.write(b"".join(out))
    print("reads written", flush=True)
    t0 = time.time()
    capi.ps_index(g_fa)
    capi.ps_index(t_fa)
    print("prepared %s: %d bp genome, %d transcripts, %d reads; both indexes in %.1f s" % (d, genome_bp, n_transcripts, n_reads, time.time() - t0), flush=True)


def run(d, how, threads):
    try:
        import torch  # noqa: F401  (before the library)
    except ImportError:
        pass
    import capi
    os.environ["PS_VERBOSE"] = "1"
    g_fa, t_fa, fq = (os.path.join(d, x) for x in ("genome.fa", "transcripts.fa", "reads.fq"))
    out = os.path.join(d, "out." + how)
    os.makedirs(out, exist_ok=True)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    P = os.path.join(out, "o")
    t0 = time.time()
    if how == "call":
        st = capi.ps_map_route(fq, g_fa, P, transcripts_fa=t_fa, threads=threads, refine=True)
        print({k: v for k, v in st.items() if not isinstance(v, dict)}, st["extract"], st["combine"])
    else:
        first, second, weak = P + ".BWA-genomic.bam", P + ".PARAsuite-genomic.bam", P + ".unaligned.fastq"
        tr = P + ".PARAsuite-transcript.bam"

        def sort_index(bam, by_name=False):
            capi.ps_bam_sort(bam, bam + ".sorted", by_name=by_name, threads=threads)
            os.replace(bam + ".sorted", bam)
            if not by_name:
                capi.ps_bam_index(bam, threads=threads)

        capi.ps_map_to_bam(threads, "2", None, None, g_fa, fq, first, min_mapq=10)
        sort_index(first)
        capi.ps_error_profile(first, g_fa, 101, None)
        ep, ip = first + ".errorprofile", first + ".indelprofile"
        capi.ps_map_to_bam(threads, "-1", ep, ip, g_fa, fq, second, min_mapq=0)
        print(capi.ps_extract_weak_reads(second, second + ".new", weak, 10, threads=threads))
        os.replace(second + ".new", second)
        sort_index(second)
        capi.ps_map_to_bam(threads, "-1", ep, ip, t_fa, weak, tr, min_mapq=1)
        sort_index(tr, by_name=True)
        os.remove(weak)
        print(capi.ps_combine_genome_transcript(second, tr, P + ".combined.bam", True, True, threads=threads))
    dt = time.time() - t0
    sizes = {f: os.path.getsize(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    print(sizes)
    print("route_time how=%s seconds=%.3f" % (how, dt), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["prepare", "run"])
    ap.add_argument("dir")
    ap.add_argument("--genome-bp", type=int, default=1_000_000_000)
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--transcripts", type=int, default=3000)
    ap.add_argument("--how", choices=["steps", "call"], default="call")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    prepare(a.dir, a.genome_bp, a.reads, a.transcripts) if a.what == "prepare" else run(a.dir, a.how, a.threads)
