"""Counts and stage times of one ps_simulate_reads call (PS_VERBOSE=1, on stderr) on a generated FASTA of N transcripts of
LEN bases with the profile files of tests/golden, and the wall time of the plain-Python restatement (tests/perl_simulator.py)
on the first 1,000 of those transcripts -- the only runnable yardstick: the Perl needs a CPAN module that is not installed.
python tools/simulate_time.py [N] [LEN] [workdir]"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "para-suite_amd"), os.path.join(ROOT, "tests")]
import capi  # noqa: E402
import perl_simulator as P  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PROFILES = [os.path.join(GOLDEN, f) for f in ("example.errorprofile", "example.sitefrequency", "example.sitepositions", "example.qualities",
                                             "example.indels")]
SUFFIXES = (".fastq", ".clusters", "_snps.vsf", ".log", ".err")


def write_fasta(path, n, length, seed=0x51A7):
    """n single-exon transcripts, strands by turns, on 24 chromosomes; one sequence line each"""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for lo in range(0, n, 10000):
            rows = lut[rng.integers(0, 4, size=(min(10000, n - lo), length), dtype=np.uint8)]
            for k, row in enumerate(rows):
                t = lo + k
                start = 10000 + 3000 * (t // 24)
                f.write(b">g%d|tr%d|%d|%d|%d|%d\n" % (t, t, t % 24 + 1, start, start + length - 1, 1 if t % 2 == 0 else -1))
                f.write(row.tobytes() + b"\n")


def head(path, out, n):
    """the first n transcripts of a FASTA written by write_fasta"""
    with open(path, "rb") as f, open(out, "wb") as g:
        for _ in range(2 * n):
            g.write(f.readline())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    length = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    d = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="ps_simtime_")
    fa, small = os.path.join(d, "transcripts.fa"), os.path.join(d, "first1001.fa")
    t0 = time.perf_counter()
    write_fasta(fa, n, length)
    head(fa, small, min(n, 1001))
    print("%d transcripts x %d bases, %.1f MB, written in %.1f s" % (n, length, os.path.getsize(fa) / 1e6, time.perf_counter() - t0), flush=True)
    os.environ["PS_VERBOSE"] = "1"
    for tag, path in (("warm-up (first 1,001)", small), ("all", fa), ("all, again", fa)):
        t0 = time.perf_counter()
        st = capi.ps_simulate_reads(path, os.path.join(d, "gpu_" + tag[:3].strip()), *PROFILES, 0.6, 42)
        wall = time.perf_counter() - t0
        draws = 2 * st["n_snp_positions"] + 3 * st["n_snps_preselected"]   # one per position in each of the two passes, three more per SNP
        print("ps_simulate_reads, %s: %.3f s wall; %d reads, %d SNPs over %d positions; SNP kernels %.2f ms = %.1f G positions/s through both passes, %.1f G draws/s"
              % (tag, wall, st["n_reads"], st["n_snps_preselected"], st["n_snp_positions"], st["s_snp_kernels"] * 1e3,
                 st["n_snp_positions"] / max(st["s_snp_kernels"], 1e-9) / 1e9, draws / max(st["s_snp_kernels"], 1e-9) / 1e9), flush=True)
        for sfx in SUFFIXES:
            print("    %-10s %12d bytes" % (sfx, os.path.getsize(os.path.join(d, "gpu_" + tag[:3].strip()) + sfx)))
    del os.environ["PS_VERBOSE"]
    t0 = time.perf_counter()
    files, exp = P.simulate(open(small, "rb").read(), *[open(p, "rb").read() for p in PROFILES], 0.6, 42)
    t1 = time.perf_counter()
    same = all(files[sfx] == open(os.path.join(d, "gpu_war") + sfx, "rb").read() for sfx in SUFFIXES)
    print("tests/perl_simulator.py (plain Python) on the first 1,001 transcripts: %.2f s, %d reads, %d SNP positions; the five files equal the library's: %s"
          % (t1 - t0, exp["n_reads"], exp["n_snp_positions"], same))


if __name__ == "__main__":
    main()
