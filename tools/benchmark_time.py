"""Stage times of one ps_benchmark_reads call (PS_VERBOSE=1, on stderr) on N simulated 50 bp reads mapped by ps_map against
an 8 Mbp four-contig genome, and the wall time of the plain-Python restatement (tests/java_benchmark.py) on the same two
files -- the only runnable yardstick while no JVM is at hand.  python tools/benchmark_time.py [N] [workdir]"""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "para-suite_amd"), os.path.join(ROOT, "tests")]
import capi  # noqa: E402
import java_benchmark as J  # noqa: E402
import simulate as S  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    d = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="ps_benchtime_")
    fa, fq, sam, bam = (os.path.join(d, x) for x in ("mid.fa", "reads.fq", "reads.sam", "reads.bam"))
    g = S.big_genome(8_000_000, 4, seed=0x5EED0007)
    S.write_fasta(fa, g)
    S.write_fastq(fq, S.simulate_reads(g, n, 50, seed=1234, indel_scale=30))
    capi.ps_index(fa)
    capi.ps_map(8, "2", None, None, fa, fq, sam)
    capi.ps_sam_to_bam(sam, bam)
    print("%d reads; FASTQ %.1f MB, SAM %.1f MB, BAM %.1f MB" % (n, *(os.path.getsize(p) / 1e6 for p in (fq, sam, bam))), flush=True)
    os.environ["PS_VERBOSE"] = "1"
    stats = {}
    for tag, mapping in (("warm-up (SAM)", sam), ("SAM", sam), ("BAM", bam)):
        t0 = time.perf_counter()
        stats[tag] = capi.ps_benchmark_reads(mapping, os.path.join(d, "gpu.stats"), fq)
        print("ps_benchmark_reads, %s: %.3f s wall" % (tag, time.perf_counter() - t0), flush=True)
    del os.environ["PS_VERBOSE"]
    t0 = time.perf_counter()
    sam_text, fq_bytes = open(sam).read(), open(fq, "rb").read()
    t1 = time.perf_counter()
    text, exp = J.benchmark(sam_text, fq_bytes)
    t2 = time.perf_counter()
    print("tests/java_benchmark.py on the same SAM and FASTQ: %.2f s to read the files, %.2f s to count" % (t1 - t0, t2 - t1))
    same = text == open(os.path.join(d, "gpu.stats"), "rb").read() and all(J.same_stats(s, exp) is None for s in stats.values())
    print("statistics file and counters equal: %s\n%s" % (same, text.decode()))


if __name__ == "__main__":
    main()
