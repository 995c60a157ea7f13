#!/usr/bin/env python3
"""combine_time.py -- stage times of ps_combine_genome_transcript at a size a user would run (measurement aid).

  python tools/combine_time.py prepare DIR --records 3000000    the two input BAMs (host code only)
  python tools/combine_time.py run DIR [--sorted 1] [--calls 2]  the call, PS_VERBOSE=1 stage times on stderr
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/combine_time.py run DIR --calls 1      the kernels, in a run of its own

The transcripts are those of tests/combine_route.py (264 transcripts of 2-4 exons on three contigs, every other one on strand
-1); the transcript file holds --records hits of 36-50 bp reads at random transcript positions, name-sorted, one read in five
with a second hit (0x100) -- half of those on the same spot, half elsewhere -- and one record in fifty without a reference;
the genomic file holds half as many records.  The bases are random: the call never looks at the genome."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "para-suite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def _seqs(rng, n, length):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, length))].view("S%d" % length).ravel().tolist()


def prepare(d, n_records):
    import capi
    import combine_route as R
    os.makedirs(d, exist_ok=True)
    data = R.make_data(d, n_reads=1)
    heads, lens = [], []
    for line in open(data["transcripts_fa"]):
        if line.startswith(">"):
            heads.append(line[1:].strip()); lens.append(0)
        else:
            lens[-1] += len(line.strip())
    rng = np.random.default_rng(7)
    qual = b"I" * 50
    with open(os.path.join(d, "t.sam"), "wb") as f:
        f.write(b"@HD\tVN:1.6\tSO:queryname\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (h.encode(), n) for h, n in zip(heads, lens)))
        n, read = 0, 0
        while n < n_records:
            m = min(200000, n_records - n)
            tr = rng.integers(0, len(heads), size=m); ln = rng.integers(36, 51, size=m); u = rng.random(m); v = rng.random(m)
            seqs = _seqs(rng, m, 50)
            out = []
            for i in range(m):
                t = int(tr[i]); L = int(ln[i]); pos = 1 + int(v[i] * (lens[t] - L + 1)); name = b"read%09d" % read
                if u[i] < 0.02:
                    out.append(b"%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (name, seqs[i][:L], qual[:L]))
                else:
                    out.append(b"%s\t%d\t%s\t%d\t25\t%dM\t*\t0\t0\t%s\t%s\tXT:A:U\tNM:i:1\tX0:i:1\n" % (name, 16 if u[i] > 0.5 else 0, heads[t].encode(), pos, L, seqs[i][:L], qual[:L]))
                    if 0.02 <= u[i] < 0.22:
                        pos2 = pos if u[i] < 0.12 else 1 + (pos + 3) % (lens[t] - L + 1)
                        out.append(b"%s\t256\t%s\t%d\t0\t%dM\t*\t0\t0\t%s\t%s\tNM:i:2\n" % (name, heads[t].encode(), pos2, L, seqs[i][:L], qual[:L]))
                read += 1
            f.write(b"".join(out))
            n += len(out)
    with open(os.path.join(d, "g.sam"), "wb") as f:
        f.write(b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (k.encode(), len(s)) for k, s in data["genome"].items()))
        for a in range(0, n_records // 2, 200000):
            m = min(200000, n_records // 2 - a)
            c = rng.integers(1, 4, size=m); pos = rng.integers(1, 99000, size=m); seqs = _seqs(rng, m, 50)
            f.write(b"".join(b"g%09d\t0\tchr%d\t%d\t37\t50M\t*\t0\t0\t%s\t%s\tXT:A:U\tNM:i:0\n" % (a + i, c[i], pos[i], seqs[i], qual) for i in range(m)))
    for x in ("g", "t"):
        st = capi.ps_sam_to_bam(os.path.join(d, x + ".sam"), os.path.join(d, x + ".bam"), threads=16)
        os.remove(os.path.join(d, x + ".sam"))
        print("prepared %s.bam: %d records, %d bytes" % (x, st["n_out"], st["bam_bytes"]), flush=True)


def run(d, want_sorted, calls):
    try:
        import torch  # noqa: F401  (before the library)
    except ImportError:
        pass
    import capi
    os.environ["PS_VERBOSE"] = "1"
    for k in range(calls):
        t0 = time.time()
        st = capi.ps_combine_genome_transcript(os.path.join(d, "g.bam"), os.path.join(d, "t.bam"), os.path.join(d, "c.bam"),
                                               sort_by_coordinate=want_sorted, write_index=want_sorted, threads=16)
        print("call %d (%s): %.3f s wall; %s" % (k, "sorted + .bai" if want_sorted else "unsorted", time.time() - t0, st), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["prepare", "run"])
    ap.add_argument("dir")
    ap.add_argument("--records", type=int, default=3_000_000)
    ap.add_argument("--sorted", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2)
    a = ap.parse_args()
    prepare(a.dir, a.records) if a.what == "prepare" else run(a.dir, bool(a.sorted), a.calls)
