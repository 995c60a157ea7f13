#!/usr/bin/env python3
"""gzip_time.py -- ps_map on the same reads as plain FASTQ, as .fq.gz and as BGZF (measurement aid for csrc/ps_inflate.h).

  python tools/gzip_time.py prepare DIR [--reads 10000000 --genome-mbp 3100]
        the inputs as tools/e2e_time.py makes them (genome in 8 contigs, 50 bp reads with indels, profile costs), the index (GPU),
        and the reads three times: reads.fq, reads.fq.gz (one member, zlib level 6) and reads.fq.bgzf (level 6)
  python tools/gzip_time.py run DIR --form plain|gz|bgzf [--calls 3]
        ps_map (16 threads, -X -1) `calls` times in this process; PARASUITE_LIB names another build of the library (the plain
        runs of the commit before)

One run per process (a fresh process each time, the builds or forms in turn); PS_VERBOSE=1 stage lines go to stderr; stdout holds
one line `gzip_time form=... call=... seconds=... sam_md5=...` per call."""
import argparse
import hashlib
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "para-suite_amd")):
    sys.path.insert(0, p)

NAMES = {"plain": "reads.fq", "gz": "reads.fq.gz", "bgzf": "reads.fq.bgzf"}


def _bgzf_block(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", 18 + len(body) + 8 - 1) + body
            + struct.pack("<II", zlib.crc32(data), len(data)))


def prepare(d, n, mbp):
    import torch
    import bench
    import capi
    os.makedirs(d, exist_ok=True)
    dev = torch.device("cuda", 0)
    contigs = bench.gen_genome(torch, dev, mbp * 1_000_000, 8, 0x5EED0002)
    fa, fq = os.path.join(d, "genome.fa"), os.path.join(d, NAMES["plain"])
    bench.write_fasta(fa, contigs)
    rd = bench.gen_reads(torch, dev, contigs, n, 50, 0x5EED0003, indels=True)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    name = np.char.zfill(np.arange(n).astype(str), 9).astype("S9").view(np.uint8).reshape(n, 9)
    rec = np.empty((n, 1 + 9 + 1 + 50 + 3 + 50 + 1), dtype=np.uint8)     # fixed-width records, as tools/e2e_time.py writes them
    rec[:, 0] = ord("@"); rec[:, 1:10] = name; rec[:, 10] = 10; rec[:, 11:61] = lut[rd]; rec[:, 61] = 10; rec[:, 62] = ord("+"); rec[:, 63] = 10
    rec[:, 64:114] = ord("I"); rec[:, 114] = 10
    text = rec.tobytes()
    del rec, contigs, rd
    open(fq, "wb").write(text)
    t0 = time.time()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(os.path.join(d, NAMES["gz"]), "wb") as f:
        for a in range(0, len(text), 64 << 20):
            f.write(c.compress(text[a:a + (64 << 20)]))
        f.write(c.flush())
    t1 = time.time()
    with ThreadPoolExecutor(16) as ex, open(os.path.join(d, NAMES["bgzf"]), "wb") as f:      # zlib releases the interpreter lock
        for blk in ex.map(lambda a: _bgzf_block(text[a:a + 0xff00], 6), range(0, len(text), 0xff00)):
            f.write(blk)
        f.write(bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    print("compressed in %.1f + %.1f s: %s" % (t1 - t0, time.time() - t1, {k: os.path.getsize(os.path.join(d, v)) for k, v in NAMES.items()}), flush=True)
    t0 = time.time()
    capi.ps_index(fa)
    print("ps_index %.1f s" % (time.time() - t0), flush=True)
    P = np.array(bench.PROFILE); P[3, 1], P[3, 3] = 0.12, 0.87
    with open(os.path.join(d, "in.errorprofile"), "w") as f:
        for row in P:
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    open(os.path.join(d, "in.indelprofile"), "w").write("2.1E-5\t5.9E-4")


def run(d, form, calls, threads):
    try:
        import torch  # noqa: F401  (before the library)
    except ImportError:
        pass
    import capi
    os.environ["PS_VERBOSE"] = "1"
    sam = os.path.join(d, "out.sam")
    for k in range(calls):
        t0 = time.time()
        capi.ps_map(threads, "-1", os.path.join(d, "in.errorprofile"), os.path.join(d, "in.indelprofile"), os.path.join(d, "genome.fa"),
                    os.path.join(d, NAMES[form]), sam)
        dt = time.time() - t0
        h = hashlib.md5()
        with open(sam, "rb") as f:
            for blk in iter(lambda: f.read(64 << 20), b""):
                h.update(blk)
        print("gzip_time form=%s call=%d seconds=%.3f sam_md5=%s" % (form, k + 1, dt, h.hexdigest()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["prepare", "run"])
    ap.add_argument("dir")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-mbp", type=int, default=3100)
    ap.add_argument("--form", choices=sorted(NAMES), default="plain")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    prepare(a.dir, a.reads, a.genome_mbp) if a.what == "prepare" else run(a.dir, a.form, a.calls, a.threads)
