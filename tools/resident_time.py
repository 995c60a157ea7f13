#!/usr/bin/env python3
"""resident_time.py -- what a resident scope (ps_resident_begin / _end) saves call by call (measurement aid).

  python tools/route_time.py prepare DIR [--genome-bp ... --reads ... --transcripts ...]      the data and both indexes
  python tools/resident_time.py run DIR --what map   --scope 0|1     three successive ps_map calls on DIR's genome and reads
  python tools/resident_time.py run DIR --what route --scope 0|1     the call-by-call route of tools/route_time.py (`--how steps`)
  python tools/resident_time.py ab DIR [--out FILE]                  the four runs above in fresh processes, in turn, and a table

`run` is one process; every library call in it runs under a time limit of its own (--limit seconds: the process ends with status
124 when a call overruns it) and prints `call <name> seconds=...`.  `ab` stops at the first run that fails."""
import argparse
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "para-suite_amd")):
    sys.path.insert(0, p)


def timed(name, limit, fn, *args, **kw):
    def overrun():                             # on a thread of its own: the library call holds the main thread
        print("call %s overran its limit of %d s" % (name, limit), flush=True)
        os._exit(124)
    watch = threading.Timer(limit, overrun)
    watch.daemon = True
    watch.start()
    t0 = time.time()
    out = fn(*args, **kw)
    dt = time.time() - t0
    watch.cancel()
    print("call %s seconds=%.3f" % (name, dt), flush=True)
    return out


def run(d, what, scope, threads, limit):
    try:
        import torch  # noqa: F401  (before the library)
    except ImportError:
        pass
    import capi
    g_fa, t_fa, fq = (os.path.join(d, x) for x in ("genome.fa", "transcripts.fa", "reads.fq"))
    out = os.path.join(d, "out.resident.%s.%d" % (what, scope))
    os.makedirs(out, exist_ok=True)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    P = os.path.join(out, "o")
    t0 = time.time()
    if scope:
        capi.ps_resident_begin(2)
    if what == "map":
        for k in range(3):
            timed("ps_map_%d" % (k + 1), limit, capi.ps_map, threads, "2", None, None, g_fa, fq, P + ".%d.sam" % k)
    else:
        first, second, weak = P + ".BWA-genomic.bam", P + ".PARAsuite-genomic.bam", P + ".unaligned.fastq"
        tr = P + ".PARAsuite-transcript.bam"

        def sort_index(bam, by_name=False):
            capi.ps_bam_sort(bam, bam + ".sorted", by_name=by_name, threads=threads)
            os.replace(bam + ".sorted", bam)
            if not by_name:
                capi.ps_bam_index(bam, threads=threads)

        timed("map_first", limit, capi.ps_map_to_bam, threads, "2", None, None, g_fa, fq, first, min_mapq=10)
        timed("sort_first", limit, sort_index, first)
        timed("profile", limit, capi.ps_error_profile, first, g_fa, 101, None)
        ep, ip = first + ".errorprofile", first + ".indelprofile"
        timed("map_refine", limit, capi.ps_map_to_bam, threads, "-1", ep, ip, g_fa, fq, second, min_mapq=0)
        timed("extract", limit, capi.ps_extract_weak_reads, second, second + ".new", weak, 10, threads=threads)
        os.replace(second + ".new", second)
        timed("sort_refine", limit, sort_index, second)
        timed("map_transcripts", limit, capi.ps_map_to_bam, threads, "-1", ep, ip, t_fa, weak, tr, min_mapq=1)
        timed("sort_transcripts", limit, sort_index, tr, True)
        os.remove(weak)
        timed("combine", limit, capi.ps_combine_genome_transcript, second, tr, P + ".combined.bam", True, True, threads=threads)
    if scope:
        print("resident", capi.ps_resident_info(), flush=True)
        timed("ps_resident_end", limit, capi.ps_resident_end)
    print("resident_time what=%s scope=%d seconds=%.3f" % (what, scope, time.time() - t0), flush=True)


def ab(d, threads, limit, out_path):
    rows = []
    for what in ("map", "route"):
        for scope in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), "run", d, "--what", what, "--scope", str(scope), "--threads", str(threads), "--limit", str(limit)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=12 * limit)
            lines = [l for l in r.stdout.splitlines() if l.startswith(("call ", "resident"))]
            print("\n".join(lines), flush=True)
            if r.returncode != 0:
                print("run what=%s scope=%d ended with status %d: stopping" % (what, scope, r.returncode), flush=True)
                sys.exit(1)
            rows.append((what, scope, [(l.split()[1], float(l.split("seconds=")[1])) for l in lines if l.startswith("call ")],
                         float(lines[-1].split("seconds=")[1])))
    text = []
    for what in ("map", "route"):
        a, b = ([r for r in rows if r[0] == what and r[1] == s][0] for s in (0, 1))
        text.append("%-18s %12s %12s" % (what, "no scope", "in a scope"))
        inside = dict(b[2])
        for name, sec in a[2]:
            text.append("  %-16s %10.3f s %10.3f s" % (name, sec, inside[name]))
        if "ps_resident_end" in inside:
            text.append("  %-16s %12s %10.3f s" % ("ps_resident_end", "", inside["ps_resident_end"]))
        text.append("  %-16s %10.3f s %10.3f s" % ("whole process", a[3], b[3]))
    text = "\n".join(text)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["run", "ab"])
    ap.add_argument("dir")
    ap.add_argument("--what", choices=["map", "route"], default="map")
    ap.add_argument("--scope", type=int, choices=[0, 1], default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    run(a.dir, a.what, a.scope, a.threads, a.limit) if a.cmd == "run" else ab(a.dir, a.threads, a.limit, a.out)
