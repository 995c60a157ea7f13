"""The BAM records of one located batch in isolation: the host route (ps_records.hip's bam_record on 16 threads) against the device
route (ps_bamrec.hip: inputs up, size kernel, host-built records spliced in, scan, fill kernel, stream down, offsets walked) on
the same batch in one process, alternating.  Simulated 50 bp reads on a simulated genome, located once; both routes run through
ps_batch_bam_records with dst NULL, so neither pays a copy into a buffer of this script.  Median and range of RUNS timed
runs after a warm-up, at MAPQ >= 0 and MAPQ >= 10, with the device route's four parts (ps_bam_records_stats) and the share of
reads whose records the host had to build.  The bytes of both routes are compared once, outside the timing.

    python tools/bamrec_time.py [N_READS=1000000] [GENOME_MBP=100] [RUNS=5] [WORKDIR=/tmp] [REPEATS=0 | 1: bench.add_repeats lays a mammalian repeat structure over the genome, as tests/test_gpu_repeats.py does]"""
import ctypes as C, os, statistics, sys, time
import numpy as np
sys.path.insert(0, 'para-suite_amd'); sys.path.insert(0, '.')
import torch, capi, bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
mbp = int(sys.argv[2]) if len(sys.argv) > 2 else 100
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
work = sys.argv[4] if len(sys.argv) > 4 else '/tmp'
repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 0
p = lambda x: os.path.join(work, 'bamrec_time.' + x)

dev = torch.device('cuda', 0)
contigs = bench.gen_genome(torch, dev, mbp * 1_000_000, 8, 0x5EED0002)
if repeats:                                     # ~45 % of the bases inside repeat copies: more reads with several best intervals, which the host finishes
    contigs = bench.add_repeats(torch, dev, contigs, 0x5EED0209)
bench.write_fasta(p('fa'), contigs)
rd = bench.gen_reads(torch, dev, contigs, n, 50, 0x5EED0003, indels=True)
lut = np.frombuffer(b"ACGT", dtype=np.uint8)
name = np.char.zfill(np.arange(n).astype(str), 9).astype('S9').view(np.uint8).reshape(n, 9)
rec = np.empty((n, 1 + 9 + 1 + 50 + 3 + 50 + 1), dtype=np.uint8)
rec[:, 0] = ord('@'); rec[:, 1:10] = name; rec[:, 10] = 10; rec[:, 11:61] = lut[rd]; rec[:, 61] = 10; rec[:, 62] = ord('+'); rec[:, 63] = 10
rec[:, 64:114] = (33 + 2 + (np.arange(n * 50, dtype=np.uint64) * 2654435761 >> 13) % 39).astype(np.uint8).reshape(n, 50); rec[:, 114] = 10
open(p('fq'), 'wb').write(rec.tobytes())
del rec, rd, contigs
ctx = capi.Ctx.build(p('fa'), device=0)
P = np.array(bench.PROFILE); P[3, 1], P[3, 3] = 0.12, 0.87
ctx.set_profile(P, 2.1e-5, 5.9e-4, -1)
b = ctx.batch_from_fastq(p('fq'))
t = time.perf_counter(); b.run(16); print('%d reads located in %.2f s' % (b.n, time.perf_counter() - t), flush=True)
lib = capi.lib()


def once(q, on_device):
    st = capi.BamRecordsStats()
    t0 = time.perf_counter()
    got = lib.ps_batch_bam_records(b.h, q, on_device, 16, None, 0, None, C.byref(st))
    dt = time.perf_counter() - t0
    assert got >= 0, lib.ps_last_error()
    return dt, st


f = lambda v: '%.1f ms (%.1f to %.1f)' % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
g = lambda v: '%.1f (%.1f to %.1f)' % (statistics.median(v), min(v), max(v))
for q in (0, 10):
    dev_b, _, st_d = b.bam_records(q, True, 16)
    host_b, _, _ = b.bam_records(q, False, 16)
    assert dev_b == host_b, 'the two routes differ at MAPQ >= %d' % q
    t_host, t_dev, parts = [], [], dict(ms_upload=[], ms_kernels=[], ms_host_records=[], ms_download=[])
    for r in range(runs + 1):                   # the first pair is the warm-up
        dh, _ = once(q, 0)
        dd, st = once(q, 1)
        if r:
            t_host.append(dh); t_dev.append(dd)
            for k in parts:
                parts[k].append(getattr(st, k))
    print('MAPQ >= %d: %d reads, %d records, %.1f MB; built by the host in the device route: %d records (%.3f %% of the reads\' records)'
          % (q, b.n, st_d['n_records'], st_d['bytes'] / 1e6, st_d['n_host'], 100.0 * st_d['n_host'] / max(1, st_d['n_records'])))
    print('MAPQ >= %d: median (range) of %d: host route on 16 threads %s; device route %s, of it in ms: upload %s, kernels %s, host-built records %s, download and offset walk %s'
          % (q, runs, f(t_host), f(t_dev), g(parts['ms_upload']), g(parts['ms_kernels']), g(parts['ms_host_records']), g(parts['ms_download'])), flush=True)
