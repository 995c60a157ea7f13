"""The name sort of one batch's BAM records in isolation: the host route (ps_bam.cpp: one std::stable_sort on one thread under the
`samtools sort -n` comparator, then the gather on 16 threads) against the device route (ps_bamsort.hip: records up, the rows of
ps_namesort.h, one radix sort per column that differs, offsets, gather kernel, permutation and stream down) through
ps_bam_name_sort_records on the same records in one process, alternating.  The corpus of tools/bam_sort_time.py: simulated 50 bp
reads on a simulated genome, located once, their records (MAPQ >= 0) built once by the device route; the names are the reads'
numbers, zero padded to nine digits.  ORDER=input leaves the records as the mapper emits them, which is name order already -- the
host sort's best case and what the transcript pass of ps_map_route hands it; ORDER=shuffled permutes them first.  Median and range of
RUNS timed pairs after a warm-up pair, with the device route's five parts, key_words and n_passes (ps_bam_name_sort_stats).  The two
routes' bytes are compared once, outside the timing.  Both routes end with one copy of the sorted stream into this script's buffer.

    python tools/bam_name_sort_time.py [N_READS=1000000] [GENOME_MBP=100] [RUNS=5] [WORKDIR=/tmp] [ORDER=input|shuffled]"""
import ctypes as C, os, statistics, sys, time
import numpy as np
sys.path.insert(0, 'para-suite_amd'); sys.path.insert(0, '.')
import torch, capi, bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
mbp = int(sys.argv[2]) if len(sys.argv) > 2 else 100
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
work = sys.argv[4] if len(sys.argv) > 4 else '/tmp'
order = sys.argv[5] if len(sys.argv) > 5 else 'input'
assert order in ('input', 'shuffled')
p = lambda x: os.path.join(work, 'bam_name_sort_time.' + x)

dev = torch.device('cuda', 0)
contigs = bench.gen_genome(torch, dev, mbp * 1_000_000, 8, 0x5EED0002)
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
records, _, st_r = b.bam_records(0, True, 16)
b.free()
if order == 'shuffled':
    raw = np.frombuffer(records, dtype=np.uint8)
    at, cuts = 0, []
    while at < len(raw):
        step = 4 + int(raw[at:at + 4].view('<u4')[0])
        cuts.append((at, step)); at += step
    records = b''.join(raw[cuts[k][0]:cuts[k][0] + cuts[k][1]].tobytes() for k in np.random.default_rng(0x5EED0004).permutation(len(cuts)))
    del raw, cuts
lib = capi.lib()
size = len(records)
dst = {-1: np.zeros(size, dtype=np.uint8), 0: np.zeros(size, dtype=np.uint8)}
print('%d records, %.1f MB, %s order' % (st_r['n_records'], size / 1e6, order), flush=True)


def once(device):
    st = capi.BamNameSortStats(struct_size=C.sizeof(capi.BamNameSortStats))
    t0 = time.perf_counter()
    got = lib.ps_bam_name_sort_records(records, size, device, 16, dst[device].ctypes.data, size, C.byref(st))
    dt = time.perf_counter() - t0
    assert got == size, lib.ps_last_error()
    return dt, st


f = lambda v: '%.1f ms (%.1f to %.1f)' % (1e3 * statistics.median(v), 1e3 * min(v), 1e3 * max(v))
g = lambda v: '%.1f (%.1f to %.1f)' % (statistics.median(v), min(v), max(v))
t_host, t_dev, parts = [], [], dict(ms_upload=[], ms_keys=[], ms_sort=[], ms_gather=[], ms_download=[])
for r in range(runs + 1):                       # the first pair is the warm-up
    dh, _ = once(-1)
    dd, st = once(0)
    if r == 0:
        assert dst[-1].tobytes() == dst[0].tobytes(), 'the two routes differ'
    else:
        t_host.append(dh); t_dev.append(dd)
        for k in parts:
            parts[k].append(getattr(st, k))
print('median (range) of %d alternating pairs: host route (stable sort on one thread, gather on 16) %s; device route %s, of it in ms: upload %s, names + rows %s, column sorts %s, offsets + gather %s, download %s; key_words %d, n_passes %d'
      % (runs, f(t_host), f(t_dev), g(parts['ms_upload']), g(parts['ms_keys']), g(parts['ms_sort']), g(parts['ms_gather']), g(parts['ms_download']), st.key_words, st.n_passes), flush=True)
