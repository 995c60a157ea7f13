"""tools/e2e_time.py's fused route alone, with and without the BGZF switch: FASTQ -> MAPQ-filtered BAM through ps_map_to_bam
(index load + search + records + BGZF + file written), unsorted and sorted + indexed, zlib level 1 on 16 threads against the
device compressor.  PS_VERBOSE=1 prints the stage times of each call, where the compress launches queue behind the search.
SWITCH=records alternates the BAM records' device route (ps_bam_records_device) instead, BGZF on host zlib throughout: the off runs
of the same command are the reference.  SWITCH=sort alternates the coordinate sort's device route (ps_bam_sort_device) the same way, on
the sorted + indexed call alone (the unsorted file never sorts); the stage lines of both routes come with PS_VERBOSE.  SWITCH=sort+bgzf
is the same with the device compressor on throughout, so that the on runs leave the sorted stream on the device for it.
SWITCH=namesort writes the unsorted MAPQ-filtered BAM once and then times ps_bam_sort by name on it (`samtools sort -n`), the name
sort's device route (ps_bam_name_sort_device) off and on in turn; SWITCH=namesort+bgzf the same with the device compressor on throughout.

    python tools/e2e_bam_time.py [N_READS=10000000] [GENOME_MBP=1000] [WORKDIR=/tmp] [SWITCH=bgzf|records|sort|sort+bgzf|namesort|namesort+bgzf]"""
import os, sys, time
import numpy as np
sys.path.insert(0, 'para-suite_amd'); sys.path.insert(0, '.')
import torch, capi, bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
mbp = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
work = sys.argv[3] if len(sys.argv) > 3 else '/tmp'
switch = sys.argv[4] if len(sys.argv) > 4 else 'bgzf'
assert switch in ('bgzf', 'records', 'sort', 'sort+bgzf', 'namesort', 'namesort+bgzf')
resident = switch.endswith('+bgzf')
if resident:
    switch = switch[:-len('+bgzf')]
    capi.ps_bgzf_device(0)
p = lambda x: os.path.join(work, 'e2e_bam.' + x)
dev = torch.device('cuda', 0)
contigs = bench.gen_genome(torch, dev, mbp * 1_000_000, 8, 0x5EED0002)
bench.write_fasta(p('fa'), contigs); print('genome written', flush=True)
rd = bench.gen_reads(torch, dev, contigs, n, 50, 0x5EED0003, indels=True)
lut = np.frombuffer(b"ACGT", dtype=np.uint8)
name = np.char.zfill(np.arange(n).astype(str), 9).astype('S9').view(np.uint8).reshape(n, 9)
rec = np.empty((n, 1 + 9 + 1 + 50 + 3 + 50 + 1), dtype=np.uint8)
rec[:, 0] = ord('@'); rec[:, 1:10] = name; rec[:, 10] = 10; rec[:, 11:61] = lut[rd]; rec[:, 61] = 10; rec[:, 62] = ord('+'); rec[:, 63] = 10
rec[:, 64:114] = ord('I'); rec[:, 114] = 10
open(p('fq'), 'wb').write(rec.tobytes()); print('reads written', flush=True)
del rec, rd, contigs
t = time.time(); capi.ps_index(p('fa')); print('ps_index %.1fs' % (time.time() - t), flush=True)
P = np.array(bench.PROFILE); P[3, 1], P[3, 3] = 0.12, 0.87
with open(p('errorprofile'), 'w') as f:
    for row in P: f.write(''.join(repr(float(v)) + '\t' for v in row) + '\n')
open(p('indelprofile'), 'w').write('2.1E-5\t5.9E-4')
os.environ['PS_BAM_LEVEL'] = '1'
os.environ['PS_VERBOSE'] = os.environ.get('E2E_VERBOSE', '1')
LABEL = dict(bgzf=('zlib level 1 on 16 threads', 'BGZF on device 0'), records=('records built on 16 host threads', 'records built on the device'),
             sort=('records sorted and gathered on the host' + ', BGZF on device 0' * resident, 'records sorted and gathered on device 0' + ', the stream left there for BGZF on device 0' * resident))
if switch == 'namesort':
    st = capi.ps_map_to_bam(16, '-1', p('errorprofile'), p('indelprofile'), p('fa'), p('fq'), p('bam'), min_mapq=10)
    print('ps_map_to_bam: %d of %d records kept, BAM %.0f MB' % (st['n_out'], st['n_in'], st['bam_bytes'] / 1e6), flush=True)
    for device in (-1, 0) * 5:
        capi.ps_bam_name_sort_device(device)
        t = time.time(); st = capi.ps_bam_sort(p('bam'), p('byname.bam'), by_name=True, threads=16); dt = time.time() - t
        print('ps_bam_sort by name, %s: %.2fs, %d records, BAM %.0f MB' % (LABEL['sort'][device >= 0], dt, st['n_out'], st['bam_bytes'] / 1e6), flush=True)
    capi.ps_bam_name_sort_device(-1)
for kw in () if switch == 'namesort' else (dict(min_mapq=10), dict(min_mapq=10, sort_by_coordinate=True, write_index=True))[1 if switch == 'sort' else 0:]:
    for device in (-1, 0) * 5:                       # the first pair warms the page cache and the page-locked buffers up; four timed pairs
        if switch == 'bgzf':
            capi.ps_bgzf_device(device)
        elif switch == 'records':
            capi.ps_bam_records_device(device >= 0)
        else:
            capi.ps_bam_sort_device(device)
        t = time.time(); st = capi.ps_map_to_bam(16, '-1', p('errorprofile'), p('indelprofile'), p('fa'), p('fq'), p('bam'), **kw); dt = time.time() - t
        print('ps_map_to_bam %s, %s: %.2fs, %d of %d records kept, BAM %.0f MB'
              % (kw, LABEL[switch][device >= 0], dt, st['n_out'], st['n_in'], st['bam_bytes'] / 1e6), flush=True)
capi.ps_bgzf_device(-1)
capi.ps_bam_records_device(0)
capi.ps_bam_sort_device(-1)
