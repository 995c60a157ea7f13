"""BGZF compression in isolation: the device path (staging, H2D, kernels, D2H, assembly: one ps_bgzf_compress call on device 0)
against the library's own host path (the same call with device -1: zlib level 1 under the library's threads, 16 of them) on the
same bytes and the same block cuts, which is what the library writes without the switch.  Three corpora from one mapping of
simulated 50 bp reads: the mapper's records in input order, the same coordinate-sorted, and the header blocks.  The two record
corpora are timed REPEAT times over in one call (default 8: more than a gigabyte, so that a timed window is a quarter of a
second and more).  Per corpus: size against zlib level 1, median and range of RUNS timed runs after a warm-up, per GB of
uncompressed BAM; kernel_ms is the kernels alone.

    python tools/bgzf_time.py [N_READS=1000000] [GENOME_MBP=100] [RUNS=5] [WORKDIR=/tmp] [REPEAT=8]"""
import ctypes as C, gzip, os, statistics, sys, time
import numpy as np
sys.path.insert(0, 'para-suite_amd'); sys.path.insert(0, '.')
import torch, capi, bench

BLK = 0xff00
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
mbp = int(sys.argv[2]) if len(sys.argv) > 2 else 100
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
work = sys.argv[4] if len(sys.argv) > 4 else '/tmp'
repeat = int(sys.argv[5]) if len(sys.argv) > 5 else 8
p = lambda x: os.path.join(work, 'bgzf_time.' + x)


def corpora():
    dev = torch.device('cuda', 0)
    contigs = bench.gen_genome(torch, dev, mbp * 1_000_000, 8, 0x5EED0002)
    bench.write_fasta(p('fa'), contigs)
    rd = bench.gen_reads(torch, dev, contigs, n, 50, 0x5EED0003, indels=True)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    name = np.char.zfill(np.arange(n).astype(str), 9).astype('S9').view(np.uint8).reshape(n, 9)
    rec = np.empty((n, 1 + 9 + 1 + 50 + 3 + 50 + 1), dtype=np.uint8)
    rec[:, 0] = ord('@'); rec[:, 1:10] = name; rec[:, 10] = 10; rec[:, 11:61] = lut[rd]; rec[:, 61] = 10; rec[:, 62] = ord('+'); rec[:, 63] = 10
    rec[:, 64:114] = (33 + 2 + (np.arange(n * 50, dtype=np.uint64) * 2654435761 >> 13) % 39).astype(np.uint8).reshape(n, 50); rec[:, 114] = 10   # Phred 2..40, not one value
    open(p('fq'), 'wb').write(rec.tobytes())
    capi.ps_index(p('fa'))
    out = {}
    for key, kw in (('unsorted', {}), ('sorted', dict(sort_by_coordinate=True))):
        capi.ps_map_to_bam(16, '2', None, None, p('fa'), p('fq'), p(key + '.bam'), **kw)
        raw = open(p(key + '.bam'), 'rb').read()
        n_head, at = 0, 0
        stream = gzip.decompress(raw)
        l_text = int.from_bytes(stream[4:8], 'little'); at = 8 + l_text
        n_ref = int.from_bytes(stream[at:at + 4], 'little'); at += 4
        for _ in range(n_ref):
            at += 8 + int.from_bytes(stream[at:at + 4], 'little')
        out[key] = stream[at:]
        out['header'] = stream[:at]
    return out


def main():
    lib = capi.lib()
    os.environ['PS_BAM_LEVEL'] = '1'
    for key, one in corpora().items():
        data = one if key == 'header' else one * repeat
        cap = len(data) + len(data) // 100 + (len(data) // BLK + 1) * 128
        dst, ref = C.create_string_buffer(cap), C.create_string_buffer(cap)
        st, sh = (capi.BgzfStats(struct_size=C.sizeof(capi.BgzfStats)) for _ in range(2))
        t_dev, t_host, k_ms = [], [], []
        for r in range(runs + 1):                      # the first run of each is the warm-up
            t = time.perf_counter(); rc = lib.ps_bgzf_compress(data, len(data), 0, dst, cap, C.byref(st)); dt = time.perf_counter() - t
            assert rc == 0, lib.ps_last_error()
            t = time.perf_counter(); rc = lib.ps_bgzf_compress(data, len(data), -1, ref, cap, C.byref(sh)); dh = time.perf_counter() - t
            assert rc == 0, lib.ps_last_error()
            if r:
                t_dev.append(dt); t_host.append(dh); k_ms.append(st.kernel_ms / 1e3)
        assert gzip.decompress(dst.raw[:st.out_bytes]) == data and gzip.decompress(ref.raw[:sh.out_bytes]) == data
        gb = len(data) / 1e9
        f = lambda v: '%.4f s (%.4f to %.4f), %.3f s/GB' % (statistics.median(v), min(v), max(v), statistics.median(v) / gb)
        print('%-8s %11d bytes in %6d blocks (stored %d fixed %d dynamic %d): device %d bytes, host zlib level 1 %d bytes, device/zlib1 %.4f'
              % (key, len(data), st.n_blocks, st.n_stored, st.n_fixed, st.n_dynamic, st.out_bytes, sh.out_bytes, st.out_bytes / sh.out_bytes))
        print('%-8s median (range) of %d: device path %s; its kernels %s; library host path, zlib level 1 on 16 threads %s'
              % (key, runs, f(t_dev), f(k_ms), f(t_host)), flush=True)


main()
