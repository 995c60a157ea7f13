"""step time of the collapsed search (ps_ctx_set_collapse) against the plain one at duplication factors 1, 2, 4, 8: the same number
of reads made of 1/f as many different ones, shuffled; factor 1 shows what the grouping stages cost, the others what they save.
    python tools/collapse_time.py [genome Mbp = 1000] [reads = 4000000]"""
import sys, os, time, numpy as np
sys.path.insert(0, 'para-suite_amd'); sys.path.insert(0, '.')
import capi, torch, bench
mbp = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4_000_000
dev = torch.device('cuda', 0)
contigs = bench.gen_genome(torch, dev, mbp * 1_000_000, 24, 0x5EED0002)
fa = '/tmp/g_collapse.fa'; bench.write_fasta(fa, contigs); torch.cuda.empty_cache()
ctx = capi.Ctx.build(fa)
P = np.array(bench.PROFILE); P[3,1], P[3,3] = 0.12, 0.87
ctx.set_profile(P, bench.INS_RATE, bench.DEL_RATE, -1)
rd = np.asarray(bench.gen_reads(torch, dev, contigs, n, 50, 0x5EED0006, indels=True))
rng = np.random.default_rng(6)
for f in (1, 2, 4, 8):
    codes = np.ascontiguousarray(np.tile(rd[:n // f], (f, 1))[rng.permutation(n // f * f)])
    for collapse in (0, 1):
        ctx.set_collapse(collapse)
        b = ctx.batch_from_codes(codes)
        best = None
        for rep in range(3):
            t = time.time(); b.run(16); dt = time.time() - t
            tm, ci = b.timing(), b.collapse_info()
            if best is None or dt < best[0]:
                best = (dt, tm, ci)
        dt, tm, ci = best
        print("factor %d collapse %s: %d reads, best of 3 runs %.3f s = %.2f M reads/s; backtrack %.0f ms in %d launches, width %.0f ms; searched %d of %d, %d groups, largest %d, collapse stages %.2f ms"
              % (f, "on " if collapse else "off", codes.shape[0], dt, codes.shape[0] / dt / 1e6, tm["ms_backtrack"], tm["n_backtrack_launches"], tm["ms_width"],
                 ci["n_searched"], ci["n_reads"], ci["n_groups"], ci["largest"], ci["ms_collapse"]), flush=True)
        b.free()
