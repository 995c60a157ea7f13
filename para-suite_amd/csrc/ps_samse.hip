// ps_samse.hip -- the samse stage of a searched batch: tie-break selection (one drand48 stream over all reads in input
// order), SA walk, strand / MAPQ and the banded DP of gapped hits.  The reads whose choice depends on the data (several best
// intervals, alternative hits, a larger search tier: Batch::sub, made by batch_search) are finished on the host by the same rules.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "ps_pipeline.h"
#include "ps_dev.h"
#include "ps_par.h"

namespace ps {

__device__ __forceinline__ unsigned long long lcg_jump(unsigned long long x, unsigned long long t)
{
    const unsigned long long M = 0xFFFFFFFFFFFFULL;
    unsigned long long a = 0x5DEECE66DULL, c = 0xBULL, ra = 1, rc = 0;
    while (t) {
        if (t & 1) { ra = (ra * a) & M; rc = (rc * a + c) & M; }
        c = (c * a + c) & M; a = (a * a) & M;
        t >>= 1;
    }
    return (ra * x + rc) & M;
}

struct SelectArgs {
    const AlnRec *alns; int aln_cap; const int32_t *n_aln; const int32_t *ids; int n;
    const uint8_t *cls; const uint32_t *e_before; const uint32_t *h_before; const unsigned long long *hard_cum;
    unsigned long long draws_in;
    SelRec *sel; bwtint *rows; int *err;
};
// ---- the choice of a read's main hit (upstream bwa_aln2seq_core), ONE copy for the device kernel and the host-finished reads ----
// Walks the best-score intervals in list order: every one costs a draw, the one that wins costs a second draw that places the hit
// inside it.  x is the state of the drand48 stream (advanced by the draws made, whose number is returned); c1 / c2 = occurrences
// at the best score / at the other listed scores.  IEEE doubles in this order of operations on both sides.
struct MainPick { bwtint sa; int32_t c1, c2; int type, n_mm, n_gapo, n_gape, ref_shift, score; };
__host__ __device__ inline unsigned long long lcg48_next(unsigned long long x) { return (x * 0x5DEECE66DULL + 0xBULL) & 0xFFFFFFFFFFFFULL; }
__host__ __device__ inline int rule_choose_main(const AlnRec *al, int na, unsigned long long &x, MainPick &h)
{
    int cnt = 0, draws = 0, i;
    const int best = al[0].score;
    h.sa = 0; h.n_mm = h.n_gapo = h.n_gape = h.ref_shift = h.score = 0;
    for (i = 0; i < na; ++i) {
        const AlnRec p = al[i];
        if (p.score > best) break;
        const unsigned long long wdt = (unsigned long long)(p.l - p.k) + 1ull;
        x = lcg48_next(x); ++draws;
        if ((double)x * (1.0 / 281474976710656.0) * (double)(wdt + (unsigned long long)(long long)cnt) > (double)cnt) {
            h.n_mm = p.n_mm; h.n_gapo = p.n_gapo; h.n_gape = p.n_gape;
            h.ref_shift = (int)p.n_del - (int)p.n_ins; h.score = p.score;
            x = lcg48_next(x); ++draws;
            h.sa = p.k + (bwtint)((double)wdt * ((double)x * (1.0 / 281474976710656.0)));
        }
        cnt += (int)wdt;
    }
    h.c1 = cnt;
    for (; i < na; ++i) cnt += (int)((unsigned long long)(al[i].l - al[i].k) + 1ull);
    h.c2 = cnt - h.c1;
    h.type = h.c1 > 1 ? 2 : 1;
    return draws;
}

// the single-best reads: two draws at a stream position known from the prefix counts
__global__ void k_select(SelectArgs a)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += gridDim.x * blockDim.x) {
        const int g = a.ids[r];
        const uint8_t c = a.cls[g];
        SelRec s; s.sa = 0; s.c1 = s.c2 = 0; s.type = 0; s.n_mm = s.n_gapo = s.n_gape = 0; s.ref_shift = 0; s.score = 0; s.pad[0] = s.pad[1] = 0;
        if (c == 1) {                       // class 1, finished on the device
            const AlnRec *al = a.alns + (size_t)r * a.aln_cap;
            const int na = a.n_aln[r];
            const unsigned int hb = a.h_before[g];
            const unsigned long long off = a.draws_in + 2ull * a.e_before[g] + (hb ? a.hard_cum[hb - 1] : 0ull);
            unsigned long long x = lcg_jump((11ull << 16) | 0x330Eull, off);
            if (lcg48_next(x) == 0) *a.err = 1;       // the offsets assume two draws per such read: the first draw wins unless it is exactly 0
            MainPick pk;
            (void)rule_choose_main(al, na, x, pk);
            s.sa = pk.sa; s.c1 = pk.c1; s.c2 = pk.c2; s.type = (uint8_t)pk.type;
            s.n_mm = (uint8_t)pk.n_mm; s.n_gapo = (uint8_t)pk.n_gapo; s.n_gape = (uint8_t)pk.n_gape; s.ref_shift = (int8_t)pk.ref_shift; s.score = (uint8_t)pk.score;
        }
        a.sel[g] = s;
        a.rows[g] = s.type ? s.sa : 0;
    }
}

struct PostArgs {
    const int32_t *ids; int n, len; const int32_t *lens; long long l_pac;
    const uint8_t *cls; const SelRec *sel; const bwtint *pos; FinRec *fin;
    int budget, profile, unit; const uint8_t *logn;     // MAPQ rule inputs; logn[n] = (int)(4.343 ln n + .5)
    const uint8_t *budget_by_len;                        // with lens: the difference budget of a read of every length (budget: the longest read's)
    RefineItem *items; int32_t *item_g; unsigned int *n_items;
};
// ---- the two samse rules every finished hit goes through, ONE copy for the device kernel and for the host-finished subset ----
// text position of an SA row -> forward coordinate of the alignment's first base and its strand (upstream bwa_sa2pos /
// bwa_cal_pac_pos_core); -1: the alignment spans the forward/reverse junction
__host__ __device__ inline long long rule_to_forward(long long pos_t, long long l_pac, int ref_len, int &strand)
{
    long long pos_f = pos_t;
    strand = 0;
    if (pos_f < l_pac && l_pac < pos_f + ref_len) return -1;
    const bool is_rev = pos_f >= l_pac;
    if (is_rev) pos_f = 2 * l_pac - 1 - pos_f;
    strand = !is_rev;
    if (is_rev) pos_f = pos_f + 1 < ref_len ? 0 : pos_f - ref_len + 1;
    return pos_f;
}
// upstream bwa_approx_mapQ with the budget rule of the cost model in use; logn[n] = (int)(4.343 ln n + .5), n < 256
__host__ __device__ inline int rule_mapq(int c1, int c2, int n_mm, int score, int budget, bool profile, int unit, const uint8_t *logn)
{
    if (c1 == 0) return 23;
    if (c1 > 1) return 0;
    if (!profile) { if (n_mm == budget) return 25; }
    else if (budget * unit - score < unit) return 25;
    if (c2 == 0) return 37;
    const int lg = logn[c2 >= 255 ? 255 : c2];
    return 23 < lg ? 0 : 23 - lg;
}
static void mapq_logn_table(uint8_t logn[256])
{
    logn[0] = 0;
    for (int n = 1; n < 256; ++n) logn[n] = (uint8_t)(int)(4.343 * std::log((double)n) + 0.5);
}

// text position -> forward coordinate + strand, MAPQ; gapped hits are queued for the banded-DP kernel
__global__ void k_post(PostArgs a)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.n; r += gridDim.x * blockDim.x) {
        const int g = a.ids[r];
        FinRec f; f.pos = -1; f.strand = 0; f.mapq = 0; f.type = 0; f.pad[0] = f.pad[1] = f.pad[2] = f.pad[3] = f.pad[4] = 0;
        const SelRec s = a.sel[g];
        if (a.cls[g] == 1 && s.type != 0) {
            const int ref_len = (a.lens ? a.lens[r] : a.len) + s.ref_shift;
            int strand = 0;
            const long long p = rule_to_forward((long long)a.pos[g], a.l_pac, ref_len, strand);
            const int budget = (a.lens && a.budget_by_len) ? (int)a.budget_by_len[a.lens[r]] : a.budget;
            const int mq = rule_mapq(s.c1, s.c2, s.n_mm, (int)s.score, budget, a.profile != 0, a.unit, a.logn);
            f.pos = p; f.strand = (uint8_t)strand; f.mapq = (uint8_t)mq; f.type = p < 0 ? 0 : s.type;
            if (f.type != 0 && s.n_gapo) {
                const unsigned int q = atomicAdd(a.n_items, 1u);
                a.items[q] = RefineItem{r, (bwtint)p, (int32_t)s.ref_shift, strand};
                a.item_g[q] = g;
            }
        }
        a.fin[g] = f;
    }
}

// ----------------------------------------------------- tie-break selection -----
// Among the hits with the best score one occurrence is chosen at random; the reference's aligner
// draws from ONE drand48 stream (seed 11) over all reads in input order.
static int choose_main(const AlnRec *al, int na, Rng48 &rng, Hit &h)
{
    MainPick pk;
    unsigned long long x = rng.x;
    const int draws = rule_choose_main(al, na, x, pk);
    rng.x = x;
    h.sa = pk.sa; h.c1 = pk.c1; h.c2 = pk.c2; h.type = pk.type;
    h.n_mm = pk.n_mm; h.n_gapo = pk.n_gapo; h.n_gape = pk.n_gape; h.ref_shift = pk.ref_shift; h.score = pk.score;
    return draws;
}

// the sequential part of the stream: reads with several best-score intervals, in input order
void batch_select_hard(Batch &b, uint64_t draws_before, uint64_t *draws_after)
{
    if (!b.searched) throw Error("select before search");
    auto t0 = HostClock::now();
    b.draws_in = draws_before;
    b.hard_draws_cum.assign((size_t)b.n_hard, 0);
    Rng48 rng(11);
    rng.jump(draws_before);
    uint64_t H = 0; int64_t e_prev = 0;
    for (SubRead &sr : b.sub) {
        if (sr.cls != 2) continue;
        rng.jump(2ull * (uint64_t)(sr.easy_before - e_prev));      // the single-best reads in between took two draws each
        e_prev = sr.easy_before;
        sr.hit = Hit();
        H += (uint64_t)choose_main(sr.alns, sr.n_alns, rng, sr.hit);
        b.hard_draws_cum[(size_t)sr.hard_before] = H;
    }
    b.draws_out = draws_before + 2ull * (uint64_t)b.n_class1 + H;
    if (draws_after) *draws_after = b.draws_out;
    b.selected_hard = true;
    b.tm.ms_select += ms_since(t0); b.tm.ms_sel_hard = ms_since(t0);
}

void batch_select_easy(Batch &b, int threads)
{
    if (!b.selected_hard) throw Error("select_easy before select_hard");
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    require_device(ctx->device);
    auto t0 = HostClock::now();
    const int64_t N = b.rs.n;
    (void)threads;
    // ---- device: prefix counts of the two draw classes, then every single-best read picks its occurrence ----
    if (b.d_sel.n < (size_t)N) { b.d_sel.alloc((size_t)N); b.d_fin.alloc((size_t)N); b.d_rows.alloc((size_t)N + 1); b.d_pos.alloc((size_t)N + 1); b.d_eb.alloc((size_t)N); b.d_hb.alloc((size_t)N); }
    const double ms_alloc = ms_since(t0);
    {
        // the counts in front of every group of 64 reads come from the host (batch_search, which has the classes in input order);
        // the kernel adds the rank inside the group.  (Two library scans over 10 M flag words did this: their kernels keep 17 KB of
        // LDS and waited for the other batch's resident search launch to drain, ps_budget.h.)
        const size_t n_grp = ((size_t)N + 63) / 64;
        uint32_t *d_grp = wk->ws_get<uint32_t>("class_grp", 2 * n_grp + 2);
        PS_HIP(hipMemcpyAsync(d_grp, b.h_grp, 2 * n_grp * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        launch_class_ranks(b.d_class.p, (long long)N, d_grp, b.d_eb.p, b.d_hb.p, s);
    }
    unsigned long long *d_cum = wk->ws_get<unsigned long long>("hard_cum", (size_t)b.n_hard + 1);
    if (b.n_hard) PS_HIP(hipMemcpyAsync(d_cum, b.hard_draws_cum.data(), (size_t)b.n_hard * 8, hipMemcpyHostToDevice, s));
    int *d_err = wk->ws_get<int>("sel_err", 4);
    PS_HIP(hipMemsetAsync(d_err, 0, 16, s));
    for (Bin &bin : b.bins) {
        SelectArgs a;
        a.alns = bin.d_alns.p; a.aln_cap = bin.aln_cap; a.n_aln = bin.d_n_aln.p; a.ids = bin.d_ids.p; a.n = (int)bin.ids.size();
        a.cls = b.d_class.p; a.e_before = b.d_eb.p; a.h_before = b.d_hb.p; a.hard_cum = d_cum; a.draws_in = b.draws_in;
        a.sel = b.d_sel.p; a.rows = b.d_rows.p; a.err = d_err;
        hipLaunchKernelGGL(k_select, dim3(std::min((a.n + 255) / 256, 4096)), dim3(256), 0, s, a);
    }
    const double ms_launch = ms_since(t0);
    // ---- host: the subset (its class-1 members by the same offset algebra, then the alternative-hit lists) ----
    const int n_occ = ctx->opt.n_occ;
    b.multis.clear();
    {
        const int nt = par_threads(b.sub.size(), threads);
        std::vector<std::vector<Multi>> part(nt);
        std::vector<size_t> first(nt + 1, 0);
        par_for(b.sub.size(), threads, [&](size_t q0, size_t q1, int t) {
            std::vector<Multi> &mine = part[t];
            first[t] = q0;
            for (size_t q = q0; q < q1; ++q) {
                SubRead &sr = b.sub[q];
                const int na = sr.n_alns;
                Hit &h = sr.hit;
                if (sr.cls == 0 || na == 0) { h = Hit(); h.type = 0; h.pos = -1; continue; }
                if (sr.cls == 1) {
                    h = Hit();
                    Rng48 rng(11);
                    rng.jump(b.draws_in + 2ull * (uint64_t)sr.easy_before + (sr.hard_before ? b.hard_draws_cum[(size_t)sr.hard_before - 1] : 0ull));
                    Rng48 probe = rng;
                    if (probe.step() == 0) throw Error("tie-break stream hit the zero state; sequential replay required");
                    choose_main(sr.alns, na, rng, h);
                }
                h.pos = -1; h.multi_begin = (int32_t)mine.size(); h.n_multi = 0;     // local index: shifted below
                if (n_occ > 0) {                     // alternative hits (samse -n): only if all occurrences of all hits number <= n_occ+1
                    int tot = 0;
                    for (int k = 0; k < na; ++k) tot += (int)((uint64_t)(sr.alns[k].l - sr.alns[k].k) + 1ull);
                    if (tot >= 0 && (long long)tot <= (long long)n_occ + 1)
                        for (int k = 0; k < na; ++k)
                            for (uint64_t row = sr.alns[k].k; row <= sr.alns[k].l; ++row) {
                                Multi m; std::memset(&m, 0, sizeof m);
                                m.row = (bwtint)row; m.gap = sr.alns[k].n_gapo + sr.alns[k].n_gape; m.mm = sr.alns[k].n_mm;
                                m.ref_shift = (int)sr.alns[k].n_del - (int)sr.alns[k].n_ins; m.pos = -1;
                                mine.push_back(m); ++h.n_multi;
                            }
                }
            }
        });
        std::vector<size_t> base(nt + 1, 0);
        for (int t = 0; t < nt; ++t) base[t + 1] = base[t] + part[t].size();
        b.multis.resize(base[nt]);
        const size_t per = b.sub.empty() ? 1 : (b.sub.size() + (size_t)nt - 1) / (size_t)nt;
        par_for((size_t)nt, nt, [&](size_t t0, size_t t1, int) {
            for (size_t t = t0; t < t1; ++t) {
                if (!part[t].empty()) std::memcpy(b.multis.data() + base[t], part[t].data(), part[t].size() * sizeof(Multi));
                const size_t q0 = t * per, q1 = std::min(b.sub.size(), q0 + per);
                for (size_t q = q0; q < q1; ++q) if (b.sub[q].cls != 0 && b.sub[q].n_alns != 0) b.sub[q].hit.multi_begin += (int32_t)base[t];
            }
        });
    }
    const double ms_host = ms_since(t0);
    int err = 0;
    PS_HIP(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    if (err) throw Error("tie-break stream hit the zero state; sequential replay required");
    if (const char *e = std::getenv("PS_VERBOSE")) if (std::atoi(e) >= 3)
        std::fprintf(stderr, "[parasuite-hip]     select_easy of %lld reads: allocations %.1f ms, launches until %.1f, host part until %.1f, device done at %.1f ms\n", (long long)N, ms_alloc, ms_launch, ms_host, ms_since(t0));
    b.selected = true;
    b.tm.ms_select += ms_since(t0); b.tm.ms_sel_easy = ms_since(t0);
}

// ------------------------------------------------- locate / MAPQ / gapped DP ----
static int fix_cigar(uint32_t *cigar, int n, int64_t &rb)
{
    if (n <= 0) return 0;
    if ((cigar[n - 1] & 0xf) == 1) cigar[n - 1] = (cigar[n - 1] >> 4 << 4) | 3;   // trailing insertion -> soft clip
    if ((cigar[0] & 0xf) == 1) cigar[0] = (cigar[0] >> 4 << 4) | 3;
    if ((cigar[n - 1] & 0xf) == 2) --n;                                            // trailing deletion dropped
    if (n > 0 && (cigar[0] & 0xf) == 2) { rb += cigar[0] >> 4; --n; std::memmove(cigar, cigar + 1, (size_t)n * 4); }
    return n;
}

// The cleaned-up CIGAR of a gapped hit as the batch keeps it.  The banded alignment hands back at most PS_MAX_CIGAR operations and drops
// what does not fit: the rest then no longer spans the whole read (read_len bases) or the whole reference window (ref_len bases).
// (Up to 2 * max_gapo + 1 operations come from the search; the alignment may trade two mismatches for one more gap.)
static int take_cigar(uint32_t *cigar, int n, int64_t &rb, int read_len, int ref_len)
{
    static_assert(PS_HIT_CIGAR == PS_MAX_CIGAR, "a Hit holds what the banded alignment hands back");
    int on_read = 0, on_ref = 0;
    for (int j = 0; j < n; ++j) { const int l = (int)(cigar[j] >> 4), op = (int)(cigar[j] & 0xf); if (op != 2) on_read += l; if (op != 1) on_ref += l; }
    if (n > 0 && (on_read != read_len || on_ref != ref_len)) throw Error("CIGAR with more than " + std::to_string(PS_HIT_CIGAR) + " operations (PS_HIT_CIGAR); lower -o");
    return fix_cigar(cigar, n, rb);
}

// banded DP kernel over a list of items of one length bin; cigars come back to the host
static void run_refine(Batch &b, Bin &bin, const RefineItem *d_items, int n_it, std::vector<uint32_t> &cig, std::vector<int32_t> &nc)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    uint32_t *d_cig = wk->ws_get<uint32_t>("rf_cig", (size_t)n_it * PS_MAX_CIGAR); int32_t *d_nc = wk->ws_get<int32_t>("rf_nc", n_it);
    int blocks = (n_it + 63) / 64; if (blocks > 2048) blocks = 2048;
    const int tmax = bin.len + 64;
    RefineArgs ra;
    ra.ix = ctx->ix.view; ra.n_items = n_it; ra.len = bin.len; ra.lens = bin.ragged ? bin.d_lens.p : nullptr; ra.n_reads = (int)bin.ids.size();
    ra.bases = bin.bases.p; ra.nmask = bin.nmask.p; ra.items = d_items; ra.cigar = d_cig; ra.n_cigar = d_nc;
    ra.z_per_block = (size_t)64 * tmax * (bin.len < 2 * tmax + 1 ? bin.len : 2 * tmax + 1);
    ra.zbuf = wk->ws_get<uint8_t>("rf_z", ra.z_per_block * blocks);
    ra.he_per_block = refine_he_words(bin.len);
    ra.hebuf = wk->ws_get<int32_t>("rf_he", ra.he_per_block * blocks);
    EventPair t(s); launch_refine(ra, blocks, s); PS_HIP(hipGetLastError()); t.stop(s);
    cig.resize((size_t)n_it * PS_MAX_CIGAR); nc.resize(n_it);
    PS_HIP(hipMemcpyAsync(cig.data(), d_cig, cig.size() * 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(nc.data(), d_nc, (size_t)n_it * 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    b.tm.ms_refine += t.ms();
}

void batch_locate(Batch &b)
{
    if (!b.selected) throw Error("locate before select");
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    require_device(ctx->device);
    const int64_t N = b.rs.n, l_pac = ctx->ix.ref.l_pac;
    auto t0 = HostClock::now();
    // ---- device-finished reads: SA walk, strand / MAPQ, queue of gapped hits ----
    // (the SA walk, k_post and the downloads go to the stream back to back; the walk's time is read after the one wait behind them)
    EventPair t_sa(s); launch_sa2pos(ctx->ix.view, b.d_rows.p, b.d_pos.p, (int)N, b.d_stats.p + 2, s); PS_HIP(hipGetLastError()); t_sa.stop(s);
    uint8_t logn[256];
    mapq_logn_table(logn);
    uint8_t *d_logn = wk->ws_get<uint8_t>("logn", 256);
    PS_HIP(hipMemcpyAsync(d_logn, logn, 256, hipMemcpyHostToDevice, s));
    uint8_t *h_budget = wk->pin_get<uint8_t>("budget_by_len_h", 256);
    for (int l2 = 0; l2 < 256; ++l2) { const int bd = budget_diffs(ctx->opt, l2); h_budget[l2] = (uint8_t)(bd > 255 ? 255 : bd); }
    uint8_t *d_budget = wk->ws_get<uint8_t>("budget_by_len", 256);
    PS_HIP(hipMemcpyAsync(d_budget, h_budget, 256, hipMemcpyHostToDevice, s));
    b.dev_cigars.clear();
    struct BinItems { RefineItem *d_items; int32_t *d_item_g; unsigned int *d_n; unsigned int n; };
    std::vector<BinItems> bi_items(b.bins.size());
    for (size_t bi = 0; bi < b.bins.size(); ++bi) {
        Bin &bin = b.bins[bi];
        const int n = (int)bin.ids.size();
        BinItems &it = bi_items[bi];
        it.d_items = wk->ws_get<RefineItem>("post_items" + std::to_string(bi), n); it.d_item_g = wk->ws_get<int32_t>("post_item_g" + std::to_string(bi), n);
        it.d_n = wk->ws_get<unsigned int>("post_n" + std::to_string(bi), 4);
        PS_HIP(hipMemsetAsync(it.d_n, 0, 16, s));
        PostArgs a;
        a.ids = bin.d_ids.p; a.n = n; a.len = bin.len; a.lens = bin.ragged ? bin.d_lens.p : nullptr; a.l_pac = l_pac; a.cls = b.d_class.p; a.sel = b.d_sel.p; a.pos = b.d_pos.p; a.fin = b.d_fin.p;
        a.budget = budget_diffs(ctx->opt, bin.len); a.profile = ctx->opt.profile; a.unit = ctx->opt.unit; a.logn = d_logn; a.budget_by_len = d_budget;
        a.items = it.d_items; a.item_g = it.d_item_g; a.n_items = it.d_n;
        hipLaunchKernelGGL(k_post, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, s, a);
        PS_HIP(hipMemcpyAsync(&it.n, it.d_n, 4, hipMemcpyDeviceToHost, s));
    }
    b.h_sel = (SelRec *)b.p_sel.get((size_t)N * sizeof(SelRec) + 64);
    b.h_fin = (FinRec *)b.p_fin.get((size_t)N * sizeof(FinRec) + 64);
    PS_HIP(hipMemcpyAsync(b.h_sel, b.d_sel.p, (size_t)N * sizeof(SelRec), hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(b.h_fin, b.d_fin.p, (size_t)N * sizeof(FinRec), hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    b.tm.ms_sa2pos += t_sa.ms();
    PS_HIP(hipMemcpy(&b.st_sa2pos, b.d_stats.p + 2, sizeof(KStats), hipMemcpyDeviceToHost));
    const bool patch_test = std::getenv("PS_LOCATE_PATCH_TEST") != nullptr && std::atoi(std::getenv("PS_LOCATE_PATCH_TEST")) > 0;
    for (size_t bi = 0; bi < b.bins.size(); ++bi) {            // gapped device-finished hits: banded DP, CIGAR clean-up
        BinItems &it = bi_items[bi];
        if (!it.n) continue;
        std::vector<uint32_t> cig; std::vector<int32_t> nc; std::vector<int32_t> gs(it.n);
        run_refine(b, b.bins[bi], it.d_items, (int)it.n, cig, nc);
        PS_HIP(hipMemcpy(gs.data(), it.d_item_g, (size_t)it.n * 4, hipMemcpyDeviceToHost));
        for (unsigned int q = 0; q < it.n; ++q) {
            const int64_t g = gs[q];
            uint32_t *c = cig.data() + (size_t)q * PS_MAX_CIGAR;
            int64_t rb = b.h_fin[g].pos;
            int n_c = take_cigar(c, nc[q], rb, b.rs.len[g], b.rs.len[g] + b.h_sel[g].ref_shift);
            if (patch_test && n_c > 0 && n_c < PS_HIT_CIGAR && (c[0] & 0xf) == 0 && (c[0] >> 4) >= 2) {
                // PS_LOCATE_PATCH_TEST (tests): what the clean-up does to an alignment that starts with a deletion -- the position moves, or the
                // CIGAR comes back empty -- on hits where the banded alignment did not produce one: the first base is clipped instead
                if (g % 5 == 4) n_c = 0;
                else { std::memmove(c + 1, c, (size_t)n_c * 4); c[1] -= 1u << 4; c[0] = (1u << 4) | 3u; ++n_c; rb += 1; }
            }
            DevCigar dc; dc.g = g; dc.n = n_c; std::memcpy(dc.c, c, sizeof dc.c);
            b.dev_cigars.push_back(dc);
            b.h_fin[g].pos = rb;
            if (n_c == 0) b.h_fin[g].type = 0;
        }
    }
    std::sort(b.dev_cigars.begin(), b.dev_cigars.end(), [](const DevCigar &x, const DevCigar &y) { return x.g < y.g; });
    auto t1 = HostClock::now();
    // ---- host-finished subset: its rows (main + alternatives) through the same SA kernel, then strand / MAPQ / DP ----
    const size_t M = b.sub.size(), n_rows = M + b.multis.size();
    if (n_rows) {
        std::vector<bwtint> rows(n_rows), pos(n_rows);
        par_for(M, ctx->host_threads, [&](size_t q0, size_t q1, int) { for (size_t q = q0; q < q1; ++q) rows[q] = b.sub[q].hit.type != 0 ? b.sub[q].hit.sa : 0; });
        par_for(b.multis.size(), ctx->host_threads, [&](size_t j0, size_t j1, int) { for (size_t j = j0; j < j1; ++j) rows[M + j] = b.multis[j].row; });
        bwtint *d_r = wk->ws_get<bwtint>("sub_rows", n_rows), *d_p = wk->ws_get<bwtint>("sub_pos", n_rows);
        PS_HIP(hipMemcpyAsync(d_r, rows.data(), n_rows * sizeof(bwtint), hipMemcpyHostToDevice, s));
        { EventPair t(s); launch_sa2pos(ctx->ix.view, d_r, d_p, (int)n_rows, nullptr, s); PS_HIP(hipGetLastError()); t.stop(s); b.tm.ms_sa2pos += t.ms(); }
        PS_HIP(hipMemcpyAsync(pos.data(), d_p, n_rows * sizeof(bwtint), hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        std::vector<std::vector<RefineItem>> items(b.bins.size());
        struct Back { size_t q; int32_t multi; };             // multi < 0: main hit
        std::vector<std::vector<Back>> back(b.bins.size());
        {
            const int nt = par_threads(M, ctx->host_threads);
            std::vector<std::vector<std::vector<RefineItem>>> t_items(nt, std::vector<std::vector<RefineItem>>(b.bins.size()));
            std::vector<std::vector<std::vector<Back>>> t_back(nt, std::vector<std::vector<Back>>(b.bins.size()));
            par_for(M, ctx->host_threads, [&](size_t q0, size_t q1, int t) {
                for (size_t q = q0; q < q1; ++q) {
                    SubRead &sr = b.sub[q]; Hit &h = sr.hit;
                    const int len = b.rs.len[sr.g], bi = b.read_bin[sr.g];
                    if (h.type != 0) {
                        int strand = 0;
                        h.pos = rule_to_forward((long long)pos[q], l_pac, len + h.ref_shift, strand);
                        h.strand = strand;
                        h.mapq = rule_mapq(h.c1, h.c2, h.n_mm, h.score, budget_diffs(ctx->opt, len), ctx->opt.profile, ctx->opt.unit, logn);
                        if (h.pos < 0) h.type = 0;
                    }
                    int kept = 0;
                    for (int j = 0; j < h.n_multi; ++j) {
                        Multi &m = b.multis[h.multi_begin + j];
                        int strand = 0;
                        m.pos = rule_to_forward((long long)pos[M + h.multi_begin + j], l_pac, len + m.ref_shift, strand);
                        m.strand = strand;
                        if (m.pos != h.pos && m.pos >= 0) b.multis[h.multi_begin + kept++] = m;
                    }
                    h.n_multi = kept;
                    for (int j = 0; j < h.n_multi; ++j) {
                        Multi &m = b.multis[h.multi_begin + j];
                        if (m.gap) { t_items[t][bi].push_back(RefineItem{b.read_local[sr.g], (bwtint)m.pos, m.ref_shift, m.strand}); t_back[t][bi].push_back(Back{q, j}); }
                    }
                    if (h.type != 0 && h.n_gapo) { t_items[t][bi].push_back(RefineItem{b.read_local[sr.g], (bwtint)h.pos, h.ref_shift, h.strand}); t_back[t][bi].push_back(Back{q, -1}); }
                }
            });
            for (int t = 0; t < nt; ++t)
                for (size_t bi = 0; bi < b.bins.size(); ++bi) {
                    items[bi].insert(items[bi].end(), t_items[t][bi].begin(), t_items[t][bi].end());
                    back[bi].insert(back[bi].end(), t_back[t][bi].begin(), t_back[t][bi].end());
                }
        }
        for (size_t bi = 0; bi < b.bins.size(); ++bi) {
            const int n_it = (int)items[bi].size();
            if (!n_it) continue;
            RefineItem *d_it = wk->ws_get<RefineItem>("sub_items", n_it);
            PS_HIP(hipMemcpyAsync(d_it, items[bi].data(), (size_t)n_it * sizeof(RefineItem), hipMemcpyHostToDevice, s));
            std::vector<uint32_t> cig; std::vector<int32_t> nc;
            run_refine(b, b.bins[bi], d_it, n_it, cig, nc);
            for (int q = 0; q < n_it; ++q) {
                const Back &bk = back[bi][q];
                Hit &h = b.sub[bk.q].hit;
                uint32_t *c = cig.data() + (size_t)q * PS_MAX_CIGAR;
                if (bk.multi < 0) {
                    int64_t rb = h.pos;
                    h.n_cigar = take_cigar(c, nc[q], rb, b.rs.len[b.sub[bk.q].g], b.rs.len[b.sub[bk.q].g] + h.ref_shift);
                    std::memcpy(h.cigar, c, sizeof h.cigar);
                    h.pos = rb;
                    if (h.n_cigar == 0) h.type = 0;
                } else {
                    Multi &m = b.multis[h.multi_begin + bk.multi];
                    int64_t rb = m.pos;
                    m.n_cigar = take_cigar(c, nc[q], rb, b.rs.len[b.sub[bk.q].g], b.rs.len[b.sub[bk.q].g] + m.ref_shift);
                    std::memcpy(m.cigar, c, sizeof m.cigar);
                    m.pos = rb;
                }
            }
        }
        par_for(M, ctx->host_threads, [&](size_t q0, size_t q1, int) {          // alternatives whose gapped refinement produced nothing are dropped
            for (size_t q = q0; q < q1; ++q) {
                Hit &h = b.sub[q].hit;
                int kept = 0;
                for (int j = 0; j < h.n_multi; ++j) {
                    Multi &m = b.multis[h.multi_begin + j];
                    if (m.gap && m.n_cigar == 0) continue;
                    b.multis[h.multi_begin + kept++] = m;
                }
                h.n_multi = kept;
            }
        });
    }
    b.tm.ms_host_post += ms_since(t1);
    b.located = true;
    b.tm.ms_total += ms_since(t0);
}

}  // namespace ps
