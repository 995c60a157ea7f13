// ps_search.hip -- the search stage of a batch: width kernel -> hand-out order -> backtracking kernel over every bin, the
// larger tiers for the reads that outgrew the first, then the classes of the tie-break stream and the hit lists of the reads the
// host finishes.  What a launch decides without the device (knobs, geometry, budget table) is ps_search_plan.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <optional>
#include "ps_pipeline.h"
#include "ps_search_plan.h"
#include "ps_dev.h"
#include "ps_par.h"

namespace ps {

__global__ void k_gather_alns(const AlnRec *alns, int aln_cap, const int32_t *n_aln, const uint32_t *off, int n, AlnRec *out)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        int m = n_aln[r]; if (m > aln_cap) m = aln_cap;
        for (int j = 0; j < m; ++j) out[off[r] + j] = alns[(size_t)r * aln_cap + j];
    }
}
__global__ void k_clip_counts(const int32_t *n_aln, int aln_cap, int n, uint32_t *out)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) { int m = n_aln[r]; out[r] = (uint32_t)(m > aln_cap ? aln_cap : (m < 0 ? 0 : m)); }
}

// hand-out order of a search launch: queue position -> read, heaviest estimated search first, the given (leading-base) order inside a class
__global__ void k_order_keys(const uint8_t *est, int n, int cap, uint8_t *key)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const int e = est[r] > cap ? cap : est[r];
        key[r] = (uint8_t)(cap - e);
    }
}

// A search launch in four steps; the first three fill the kernel's arguments `a`.  Step 1, the width kernel: a.w, a.cwb, a.cswb (t: its time)
static void search_width(Batch &b, BtArgs &a, EventPair &t)
{
    Work *wk = b.wk; const size_t n = (size_t)a.n_reads;
    uint32_t *cwb = wk->ws_get<uint32_t>("cwb", (size_t)lm_ncw(a.len) * n), *cswb = wk->ws_get<uint32_t>("cswb", (size_t)(lm_ncsw(a.md.seed_len) + 1) * n);
    a.w = wk->ws_get<uint32_t>("w", (size_t)(a.len + 1) * n); a.cwb = cwb; a.cswb = cswb;
    WidthArgs wa;
    wa.ix = a.ix; wa.n_reads = a.n_reads; wa.len = a.len; wa.lens = a.lens; wa.seed_len = a.md.seed_len; wa.use_seed = a.md.use_seed;
    wa.bases = a.bases; wa.nmask = a.nmask; wa.w = a.w; wa.cwb = cwb; wa.cswb = cswb; wa.stats = b.d_stats.p + 0;
    t.start(wk->stream); launch_width(wa, wk->stream); PS_HIP(hipGetLastError()); t.stop(wk->stream); ++b.tm.n_width_launches;
}

// Step 2, the hand-out order: the reads with the heaviest predicted search first (ps_effort.hip), so that the launch does not end on
// them.  PS_ORDER=0 switches it off, 2 orders by the estimated best score alone (A/B runs).  Narrow launches only: the wide
// stack takes its reads in queue order and never reads the estimate (its budget can also pass the 63 units k_effort_model
// has lanes for: -X 10 and up).  Sets a.order, a.est, a.est_ab, which stay null where there is no order (queue position == read);
// t: started here if there is one to make.  ob: the key the sort took and the model's number (profiling mode only: Ctx::launch_order)
struct OrderBufs { const uint8_t *key = nullptr; const float *pred = nullptr; };
static void search_order(Batch &b, BtArgs &a, const SearchKnobs &kn, std::optional<EventPair> &t, OrderBufs &ob)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    const Model &md = a.md; const int n = a.n_reads;
    if (a.wide || kn.order <= 0 || n < kn.order_min || md.max_units < md.c_min) return;      // a search that can afford no difference is ~len steps for every read: nothing to order
    t.emplace(s);
    uint8_t *est = wk->ws_get<uint8_t>("est", (size_t)n), *key = wk->ws_get<uint8_t>("okey", (size_t)n);
    int32_t *order = wk->ws_get<int32_t>("order", (size_t)n);
    EffortArgs ea;
    ea.ix = a.ix; ea.n_reads = n; ea.len = a.len; ea.lens = a.lens; ea.bases = a.bases; ea.nmask = a.nmask; ea.est = est;
    // everything here is in BUDGET UNITS (what the search's limits are in): the profile model has units == score, stock counts
    // every difference as one unit whatever it scores
    int csum = 0;
    for (int c = 0; c < 5; ++c) ea.s_pk[c] = md.u_mm_pk[c];
    for (int sc = 0; sc < 4; ++sc) for (int tc = 0; tc < 4; ++tc) if (sc != tc) csum += md.u_mm[sc][tc];
    ea.c_restart = kn.order_restart > 0 ? kn.order_restart : std::max(1, (csum + 6) / 12);       // an average mismatch
    ea.w_pin = (uint32_t)kn.order_wpin;
    int lv = 0; while (lv < 31 && (a.ix.seq_len >> (2 * lv)) > 0) ++lv;                      // 4^lv > rows: 17 at hg19 size
    ea.est_ab = ctx->want_read_iters ? wk->ws_get<uint16_t>("est_ab", (size_t)n) : nullptr;
    launch_effort(ea, s);
    if (kn.order == 2) hipLaunchKernelGGL(k_order_keys, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, s, est, n, kn.order_cap, key);
    else {
        EffortModelArgs em;
        em.n_reads = n; em.len = a.len; em.lens = a.lens; em.units_by_len = a.units_by_len; em.bases = a.bases; em.nmask = a.nmask; em.cwb = a.cwb; em.est = est;
        for (int c = 0; c < 5; ++c) em.s_pk[c] = md.u_mm_pk[c];
        em.inv_c_min = (uint32_t)md.inv_c_min; em.max_units = md.max_units; em.u_tight = md.u_tight;
        em.seed_units = md.max_seed_diff * md.u_tight; em.use_seed = md.use_seed; em.seed_len = md.seed_len;
        em.max_gapo = md.max_gapo; em.indel_end_skip = md.indel_end_skip; em.u_gapo_ins = md.u_gapo_ins; em.u_gapo_del = md.u_gapo_del;
        em.depth = lv + 3; em.rows = (float)a.ix.seq_len; em.log_scale = kn.order_scale;
        em.key = key; em.pred = ctx->want_read_iters ? wk->ws_get<float>("pred", (size_t)n) : nullptr;      // profiling only: the timed launch writes no number
        launch_effort_model(em, s);
        ob.pred = em.pred;
    }
    // stable: the given (leading-base) order inside a class.  A counting sort of our own: the library's radix sort kernels (20 KB
    // of LDS, 100 VGPRs) do not start beside the other batch's resident search launch (ps_budget.h)
    launch_order_sort(key, n, wk->ws_get<uint32_t>("order_tmp", order_sort_tmp_words(n)), order, s);
    PS_HIP(hipGetLastError());
    t->stop(s);
    a.order = order; a.est = est; a.est_ab = ea.est_ab; ob.key = key;
}

// ragged launch: every read's own budget, by its length -- one table for the order's model and the search
static const uint8_t *upload_units_by_len(Batch &b)
{
    uint8_t *tab = b.wk->pin_get<uint8_t>("units_by_len_h", 256), *d_tab = b.wk->ws_get<uint8_t>("units_by_len", 256);
    budget_units_by_len(b.ctx->opt, tab);
    PS_HIP(hipMemcpyAsync(d_tab, tab, 256, hipMemcpyHostToDevice, b.wk->stream));
    return d_tab;
}

// Step 3: the geometry (ps_search_plan.h) and what it sizes -- the lanes' stacks, the large slots, the queue counters
static SearchPlan search_stacks(Batch &b, BtArgs &a, const SearchKnobs &kn, int lm)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    const SearchPlan p = plan_search(a.n_reads, lm, a.pool_cap, a.wide != 0, ctx->cus, ctx->bt_blocks, kn.max_per_cu, ctx->n_big);
    a.n_lanes = p.lanes;
    a.pool = wk->ws_get<uint8_t>("pool", p.pool_bytes);
    a.heads = a.wide ? wk->ws_get<uint32_t>("heads", p.head_words) : nullptr;
    a.queue = wk->ws_get<uint32_t>("queue", 16);
    PS_HIP(hipMemsetAsync(a.queue, 0, 64, s));
    if (p.n_big) {                                               // large slots for the reads that outgrow their private slice
        a.big_cap = PS_BIG_CAP; a.n_big = p.n_big;
        a.big_pool = wk->ws_get<uint8_t>("big_pool", p.big_bytes);
        a.big_next = a.queue + 4;                                // second counter in the zeroed queue words
        a.big_busy = wk->ws_get<uint32_t>("big_busy", a.n_big);
        PS_HIP(hipMemsetAsync(a.big_busy, 0, (size_t)a.n_big * 4, s));
    }
    return p;
}

// width + backtracking kernels over n reads of one length that are already packed on the device
static void run_search(Batch &b, const SearchKnobs &kn, const Model &md, int n, const uint32_t *d_bases, const uint32_t *d_nmask, const int32_t *d_lens,
                       uint32_t pool_cap, int aln_cap, AlnRec *alns, int32_t *n_aln, uint8_t *status, bool first_tier = false, const int32_t *launch_ids = nullptr)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    const int len = md.len;
    const bool wide = launch_is_wide(md, pool_cap);
    BtArgs a; std::memset(&a, 0, sizeof a);
    a.ix = ctx->ix.view; a.md = md; a.n_reads = n; a.len = len; a.lens = d_lens;
    a.bases = d_bases; a.nmask = d_nmask; a.n_bw = (len + 15) / 16; a.n_mw = (len + 31) / 32;
    a.alns = alns; a.aln_cap = aln_cap; a.n_aln = n_aln; a.status = status;
    a.pool_cap = pool_cap; a.wide = wide ? 1 : 0; a.stats = b.d_stats.p + 1; a.fetch_min = kn.fetch_min; a.hit_min = kn.hit_min;
    a.no_skip = kn.skip ? 0 : 1; a.no_chase = kn.chase ? 0 : 1; a.chase_min2 = kn.chase_min2;
    // width -> effort -> model -> sort -> search launch go to the stream back to back: the host reads the stage times only after
    // the search launch's own end (a wait after every stage put a host round trip, each behind a full machine, in front of the launch)
    EventPair t_width; std::optional<EventPair> t_order;
    search_width(b, a, t_width);
    if (d_lens) a.units_by_len = upload_units_by_len(b);
    OrderBufs ob;
    search_order(b, a, kn, t_order, ob);
    // the estimate also spares the search entries (ps_narrow.h, nt_tail): first tier and profile costs only (units == score); a read it fails on starts over without it inside the launch
    a.cap_est = (first_tier && !wide && a.est && md.profile && kn.cap) ? 1 + kn.cap_bias : 0;
    const int lm = lm_bytes(len, md.seed_len, md.n_buckets, wide);
    const SearchPlan p = search_stacks(b, a, kn, lm);
    if (ctx->want_read_iters) { a.read_iters = wk->ws_get<uint32_t>("riters", (size_t)n * PS_RI_WORDS); PS_HIP(hipMemsetAsync(a.read_iters, 0, (size_t)n * PS_RI_WORDS * 4, s)); }
    // step 4: the launch; the times of all stages are read behind it
    EventPair t(s);
    if (!launch_backtrack(a, wk->ws_get<BtArgs>("btargs", 1), wk->pin_get<BtArgs>("btargs_h", 1), p.blocks, lm, s, ctx->want_kstats || ctx->want_read_iters)) throw Error("cost model outside the ranges the search kernel packs (gap/score fields must fit a byte)");
    PS_HIP(hipGetLastError());
    t.stop(s);
    const double ms = t.ms(); b.tm.ms_backtrack += ms; ++b.tm.n_backtrack_launches;
    b.tm.ms_width += t_width.ms();
    if (t_order) b.tm.ms_width += t_order->ms();                     // reported with the width stage: both prepare the search
    { double t0_ = 0, t1_ = 0; t.span(ctx->ref_event, t0_, t1_); if (b.tm.n_backtrack_launches == 1) b.tm.bt_begin_ms = t0_; b.tm.bt_end_ms = t1_; }
    if (std::getenv("PS_VERBOSE")) std::fprintf(stderr, "[parasuite-hip]   backtrack launch: %d reads x %d bp, stack %u%s, %d lanes, %.1f ms\n", n, len, pool_cap, wide ? " (wide)" : "", p.lanes, ms);
    if (ctx->want_read_iters) {
        ctx->read_iters.resize((size_t)n * PS_RI_WORDS); PS_HIP(hipMemcpyAsync(ctx->read_iters.data(), a.read_iters, (size_t)n * PS_RI_WORDS * 4, hipMemcpyDeviceToHost, s));
        // what the launch was prepared with (ps_ctx_launch_order): nothing where it made no order
        Ctx::LaunchOrder &lo = ctx->launch_order;
        lo.clear();
        if (a.order) {
            lo.est.resize((size_t)n); lo.key.resize((size_t)n); lo.pred.assign((size_t)n, 0.f); lo.order.resize((size_t)n); lo.ids.resize((size_t)n);
            PS_HIP(hipMemcpyAsync(lo.est.data(), a.est, (size_t)n, hipMemcpyDeviceToHost, s));
            PS_HIP(hipMemcpyAsync(lo.key.data(), ob.key, (size_t)n, hipMemcpyDeviceToHost, s));
            if (ob.pred) PS_HIP(hipMemcpyAsync(lo.pred.data(), ob.pred, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            PS_HIP(hipMemcpyAsync(lo.order.data(), a.order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            for (int r = 0; r < n; ++r) lo.ids[(size_t)r] = launch_ids ? launch_ids[r] : r;
        }
        PS_HIP(hipStreamSynchronize(s));
    }
}

// download the hit lists of n reads (stride aln_cap on the device) in compact form
static void download_alns(Work *wk, int n, int aln_cap, const AlnRec *d_alns, const int32_t *d_n_aln,
                          std::vector<int32_t> &n_aln, std::vector<uint32_t> &off, std::vector<AlnRec> &alns)
{
    hipStream_t s = wk->stream;
    uint32_t *cnt = wk->ws_get<uint32_t>("cnt", n), *d_off = wk->ws_get<uint32_t>("off", (size_t)n + 1);
    hipLaunchKernelGGL(k_clip_counts, dim3((n + 255) / 256), dim3(256), 0, s, d_n_aln, aln_cap, n, cnt);
    size_t tb = 0;
    PS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, d_off, n, s));
    uint8_t *tmp = wk->ws_get<uint8_t>("scan_tmp", tb ? tb : 1);
    PS_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, d_off, n, s));
    int32_t *p_na = wk->pin_get<int32_t>("dl_n_aln", n); uint32_t *p_off = wk->pin_get<uint32_t>("dl_off", (size_t)n + 1);
    PS_HIP(hipMemcpyAsync(p_na, d_n_aln, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(p_off, d_off, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    uint32_t last = 0;
    if (n) { int m = p_na[n - 1]; last = p_off[n - 1] + (uint32_t)(m > aln_cap ? aln_cap : (m < 0 ? 0 : m)); }
    p_off[n] = last;
    n_aln.assign(p_na, p_na + n); off.assign(p_off, p_off + n + 1); alns.resize(last);
    if (last) {
        AlnRec *comp = wk->ws_get<AlnRec>("comp", last);
        hipLaunchKernelGGL(k_gather_alns, dim3((n + 255) / 256), dim3(256), 0, s, d_alns, aln_cap, d_n_aln, d_off, n, comp);
        AlnRec *p_al = wk->pin_get<AlnRec>("dl_alns", last);
        PS_HIP(hipMemcpyAsync(p_al, comp, (size_t)last * sizeof(AlnRec), hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        std::memcpy(alns.data(), p_al, (size_t)last * sizeof(AlnRec));
    }
}

// Read classes for the tie-break stream (one drand48 stream over all reads in input order):
//   0 no hit (no draw) | 1 exactly one best-score SA interval (always two draws) | 2 several (data dependent)
// bit 2 (PS_CLS_HOST, ps_pipeline.h): the read is finished on the host -- class 2 (sequential chain), reads that list
// alternative hits (XA), reads that needed a larger search tier.  Everything else never leaves the GPU.
__global__ void k_classify(const AlnRec *alns, int aln_cap, const int32_t *n_aln, const uint8_t *status, const int32_t *ids,
                           int n, int n_occ, uint8_t *cls_out)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        uint8_t c = 0;
        if (status[r] != RS_OK) c = 3 | PS_CLS_HOST;        // hit list lives on the host (larger tier): class fixed there
        else {
            const int na = n_aln[r];
            if (na > 0) {
                const AlnRec *al = alns + (size_t)r * aln_cap;
                const int best = al[0].score;
                int nb = 0; unsigned long long tot = 0;
                for (int j = 0; j < na; ++j) { if (al[j].score == best && nb == j) ++nb; tot += (unsigned long long)(al[j].l - al[j].k) + 1ull; }
                c = nb == 1 ? 1 : 2;
                if (c == 2 || (n_occ > 0 && tot >= 2 && tot <= (unsigned long long)n_occ + 1ull)) c |= PS_CLS_HOST;
            }
        }
        cls_out[ids[r]] = c;
    }
}
__global__ void k_gather_sub(const AlnRec *alns, int aln_cap, const int32_t *n_aln, const int32_t *local, int m, AlnRec *out, int32_t *n_out)
{
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += gridDim.x * blockDim.x) {
        const int r = local[q]; int na = n_aln[r]; if (na > aln_cap) na = aln_cap;
        n_out[q] = na;
        for (int j = 0; j < na; ++j) out[(size_t)q * aln_cap + j] = alns[(size_t)r * aln_cap + j];
    }
}

// The big allocations of a lane of work (tier-1 stack slices, the large stack slots) made ahead of its first search: a
// hipMalloc of tens of GB synchronises the device, so when a second worker makes its own while the first worker's search kernel
// runs it waits for that kernel (seen as a 1-2 s stall of a piece).  ps_map calls this when a worker starts, before any search.
void reserve_search_workspace(Ctx *ctx, int work_index)
{
    require_device(ctx->device);
    Work *wk = ctx->work_at(work_index);
    const SearchPlan p = plan_search_reserve(ctx->pool_cap[0], ctx->cus, ctx->bt_blocks, ctx->n_big);
    if (p.pool_bytes) (void)wk->ws_get<uint8_t>("pool", p.pool_bytes);
    if (p.n_big) {
        (void)wk->ws_get<uint8_t>("big_pool", p.big_bytes);
        (void)wk->ws_get<uint32_t>("big_busy", p.n_big);
    }
}

// The first tier of a bin with its identical reads searched once (ps_collapse.h, ps_collapse.hip): the groups on the device, one
// representative per group through run_search() as it stands, the result copied to every read of the group -- from there on
// the status download, k_classify, the hit-list downloads and the samse stage see what they would have seen.  false: the bin has
// no duplicate (m == n) and is to be searched in place; nothing was gathered.  All scratch is the lane's (a fresh hipMalloc
// synchronises the device: reserve_search_workspace).
static bool search_bin_collapsed(Batch &b, const SearchKnobs &kn, Bin &bin)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    const int n = (int)bin.ids.size();
    ps_collapse_info &ci = b.collapse;
    ci.n_reads += n; ++ci.n_bins;
    if (n < 2) { ci.n_searched += n; ci.n_groups += n; ci.largest = std::max<int64_t>(ci.largest, n); return false; }
    CollapseArgs ca;
    ca.n = n; ca.n_bw = bin.n_bw; ca.n_mw = bin.n_mw; ca.len = bin.len; ca.hash_bits = kn.collapse_hash_bits;
    ca.lens = bin.ragged ? bin.d_lens.p : nullptr; ca.bases = bin.bases.p; ca.nmask = bin.nmask.p;
    ca.key = wk->ws_get<uint64_t>("cl_key", (size_t)n);
    ca.perm[0] = wk->ws_get<int32_t>("cl_perm0", (size_t)n); ca.perm[1] = wk->ws_get<int32_t>("cl_perm1", (size_t)n);
    ca.digit = wk->ws_get<uint8_t>("cl_digit", (size_t)n); ca.order = wk->ws_get<int32_t>("cl_order", (size_t)n);
    ca.sort_tmp = wk->ws_get<uint32_t>("cl_sort_tmp", order_sort_tmp_words(n));
    ca.part = wk->ws_get<uint32_t>("cl_part", (size_t)2 * PS_SORT_MAX_WG + 1); ca.m = ca.part + 2 * PS_SORT_MAX_WG;
    ca.rep_of = wk->ws_get<int32_t>("cl_rep_of", (size_t)n); ca.slot = wk->ws_get<int32_t>("cl_slot", (size_t)n); ca.reps = wk->ws_get<int32_t>("cl_reps", (size_t)n);
    uint32_t *h_m = wk->pin_get<uint32_t>("cl_m", 1);
    EventPair t_groups(s);
    launch_collapse_groups(ca, s);
    PS_HIP(hipGetLastError());
    t_groups.stop(s);
    PS_HIP(hipMemcpyAsync(h_m, ca.m, 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    ci.ms_collapse += t_groups.ms();
    const int m = (int)*h_m;
    if (m < 1 || m > n) throw Error("internal: collapsed search counted more groups than reads");
    ci.n_searched += m; ci.n_groups += m;
    if (m == n) { ci.largest = std::max<int64_t>(ci.largest, 1); return false; }
    ++ci.n_bins_collapsed;
    uint32_t *g_bases = wk->ws_get<uint32_t>("cl_bases", (size_t)bin.n_bw * m), *g_nmask = wk->ws_get<uint32_t>("cl_nmask", (size_t)bin.n_mw * m);
    int32_t *g_lens = bin.ragged ? wk->ws_get<int32_t>("cl_lens", (size_t)m) : nullptr;
    AlnRec *t_alns = wk->ws_get<AlnRec>("cl_alns", (size_t)m * bin.aln_cap);
    int32_t *t_n_aln = wk->ws_get<int32_t>("cl_n_aln", (size_t)m); uint8_t *t_status = wk->ws_get<uint8_t>("cl_status", (size_t)m);
    EventPair t_gather(s);
    launch_collapse_gather(ca, m, g_bases, g_nmask, g_lens, s);
    PS_HIP(hipGetLastError());
    t_gather.stop(s);
    bin.h_rep_of.resize((size_t)n);
    PS_HIP(hipMemcpyAsync(bin.h_rep_of.data(), ca.rep_of, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    run_search(b, kn, bin.md, m, g_bases, g_nmask, g_lens, ctx->pool_cap[0], bin.aln_cap, t_alns, t_n_aln, t_status, true);
    EventPair t_expand(s);
    launch_collapse_expand(ca, m, t_alns, t_n_aln, t_status, bin.aln_cap, bin.d_alns.p, bin.d_n_aln.p, bin.d_status.p, s);
    PS_HIP(hipGetLastError());
    t_expand.stop(s);
    ci.ms_collapse += t_gather.ms() + t_expand.ms();                 // waits for the expansion, and with it for the download of rep_of
    std::vector<int32_t> size((size_t)n, 0);
    for (int r = 0; r < n; ++r) {
        const int32_t rep = bin.h_rep_of[(size_t)r];
        if (rep < 0 || rep >= n || bin.h_rep_of[(size_t)rep] != rep) throw Error("internal: collapsed search left a read without a representative");
        ++size[(size_t)rep];
    }
    for (int r = 0; r < n; ++r) { ci.n_multi += size[(size_t)r] > 1; ci.largest = std::max<int64_t>(ci.largest, size[(size_t)r]); }
    return true;
}

// step 1 of batch_search, per bin: the first tier, then the larger tiers for the reads it could not hold (their hit lists go to bin.overflow)
static void search_bin(Batch &b, const SearchKnobs &kn, Bin &bin)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    const int n = (int)bin.ids.size();
    bin.host_alns_valid = false; bin.h_rep_of.clear();
    const int cap1 = (bin.len <= 40 && ctx->aln_cap_short > ctx->aln_cap[0]) ? ctx->aln_cap_short : ctx->aln_cap[0];
    if (bin.d_alns.n < (size_t)n * cap1 || bin.aln_cap != cap1) { bin.d_alns.alloc((size_t)n * cap1); bin.d_n_aln.alloc(n); bin.d_status.alloc(n); }
    bin.aln_cap = cap1;
    if (!b.collapse_on || !search_bin_collapsed(b, kn, bin))
        run_search(b, kn, bin.md, n, bin.bases.p, bin.nmask.p, bin.ragged ? bin.d_lens.p : nullptr, ctx->pool_cap[0], bin.aln_cap, bin.d_alns.p, bin.d_n_aln.p, bin.d_status.p, true, bin.ids.data());
    // collapsed: the larger tiers search the representatives alone -- a read whose search overflowed is the dearest kind, and all its
    // duplicates overflow with it -- and a group's members take the representative's list afterwards; size[rep]: reads it stands for
    const std::vector<int32_t> &rep_of = bin.h_rep_of;
    std::vector<int32_t> size;
    if (!rep_of.empty()) { size.assign((size_t)n, 0); for (int r = 0; r < n; ++r) ++size[(size_t)rep_of[(size_t)r]]; }
    uint8_t *h_status = wk->pin_get<uint8_t>("status", n);
    PS_HIP(hipMemcpyAsync(h_status, bin.d_status.p, (size_t)n, hipMemcpyDeviceToHost, s));
    hipLaunchKernelGGL(k_classify, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, s, bin.d_alns.p, bin.aln_cap, bin.d_n_aln.p, bin.d_status.p,
                       bin.d_ids.p, n, ctx->opt.n_occ, b.d_class.p);
    PS_HIP(hipStreamSynchronize(s));
    bin.overflow.clear();
    // reads that need a deeper stack / a longer hit list: the second narrow tier, then the wide one.  A read whose stack outgrew
    // 65,535 entries already (RS_OVERFLOW_DEEP: on a large slot of the first launch) skips the second tier, which has no more than
    // that: on a repeat-rich genome those are the longest searches of the batch, and every tier starts them from scratch
    std::vector<int32_t> todo, deep;
    for (int r = 0; r < n; ++r) {
        if (h_status[r] == RS_BAD_SCORE) throw Error("internal: score outside the bucket range");
        if (h_status[r] != RS_OK && (rep_of.empty() || rep_of[(size_t)r] == r)) (h_status[r] == RS_OVERFLOW_DEEP ? deep : todo).push_back(r);
    }
    for (int tier = 1; tier < 3; ++tier) {
        if (tier == 2) { todo.insert(todo.end(), deep.begin(), deep.end()); std::sort(todo.begin(), todo.end()); deep.clear(); }
        if (todo.empty()) continue;
        const int m = (int)todo.size();
        int64_t stood_for = m;                                      // the counter keeps counting reads
        if (!size.empty()) { stood_for = 0; for (int32_t r : todo) stood_for += size[(size_t)r]; }
        b.n_overflow[tier] += stood_for;
        if (b.collapse_on) { b.collapse.n_overflow_reads += stood_for; b.collapse.n_overflow_searched += m; }
        std::vector<uint32_t> hb((size_t)bin.n_bw * m), hm((size_t)bin.n_mw * m);
        for (int q = 0; q < m; ++q) {
            for (int wv = 0; wv < bin.n_bw; ++wv) hb[(size_t)wv * m + q] = bin.h_bases[(size_t)wv * n + todo[q]];
            for (int wv = 0; wv < bin.n_mw; ++wv) hm[(size_t)wv * m + q] = bin.h_nmask[(size_t)wv * n + todo[q]];
        }
        DevBuf<uint32_t> db, dm; db.alloc(hb.size()); dm.alloc(hm.size());
        db.upload(hb.data(), hb.size(), s); dm.upload(hm.data(), hm.size(), s);
        std::vector<int32_t> hl(m); DevBuf<int32_t> dl;
        if (bin.ragged) { for (int q = 0; q < m; ++q) hl[q] = bin.lens[todo[q]]; dl.alloc(m); dl.upload(hl.data(), m, s); }
        DevBuf<AlnRec> ta; DevBuf<int32_t> tn; DevBuf<uint8_t> ts;
        ta.alloc((size_t)m * ctx->aln_cap[tier]); tn.alloc(m); ts.alloc(m);
        std::vector<int32_t> tid;
        if (ctx->want_read_iters) { tid.resize((size_t)m); for (int q = 0; q < m; ++q) tid[(size_t)q] = bin.ids[(size_t)todo[q]]; }
        run_search(b, kn, bin.md, m, db.p, dm.p, bin.ragged ? dl.p : nullptr, ctx->pool_cap[tier], ctx->aln_cap[tier], ta.p, tn.p, ts.p, false, tid.empty() ? nullptr : tid.data());
        std::vector<uint8_t> st(m); ts.download(st.data(), m, s);
        std::vector<int32_t> na; std::vector<uint32_t> off; std::vector<AlnRec> al;
        download_alns(wk, m, ctx->aln_cap[tier], ta.p, tn.p, na, off, al);
        std::vector<int32_t> still;
        for (int q = 0; q < m; ++q) {
            if (st[q] == RS_BAD_SCORE) throw Error("internal: score outside the bucket range");
            if (st[q] != RS_OK) { still.push_back(todo[q]); continue; }
            bin.overflow[todo[q]] = std::vector<AlnRec>(al.begin() + off[q], al.begin() + off[q + 1]);
        }
        todo.swap(still);
    }
    if (!todo.empty()) throw Error("a read exceeded the largest search tier (stack or hit capacity)");
    if (!rep_of.empty() && !bin.overflow.empty())
        for (int r = 0; r < n; ++r)
            if (rep_of[(size_t)r] != r) { auto it = bin.overflow.find(rep_of[(size_t)r]); if (it != bin.overflow.end()) bin.overflow[r] = it->second; }
}

// step 2: the classes on the host (larger-tier reads: from their host-side hit list), the number of class-1 / class-2 reads in front
// of every read the host finishes (Batch::sub, hit lists not yet attached) and in front of every group of 64 reads
static void classes_and_counts(Batch &b)
{
    Ctx *ctx = b.ctx; hipStream_t s = b.wk->stream;
    const int64_t N = b.rs.n;
    b.h_class = (uint8_t *)b.p_class.get((size_t)N + 64);
    PS_HIP(hipMemcpyAsync(b.h_class, b.d_class.p, (size_t)N, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    bool patched = false;
    for (Bin &bin : b.bins)
        for (auto &kv : bin.overflow) {                       // larger-tier reads: class from their host-side hit list
            const std::vector<AlnRec> &al = kv.second;
            int nb = 0;
            for (; nb < (int)al.size() && al[nb].score == al[0].score; ++nb) {}
            b.h_class[bin.ids[kv.first]] = (uint8_t)((al.empty() ? 0 : (nb == 1 ? 1 : 2)) | PS_CLS_HOST);
            patched = true;
        }
    if (patched) PS_HIP(hipMemcpyAsync(b.d_class.p, b.h_class, (size_t)N, hipMemcpyHostToDevice, s));
    b.sub.clear(); b.n_class1 = 0; b.n_hard = 0;
    // pass 1: per range, the number of class-1 / class-2 reads and of reads the host finishes
    const int nt = par_threads((size_t)N, ctx->host_threads);
    std::vector<int64_t> ce(nt + 1, 0), ch(nt + 1, 0), cs(nt + 1, 0);
    par_for((size_t)N, ctx->host_threads, [&](size_t g0, size_t g1, int t) {
        int64_t e = 0, h = 0, sn = 0;
        for (size_t g = g0; g < g1; ++g) { const uint8_t c = b.h_class[g]; e += (c & 3) == 1; h += (c & 3) == 2; sn += (c & PS_CLS_HOST) != 0; }
        ce[t + 1] = e; ch[t + 1] = h; cs[t + 1] = sn;
    });
    for (int t = 0; t < nt; ++t) { ce[t + 1] += ce[t]; ch[t + 1] += ch[t]; cs[t + 1] += cs[t]; }
    b.n_class1 = ce[nt]; b.n_hard = ch[nt];
    b.sub.resize((size_t)cs[nt]);
    // pass 2: the subset with its position in the tie-break stream, and the two counts in front of every group of 64 reads
    // (batch_select_easy: the device adds the rank inside a group)
    b.h_grp = (uint32_t *)b.p_grp.get((((size_t)N + 63) / 64 * 2 + 2) * sizeof(uint32_t));
    par_for((size_t)N, ctx->host_threads, [&](size_t g0, size_t g1, int t) {
        int64_t e = ce[t], h = ch[t]; size_t q = (size_t)cs[t];
        for (size_t g = g0; g < g1; ++g) {
            const uint8_t c = b.h_class[g];
            if ((g & 63) == 0) { b.h_grp[2 * (g >> 6)] = (uint32_t)e; b.h_grp[2 * (g >> 6) + 1] = (uint32_t)h; }
            if (c & PS_CLS_HOST) { SubRead &sr = b.sub[q++]; sr = SubRead(); sr.g = (int64_t)g; sr.cls = c & 3; sr.easy_before = e; sr.hard_before = h; }
            e += (c & 3) == 1; h += (c & 3) == 2;
        }
    });
}

// step 3: hit lists of the subset: gathered on the device in subset order, one pinned download per bin
static void gather_sub_alns(Batch &b)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    std::vector<std::vector<int32_t>> want(b.bins.size());
    std::vector<int32_t> slot(b.sub.size(), -1);
    for (size_t q = 0; q < b.sub.size(); ++q) {
        const SubRead &sr = b.sub[q];
        const int bi = b.read_bin[sr.g]; const Bin &bin = b.bins[bi];
        if (bin.overflow.empty() || !bin.overflow.count(b.read_local[sr.g])) { slot[q] = (int32_t)want[bi].size(); want[bi].push_back(b.read_local[sr.g]); }
    }
    b.sub_alns.resize(b.bins.size());
    std::vector<const AlnRec *> got(b.bins.size(), nullptr); std::vector<const int32_t *> got_n(b.bins.size(), nullptr);
    for (size_t bi = 0; bi < b.bins.size(); ++bi) {
        const int m = (int)want[bi].size();
        if (!m) continue;
        Bin &bin = b.bins[bi];
        int32_t *d_loc = wk->ws_get<int32_t>("sub_local", m); AlnRec *d_out = wk->ws_get<AlnRec>("sub_alns", (size_t)m * bin.aln_cap);
        int32_t *d_no = wk->ws_get<int32_t>("sub_n", m);
        PS_HIP(hipMemcpyAsync(d_loc, want[bi].data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_gather_sub, dim3((m + 255) / 256), dim3(256), 0, s, bin.d_alns.p, bin.aln_cap, bin.d_n_aln.p, d_loc, m, d_out, d_no);
        if (!b.sub_alns[bi]) b.sub_alns[bi].reset(new PinBuf());
        const size_t bytes_al = (size_t)m * bin.aln_cap * sizeof(AlnRec);
        uint8_t *hp = (uint8_t *)b.sub_alns[bi]->get(bytes_al + (size_t)m * 4 + 64);
        PS_HIP(hipMemcpyAsync(hp, d_out, bytes_al, hipMemcpyDeviceToHost, s));
        PS_HIP(hipMemcpyAsync(hp + bytes_al, d_no, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        got[bi] = reinterpret_cast<const AlnRec *>(hp); got_n[bi] = reinterpret_cast<const int32_t *>(hp + bytes_al);
    }
    PS_HIP(hipStreamSynchronize(s));
    par_for(b.sub.size(), ctx->host_threads, [&](size_t q0, size_t q1, int) {
        for (size_t q = q0; q < q1; ++q) {
            SubRead &sr = b.sub[q];
            const int bi = b.read_bin[sr.g]; Bin &bin = b.bins[bi];
            if (slot[q] < 0) { const std::vector<AlnRec> &v = bin.overflow.find(b.read_local[sr.g])->second; sr.alns = v.data(); sr.n_alns = (int32_t)v.size(); }
            else { sr.alns = got[bi] + (size_t)slot[q] * bin.aln_cap; sr.n_alns = got_n[bi][slot[q]]; }
        }
    });
}

void batch_search(Batch &b)
{
    Ctx *ctx = b.ctx; hipStream_t s = b.wk->stream;
    require_device(ctx->device);
    const SearchKnobs kn = search_knobs_from_env(ctx->fetch_min, ctx->hit_min);     // the one place the search stage reads its environment
    b.tm = Timing();
    auto t0 = HostClock::now();
    b.d_stats.zero(s);
    for (int t = 0; t < 3; ++t) b.n_overflow[t] = 0;
    // identical reads searched once: the context's word, else the environment's; not with the per-read profile, which is in launch order
    b.collapse_on = (ctx->collapse_mode < 0 ? kn.collapse : ctx->collapse_mode > 0) && !ctx->want_read_iters;
    b.collapse = ps_collapse_info();
    if (b.d_class.n < (size_t)b.rs.n) b.d_class.alloc((size_t)b.rs.n);
    for (Bin &bin : b.bins) search_bin(b, kn, bin);
    KStats hs[3];
    b.d_stats.download(hs, 3, s);
    // classes to the host; the host-finished subset and its position in the tie-break stream
    auto tcl = HostClock::now();
    classes_and_counts(b);
    b.st_width = hs[0]; b.st_backtrack = hs[1];                  // behind the wait in classes_and_counts: the download above is asynchronous
    gather_sub_alns(b);
    b.tm.ms_classify = ms_since(tcl);
    if (!b.collapse_on) b.collapse.n_reads = b.collapse.n_searched = b.rs.n;
    b.collapse_known = true;
    if (b.collapse_on && std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip]   collapsed search: %lld reads, %lld searched, %lld groups, largest %lld, %.2f ms\n", (long long)b.collapse.n_reads,
                     (long long)b.collapse.n_searched, (long long)b.collapse.n_groups, (long long)b.collapse.largest, b.collapse.ms_collapse);
    b.searched = true; b.selected_hard = b.selected = b.located = false;
    b.tm.ms_total = ms_since(t0);
}

void Batch::ensure_host_alns()
{
    require_device(ctx->device);
    for (Bin &bin : bins) {
        if (bin.host_alns_valid) continue;
        download_alns(wk, (int)bin.ids.size(), bin.aln_cap, bin.d_alns.p, bin.d_n_aln.p, bin.h_n_aln, bin.h_off, bin.h_alns);
        for (auto &kv : bin.overflow) bin.h_n_aln[kv.first] = (int32_t)kv.second.size();
        bin.host_alns_valid = true;
    }
}
const AlnRec *Batch::alns_of(int64_t g, int &n)
{
    ensure_host_alns();
    const Bin &bin = bins[read_bin[g]];
    int32_t r = read_local[g];
    n = bin.h_n_aln[r];
    if (!bin.overflow.empty()) {
        auto it = bin.overflow.find(r);
        if (it != bin.overflow.end()) return it->second.data();
    }
    return bin.h_alns.data() + bin.h_off[r];
}

}  // namespace ps
