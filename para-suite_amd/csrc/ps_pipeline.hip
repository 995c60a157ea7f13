// ps_pipeline.hip -- host orchestration of one mapping job.
//
// Replaces what the reference runs as two child processes,
//   bwa parasuite|aln ... -f P.sai     PARAsuiteMapping.java:63-77 / BWAMapping.java:51-61
//   bwa samse ref P.sai fq -f P.sam    PARAsuiteMapping.java:85-92 / BWAMapping.java:68-75
// by one pass: reads binned by length and 2-bit packed in HBM -> width kernel ->
// backtracking kernel -> tie-break selection (one drand48 stream in input order)
// -> SA-walk kernel -> banded-DP kernel for gapped hits -> SAM text.
// No stage has a CPU implementation of the kernels' work: without a HIP device
// every entry point fails.
#include <hip/hip_runtime.h>
#include <mutex>
#include <optional>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include "ps_pipeline.h"
#include "ps_par.h"
#include "ps_core.h"

namespace ps {

typedef std::chrono::steady_clock Clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

void require_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) throw Error("no HIP device available: parasuite-hip has no CPU path");
    if (device < 0 || device >= n) throw Error("HIP device index out of range");
    PS_HIP(hipSetDevice(device));
}

Ctx::Ctx(int device_) : device(device_)
{
    if (const char *e = std::getenv("PS_FETCH_MIN")) fetch_min = std::atoi(e);       // tuning knobs
    if (const char *e = std::getenv("PS_N_BIG")) n_big = std::atoi(e);
    if (const char *e = std::getenv("PS_HIT_MIN")) hit_min = std::atoi(e);
    if (std::getenv("PS_READ_ITERS")) want_read_iters = true;
    if (std::getenv("PS_KSTATS")) want_kstats = true;
    if (const char *e = std::getenv("PS_BT_BLOCKS")) bt_blocks = std::atoi(e);
    if (const char *e = std::getenv("PS_POOL_CAP")) pool_cap[0] = (uint32_t)std::atoi(e);
    if (const char *e = std::getenv("PS_ALN_CAP")) { aln_cap[0] = std::max(1, std::atoi(e)); aln_cap_short = 0; }   // hit intervals a read may list in the first tier (stated: for every length)
}
void Ctx::attach_device()
{
    require_device(device);
    if (stream) return;
    PS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    PS_HIP(hipEventCreate(&ref_event)); PS_HIP(hipEventRecord(ref_event, stream)); PS_HIP(hipEventSynchronize(ref_event));
}
void Ctx::set_stock(const char *n_arg)
{
    Options o; set_stock_n(o, n_arg);
    if (o.max_diff < 0 && !(o.fnr > 0.0)) throw Error("bad -n argument");
    opt = o;
}
void Ctx::set_profile(const char *ep, const char *ip, const char *x_arg)
{
    double P[16], ins, del; std::string err;
    if (!read_profile_files(ep, ip, P, ins, del, err)) throw Error(err);
    Options o; profile_costs(o, P, ins, del, x_arg ? std::atoi(x_arg) : -1); opt = o;
}
Ctx::~Ctx() { if (ref_event) (void)hipEventDestroy(ref_event); if (stream) (void)hipStreamDestroy(stream); }
void ctx_release_device(Ctx &c)
{
    require_device(c.device);
    {
        std::lock_guard<std::mutex> l(c.work_mu);
        for (auto &w : c.work) w.reset();
    }
    c.ix.blocks.release(); c.ix.sa.release(); c.ix.pac.release(); c.ix.jump.release();     // the view keeps its (now dangling) device pointers: nothing may search with this context again
}
Work *Ctx::work_at(int w)
{
    std::lock_guard<std::mutex> l(work_mu);
    if (w < 0 || w >= (int)N_WORK) throw Error("internal: work lane out of range");
    if (!work[w]) { work[w].reset(new Work()); PS_HIP(hipStreamCreateWithFlags(&work[w]->stream, hipStreamNonBlocking)); }
    return work[w].get();
}
Work *Ctx::take_work()
{
    int w;
    { std::lock_guard<std::mutex> l(work_mu); w = next_work; next_work = (next_work + 1) % std::max(1, std::min(n_work, (int)N_WORK)); }
    return work_at(w);
}
namespace {
struct PinCache {
    std::mutex mu; std::vector<std::pair<void *, size_t>> kept; size_t held = 0;
    static constexpr size_t CAP = (size_t)3 << 30;            // bytes kept at most
};
PinCache &pin_cache() { static PinCache *c = new PinCache(); return *c; }   // never destroyed: buffers may be given back during exit
}
void *pin_cache_take(size_t need, size_t &got)
{
    PinCache &c = pin_cache();
    {
        std::lock_guard<std::mutex> l(c.mu);
        int best = -1;
        for (size_t i = 0; i < c.kept.size(); ++i)            // the smallest kept buffer that fits (the pieces of ps_map differ in size from call to call: a larger buffer than needed beats locking a new one)
            if (c.kept[i].second >= need && (best < 0 || c.kept[i].second < c.kept[(size_t)best].second)) best = (int)i;
        if (best >= 0) {
            void *p = c.kept[(size_t)best].first; got = c.kept[(size_t)best].second;
            c.held -= got; c.kept.erase(c.kept.begin() + best);
            return p;
        }
    }
    const size_t want = need + need / 8 + 4096;               // a little room: the next piece is rarely exactly as large
    void *p = nullptr;
    PS_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    got = want;
    return p;
}
void pin_cache_give(void *p, size_t bytes)
{
    if (!p) return;
    PinCache &c = pin_cache();
    {
        std::lock_guard<std::mutex> l(c.mu);
        if (c.held + bytes <= PinCache::CAP) { c.kept.emplace_back(p, bytes); c.held += bytes; return; }
    }
    (void)hipHostFree(p);
}
void pin_cache_release()
{
    PinCache &c = pin_cache();
    std::vector<std::pair<void *, size_t>> all;
    { std::lock_guard<std::mutex> l(c.mu); all.swap(c.kept); c.held = 0; }
    for (auto &e : all) (void)hipHostFree(e.first);
}

void Batch::release_device()
{
    for (Bin &bin : bins) {
        bin.bases.release(); bin.nmask.release(); bin.w.release(); bin.cwb.release(); bin.cswb.release(); bin.status.release();
        bin.alns.release(); bin.n_aln.release(); bin.d_lens.release(); bin.d_ids.release();
        bin.d_alns.release(); bin.d_n_aln.release(); bin.d_status.release();
    }
    d_class.release(); d_eb.release(); d_hb.release(); d_rows.release(); d_pos.release(); d_sel.release(); d_fin.release(); d_stats.release();
    searched = false;              // the batch can be written, not searched again
}

// ------------------------------------------------------------ batch set-up ---
// host half of batch_create: bins, order inside the bins, 2-bit packing -- no device call, so the parser thread of
// ps_map runs it while the GPU thread is busy with the piece before
std::unique_ptr<Batch> batch_prepare(Ctx *ctx, ReadSet &&rs_in, int threads)
{
    const auto t_prep0 = std::chrono::steady_clock::now();
    struct PrepTimes { double bins = 0, sort = 0, pack = 0; } pt;
    std::unique_ptr<Batch> b(new Batch());
    b->ctx = ctx; b->rs = std::move(rs_in);
    const ReadSet &rs = b->rs;
    // cost class of a length: everything of the search model that depends on the length except the length itself
    std::vector<int> class_of_len;                       // length -> bin (-1: not seen yet)
    std::map<std::vector<int>, int> bin_of_class;
    b->read_bin.resize((size_t)rs.n); b->read_local.resize((size_t)rs.n);
    for (int64_t g = 0; g < rs.n; ++g) {
        const int len = rs.len[g];
        if (len < 1) throw Error("empty read in input");
        if ((size_t)len >= class_of_len.size()) class_of_len.resize((size_t)len + 64, -1);
        int cls = class_of_len[(size_t)len];
        if (cls < 0) {
            Model md; std::string err;
            if (!make_model(ctx->opt, len, md, err)) throw Error(err);
            // What a launch needs to be uniform in: the seed rule and the gap limit.  The difference budget, the number of score buckets,
            // the packed word count and where the N mask lives follow the read (budget: BtArgs::units_by_len) or the longest read of
            // the bin (local-memory layout), so that adapter-trimmed input with dozens of lengths is ONE launch where it used to be
            // one per budget step -- every launch ends with ~0.2 s of emptying machine
            const std::vector<int> key = {md.max_gapo};      // the seed rule follows the read too (len > seed_len, checked per read by the kernels) since adapter-trimmed
                                                             // PAR-CLIP reads lie on both sides of the 32-base seed: 18-40 bp input is one launch, not two
            auto bc = bin_of_class.find(key);
            if (bc == bin_of_class.end()) { bc = bin_of_class.emplace(key, (int)b->bins.size()).first; b->bins.emplace_back(); }
            cls = class_of_len[(size_t)len] = bc->second;
        }
        Bin &bin = b->bins[(size_t)cls];
        if (bin.len && bin.len != len) bin.ragged = true;
        if (len > bin.len) bin.len = len;
        b->read_bin[g] = cls; b->read_local[g] = (int32_t)bin.ids.size();
        bin.ids.push_back((int32_t)g);
    }
    pt.bins = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count();
    for (Bin &bin : b->bins) {
        std::string err;
        if (!make_model(ctx->opt, bin.len, bin.md, err)) throw Error(err);
        // Order the reads of a bin by their leading bases (the search consumes a read from its first base): the
        // lanes of a wave then walk the same top levels of the BWT, so their Occ loads coalesce and hit in cache.
        // Results return to input order through ids[]; the order inside a bin is free.  (Handing the kernels a sorted
        // LIST instead and leaving the reads where they are cost the search kernel 1.6 % and the width stage 20 %:
        // profiles/r03_kernel_experiments.txt.)  An LSD radix sort over the first 16 bases, every pass on all threads:
        // counts per thread and digit, places from their prefix sums (stable), 0.15 s per 3.6 M reads when one thread did it.
        if (!std::getenv("PS_KEEP_ORDER")) {         // PS_KEEP_ORDER=1: the reads stay in input order (tools/order_probe.py hands them out in an order of its own)
            const size_t n = bin.ids.size();
            const int nt = par_threads(n, threads);
            std::vector<uint32_t> key(n), key2(n); std::vector<int32_t> id2(n);
            par_for(n, nt, [&](size_t r0, size_t r1, int) {
                for (size_t r = r0; r < r1; ++r) {
                    const uint8_t *sq = rs.seq.data() + rs.off[bin.ids[r]];
                    const int kb = rs.len[bin.ids[r]] < 16 ? rs.len[bin.ids[r]] : 16;
                    uint32_t k = 0;
                    for (int j = 0; j < kb; ++j) k = (k << 2) | (uint32_t)(sq[j] & 3);
                    key[r] = k << (2 * (16 - kb));
                }
            });
            std::vector<size_t> cnt((size_t)nt * 256);
            for (int sh = 0; sh < 32; sh += 8) {
                std::fill(cnt.begin(), cnt.end(), 0);
                par_for(n, nt, [&](size_t r0, size_t r1, int t) { size_t *c = cnt.data() + (size_t)t * 256; for (size_t r = r0; r < r1; ++r) ++c[(key[r] >> sh) & 0xff]; });
                size_t at = 0;
                for (int d = 0; d < 256; ++d) for (int t = 0; t < nt; ++t) { const size_t c = cnt[(size_t)t * 256 + d]; cnt[(size_t)t * 256 + d] = at; at += c; }
                par_for(n, nt, [&](size_t r0, size_t r1, int t) {
                    size_t *c = cnt.data() + (size_t)t * 256;
                    for (size_t r = r0; r < r1; ++r) { const size_t p = c[(key[r] >> sh) & 0xff]++; key2[p] = key[r]; id2[p] = bin.ids[r]; }
                });
                key.swap(key2); bin.ids.swap(id2);
            }
            par_for(n, nt, [&](size_t r0, size_t r1, int) { for (size_t r = r0; r < r1; ++r) b->read_local[bin.ids[r]] = (int32_t)r; });
        }
        const size_t n = bin.ids.size();
        pt.sort = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count() - pt.bins - pt.pack;
        bin.n_bw = (bin.len + 15) / 16; bin.n_mw = (bin.len + 31) / 32;
        bin.h_bases.resize((size_t)bin.n_bw * n); bin.h_nmask.resize((size_t)bin.n_mw * n);
        bin.lens.resize(n);
        {
            const int nt = std::max(1, std::min(threads, 64));
            auto pack = [&](int t) {                                  // distinct reads write distinct words: no sharing.  Whole words, bases behind the read's end 0
                // the reads come in leading-base order, i.e. from all over the piece: three dependent cache misses per read (its offset,
                // its length, its bases) unless they are asked for ahead (257 ms per 9.3 M reads on 16 threads without)
                const size_t r_end = n * (t + 1) / nt, AHEAD = 12;
                for (size_t r = n * t / nt; r < r_end; ++r) {
                    if (r + 2 * AHEAD < r_end) { const int32_t g2 = bin.ids[r + 2 * AHEAD]; __builtin_prefetch(&rs.off[g2]); __builtin_prefetch(&rs.len[g2]); }
                    if (r + AHEAD < r_end) { const uint8_t *q = rs.seq.data() + rs.off[bin.ids[r + AHEAD]]; __builtin_prefetch(q); __builtin_prefetch(q + 63); }
                    const uint8_t *s = rs.seq.data() + rs.off[bin.ids[r]];
                    const int rl = rs.len[bin.ids[r]];
                    bin.lens[r] = rl;
                    for (int p = 0; p < bin.n_bw; ++p) {
                        uint32_t wd = 0;
                        const int j1 = std::min(rl, 16 * p + 16);
                        for (int j = 16 * p; j < j1; ++j) if (s[j] <= 3) wd |= (uint32_t)s[j] << (2 * (j & 15));
                        bin.h_bases[(size_t)p * n + r] = wd;
                    }
                    for (int p = 0; p < bin.n_mw; ++p) {
                        uint32_t wd = 0;
                        const int j1 = std::min(rl, 32 * p + 32);
                        for (int j = 32 * p; j < j1; ++j) if (s[j] > 3) wd |= 1u << (j & 31);
                        bin.h_nmask[(size_t)p * n + r] = wd;
                    }
                }
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nt; ++t) th.emplace_back(pack, t);
            pack(0);
            for (auto &x : th) x.join();
        }
        pt.pack = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count() - pt.bins - pt.sort;
    }
    if (const char *e = std::getenv("PS_VERBOSE")) if (std::atoi(e) >= 2)
        std::fprintf(stderr, "[parasuite-hip]     piece of %lld reads made ready in %.0f ms (bins %.0f, leading-base sort %.0f, packing %.0f)\n", (long long)rs.n,
                     1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count(), 1e3 * pt.bins, 1e3 * pt.sort, 1e3 * pt.pack);
    return b;
}
// device half: allocate and upload
void batch_upload(Batch &bb)
{
    Batch *b = &bb; Ctx *ctx = b->ctx;
    require_device(ctx->device);
    b->wk = b->work_index >= 0 ? ctx->work_at(b->work_index) : ctx->take_work();
    Work *wk = b->wk;
    for (Bin &bin : b->bins) {
        const size_t n = bin.ids.size();
        if (bin.ragged) { bin.d_lens.alloc(n); bin.d_lens.upload(bin.lens.data(), n, wk->stream); }
        bin.d_ids.alloc(n); bin.d_ids.upload(bin.ids.data(), n, wk->stream);
        bin.bases.alloc(bin.h_bases.size()); bin.nmask.alloc(bin.h_nmask.size());
        bin.bases.upload(bin.h_bases.data(), bin.h_bases.size(), wk->stream);
        bin.nmask.upload(bin.h_nmask.data(), bin.h_nmask.size(), wk->stream);
    }
    b->d_stats.alloc(3);
    PS_HIP(hipStreamSynchronize(wk->stream));
}
std::unique_ptr<Batch> batch_create(Ctx *ctx, ReadSet &&rs_in)
{
    std::unique_ptr<Batch> b = batch_prepare(ctx, std::move(rs_in), ctx->host_threads);
    batch_upload(*b);
    return b;
}

// --------------------------------------------------------------- search -------
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

struct EvTimer {
    hipEvent_t a, b; hipStream_t s;
    explicit EvTimer(hipStream_t st) : s(st) { PS_HIP(hipEventCreate(&a)); PS_HIP(hipEventCreate(&b)); PS_HIP(hipEventRecord(a, s)); }
    double stop() { mark(); return read(); }
    // mark(): the end is recorded and the host goes on submitting; read(): the time, once the host has a reason to wait anyway
    void mark() { PS_HIP(hipEventRecord(b, s)); }
    double read() { PS_HIP(hipEventSynchronize(b)); float ms = 0; PS_HIP(hipEventElapsedTime(&ms, a, b)); return ms; }
    // begin / end on the context's clock (ms since its reference event): launches of two streams that overlap in time
    void span(hipEvent_t ref, double &t_begin, double &t_end) { float x = 0, y = 0; if (ref && hipEventElapsedTime(&x, ref, a) == hipSuccess && hipEventElapsedTime(&y, ref, b) == hipSuccess) { t_begin = x; t_end = y; } }
    ~EvTimer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
};


// width + backtracking kernels over n reads of one length that are already packed on the device
static void run_search(Batch &b, const Model &md, int n, const uint32_t *d_bases, const uint32_t *d_nmask, const int32_t *d_lens,
                       uint32_t pool_cap, int aln_cap, AlnRec *alns, int32_t *n_aln, uint8_t *status, bool first_tier = false)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    const int len = md.len, seed_len = md.seed_len;
    uint32_t *w = wk->ws_get<uint32_t>("w", (size_t)(len + 1) * n);
    uint32_t *cwb = wk->ws_get<uint32_t>("cwb", (size_t)lm_ncw(len) * n);
    uint32_t *cswb = wk->ws_get<uint32_t>("cswb", (size_t)(lm_ncsw(seed_len) + 1) * n);
    WidthArgs wa;
    wa.ix = ctx->ix.view; wa.n_reads = n; wa.len = len; wa.lens = d_lens; wa.seed_len = seed_len; wa.use_seed = md.use_seed;
    wa.bases = d_bases; wa.nmask = d_nmask; wa.w = w; wa.cwb = cwb; wa.cswb = cswb; wa.stats = b.d_stats.p + 0;
    // width -> effort -> model -> sort -> search launch go to the stream back to back: the host reads the stage times only after
    // the search launch's own end (a wait after every stage put a host round trip, each behind a full machine, in front of the launch)
    std::optional<EvTimer> t_width, t_order;
    t_width.emplace(s); launch_width(wa, s); PS_HIP(hipGetLastError()); t_width->mark(); ++b.tm.n_width_launches;
    const bool wide = launch_is_wide(md, pool_cap);
    // ---- hand-out order: the reads with the heaviest predicted search first (ps_effort.hip), so that the launch does not end on
    // them.  PS_ORDER=0 switches it off, 2 orders by the estimated best score alone (A/B runs).  Narrow launches only: the wide
    // stack takes its reads in queue order and never reads the estimate (its budget can also pass the 63 units k_effort_model
    // has lanes for: -X 10 and up)
    const int32_t *d_order = nullptr; const uint8_t *d_est = nullptr; const uint16_t *d_est_ab = nullptr;
    if (!wide) {
        const char *eo = std::getenv("PS_ORDER");
        const int mode = eo ? std::atoi(eo) : 1;
        int min_n = 4096;                                     // below that every read has a lane to itself at once: no order to choose
        if (const char *e = std::getenv("PS_ORDER_MIN")) min_n = std::max(1, std::atoi(e));      // tests: the small launches of the fuzz sweep too
        if (mode > 0 && n >= min_n && md.max_units >= md.c_min) {      // a search that can afford no difference is ~len steps for every read: nothing to order
            t_order.emplace(s);
            uint8_t *est = wk->ws_get<uint8_t>("est", (size_t)n), *key = wk->ws_get<uint8_t>("okey", (size_t)n);
            int32_t *order = wk->ws_get<int32_t>("order", (size_t)n);
            EffortArgs ea;
            ea.ix = ctx->ix.view; ea.n_reads = n; ea.len = len; ea.lens = d_lens; ea.bases = d_bases; ea.nmask = d_nmask; ea.est = est;
            // everything here is in BUDGET UNITS (what the search's limits are in): the profile model has units == score, stock counts
            // every difference as one unit whatever it scores
            int csum = 0;
            for (int c = 0; c < 5; ++c) ea.s_pk[c] = md.u_mm_pk[c];
            for (int sc = 0; sc < 4; ++sc) for (int tc = 0; tc < 4; ++tc) if (sc != tc) csum += md.u_mm[sc][tc];
            ea.c_restart = std::max(1, (csum + 6) / 12);                      // an average mismatch
            if (const char *e = std::getenv("PS_ORDER_RESTART")) ea.c_restart = std::max(1, std::atoi(e));
            ea.w_pin = 16;
            if (const char *e = std::getenv("PS_ORDER_WPIN")) ea.w_pin = (uint32_t)std::max(1, std::atoi(e));
            int lv = 0; while (lv < 31 && (ctx->ix.view.seq_len >> (2 * lv)) > 0) ++lv;              // 4^lv > rows: 17 at hg19 size
            ea.est_ab = ctx->want_read_iters ? wk->ws_get<uint16_t>("est_ab", (size_t)n) : nullptr;
            launch_effort(ea, s);
            d_est_ab = ea.est_ab;
            if (mode == 2) {
                int cap = 255;
                if (const char *e = std::getenv("PS_ORDER_CAP")) cap = std::max(1, std::min(255, std::atoi(e)));
                hipLaunchKernelGGL(k_order_keys, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, s, est, n, cap, key);
            } else {
                EffortModelArgs em;
                em.n_reads = n; em.len = len; em.lens = d_lens; em.units_by_len = nullptr; em.bases = d_bases; em.nmask = d_nmask; em.cwb = cwb; em.est = est;
                for (int c = 0; c < 5; ++c) em.s_pk[c] = md.u_mm_pk[c];
                em.inv_c_min = (uint32_t)md.inv_c_min; em.max_units = md.max_units; em.u_tight = md.u_tight;
                em.seed_units = md.max_seed_diff * md.u_tight; em.use_seed = md.use_seed; em.seed_len = md.seed_len;
                em.max_gapo = md.max_gapo; em.indel_end_skip = md.indel_end_skip; em.u_gapo_ins = md.u_gapo_ins; em.u_gapo_del = md.u_gapo_del;
                em.depth = lv + 3; em.rows = (float)ctx->ix.view.seq_len; em.log_scale = 8;
                if (const char *e = std::getenv("PS_ORDER_SCALE")) em.log_scale = std::max(1, std::min(12, std::atoi(e)));
                if (d_lens) {                                             // ragged launch: every read's own budget, by its length
                    uint8_t *tab = wk->pin_get<uint8_t>("units_by_len_h2", 256);
                    for (int l2 = 0; l2 < 256; ++l2) { const int u = budget_diffs(ctx->opt, l2) * (ctx->opt.profile ? ctx->opt.unit : 1); tab[l2] = (uint8_t)(u > 255 ? 255 : u); }
                    uint8_t *d_tab = wk->ws_get<uint8_t>("units_by_len2", 256);
                    PS_HIP(hipMemcpyAsync(d_tab, tab, 256, hipMemcpyHostToDevice, s));
                    em.units_by_len = d_tab;
                }
                em.key = key; em.pred = nullptr;
                launch_effort_model(em, s);
            }
            // stable: the given (leading-base) order inside a class.  A counting sort of our own: the library's radix sort kernels (20 KB
            // of LDS, 100 VGPRs) do not start beside the other batch's resident search launch (ps_budget.h)
            launch_order_sort(key, n, wk->ws_get<uint32_t>("order_tmp", order_sort_tmp_words(n)), order, s);
            PS_HIP(hipGetLastError());
            t_order->mark();
            d_order = order; d_est = est;
        }
    }
    int dev_cus = 256;
    { hipDeviceProp_t p; if (hipGetDeviceProperties(&p, ctx->device) == hipSuccess && p.multiProcessorCount > 0) dev_cus = p.multiProcessorCount; }
    const int lm = lm_bytes(len, seed_len, md.n_buckets, wide);
    int per_cu = (int)((size_t)(160 * 1024) / ((size_t)256 * lm));
    if (per_cu < 1) throw Error("read length / score range too large for the per-lane LDS state");
    { const char *e = std::getenv("PS_MAX_PER_CU"); const int cap = e ? std::atoi(e) : 4; if (per_cu > cap) per_cu = cap; }   // workgroups per CU the kernel's registers allow (ps_kernels.hip: PS_BT_WAVES)
    int blocks = ctx->bt_blocks > 0 ? ctx->bt_blocks : dev_cus * per_cu;
    int need = (n + 255) / 256;
    if (blocks > need) blocks = need;
    // bound the lanes by stack memory (the widest tier keeps 64 MB per lane)
    const size_t per_lane = (size_t)pool_cap * (wide ? sizeof(Entry) : 16) + (wide ? PS_MAX_BUCKETS * 4 : 0);
    const size_t max_lanes = ((size_t)(wide ? 32 : 64) << 30) / per_lane;
    if ((size_t)blocks * 256 > max_lanes) blocks = (int)std::max<size_t>(1, max_lanes / 256);
    const int n_lanes = blocks * 256;
    uint8_t *pool = wk->ws_get<uint8_t>("pool", (size_t)n_lanes * pool_cap * (wide ? sizeof(Entry) : 16));
    uint32_t *heads = wide ? wk->ws_get<uint32_t>("heads", (size_t)n_lanes * PS_MAX_BUCKETS) : nullptr;
    uint32_t *queue = wk->ws_get<uint32_t>("queue", 16);
    PS_HIP(hipMemsetAsync(queue, 0, 64, s));
    BtArgs a; std::memset(&a, 0, sizeof a);
    a.ix = ctx->ix.view; a.md = md; a.n_reads = n; a.len = len; a.lens = d_lens; a.n_lanes = n_lanes;
    if (d_lens) {                                               // ragged launch: every read's own budget, by its length
        uint8_t *tab = wk->pin_get<uint8_t>("units_by_len_h", 256);
        for (int l2 = 0; l2 < 256; ++l2) { const int u = budget_diffs(ctx->opt, l2) * (ctx->opt.profile ? ctx->opt.unit : 1); tab[l2] = (uint8_t)(u > 255 ? 255 : u); }
        uint8_t *d_tab = wk->ws_get<uint8_t>("units_by_len", 256);
        PS_HIP(hipMemcpyAsync(d_tab, tab, 256, hipMemcpyHostToDevice, s));
        a.units_by_len = d_tab;
    }
    a.bases = d_bases; a.nmask = d_nmask; a.n_bw = (len + 15) / 16; a.n_mw = (len + 31) / 32;
    a.w = w; a.cwb = cwb; a.cswb = cswb;
    a.alns = alns; a.aln_cap = aln_cap; a.n_aln = n_aln; a.status = status;
    a.pool = pool; a.pool_cap = pool_cap; a.heads = heads; a.wide = wide ? 1 : 0; a.stats = b.d_stats.p + 1;
    a.queue = queue; a.fetch_min = ctx->fetch_min; a.hit_min = ctx->hit_min;
    a.order = d_order; a.est = d_est; a.est_ab = d_est_ab;                   // all null in a wide launch
    // the estimate also spares the search entries (ps_narrow.h, nt_tail): first tier and profile costs only (units == score); a read it fails on starts over without it inside the launch
    a.cap_est = (first_tier && !wide && d_est && md.profile && !(std::getenv("PS_CAP") && std::atoi(std::getenv("PS_CAP")) == 0)) ? 1 : 0;
    if (a.cap_est) if (const char *e = std::getenv("PS_CAP_BIAS")) a.cap_est += std::max(0, std::min(200, std::atoi(e)));      // tests: estimates too low by that much, so that the restart path runs
    if (const char *e = std::getenv("PS_FETCH_MIN")) a.fetch_min = std::max(1, std::atoi(e));       // tuning: read at every launch
    if (const char *e = std::getenv("PS_HIT_MIN")) a.hit_min = std::max(1, std::atoi(e));
    if (!wide && pool_cap < 65535 && ctx->n_big > 0) {         // large slots for the reads that outgrow their private slice
        a.big_cap = 65535; a.n_big = (uint32_t)std::min<int64_t>(ctx->n_big, std::max(64, n));
        a.big_pool = wk->ws_get<uint8_t>("big_pool", (size_t)a.n_big * a.big_cap * 16);
        a.big_next = queue + 4;                                  // second counter in the zeroed queue words
        a.big_busy = wk->ws_get<uint32_t>("big_busy", a.n_big);
        PS_HIP(hipMemsetAsync(a.big_busy, 0, (size_t)a.n_big * 4, s));
    }
    uint32_t *riters = nullptr;
    if (ctx->want_read_iters) { riters = wk->ws_get<uint32_t>("riters", (size_t)n * PS_RI_WORDS); PS_HIP(hipMemsetAsync(riters, 0, (size_t)n * PS_RI_WORDS * 4, s)); a.read_iters = riters; }
    { EvTimer t(s);
      if (!launch_backtrack(a, wk->ws_get<BtArgs>("btargs", 1), wk->pin_get<BtArgs>("btargs_h", 1), blocks, lm, s, ctx->want_kstats || ctx->want_read_iters)) throw Error("cost model outside the ranges the search kernel packs (gap/score fields must fit a byte)");
      PS_HIP(hipGetLastError());
      const double ms = t.stop(); b.tm.ms_backtrack += ms; ++b.tm.n_backtrack_launches;
      b.tm.ms_width += t_width->read();
      if (t_order) b.tm.ms_width += t_order->read();                    // reported with the width stage: both prepare the search
      { double t0_ = 0, t1_ = 0; t.span(ctx->ref_event, t0_, t1_); if (b.tm.n_backtrack_launches == 1) b.tm.bt_begin_ms = t0_; b.tm.bt_end_ms = t1_; }
      if (std::getenv("PS_VERBOSE")) std::fprintf(stderr, "[parasuite-hip]   backtrack launch: %d reads x %d bp, stack %u%s, %d lanes, %.1f ms\n", n, len, pool_cap, wide ? " (wide)" : "", n_lanes, ms); }
    if (ctx->want_read_iters) { ctx->read_iters.resize((size_t)n * PS_RI_WORDS); PS_HIP(hipMemcpyAsync(ctx->read_iters.data(), riters, (size_t)n * PS_RI_WORDS * 4, hipMemcpyDeviceToHost, s)); PS_HIP(hipStreamSynchronize(s)); }
}

// ------------------------------------------------------------- host helpers ------
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

// ------------------------------------------------- samse stage on the device --------
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

// The big allocations of a lane of work (tier-1 stack slices, the large stack slots) made ahead of its first search: a
// hipMalloc of tens of GB synchronises the device, so when a second worker makes its own while the first worker's search kernel
// runs it waits for that kernel (seen as a 1-2 s stall of a piece).  ps_map calls this when a worker starts, before any search.
void reserve_search_workspace(Ctx *ctx, int work_index)
{
    require_device(ctx->device);
    Work *wk = ctx->work_at(work_index);
    int dev_cus = 256;
    { hipDeviceProp_t p; if (hipGetDeviceProperties(&p, ctx->device) == hipSuccess && p.multiProcessorCount > 0) dev_cus = p.multiProcessorCount; }
    const uint32_t pool_cap = ctx->pool_cap[0];
    if (pool_cap > 65535) return;                             // first tier is the wide one: sized by the launch
    int blocks = ctx->bt_blocks > 0 ? ctx->bt_blocks : dev_cus * 4;
    const size_t per_lane = (size_t)pool_cap * 16, max_lanes = ((size_t)64 << 30) / per_lane;
    if ((size_t)blocks * 256 > max_lanes) blocks = (int)std::max<size_t>(1, max_lanes / 256);
    (void)wk->ws_get<uint8_t>("pool", (size_t)blocks * 256 * per_lane);
    if (pool_cap < 65535 && ctx->n_big > 0) {
        (void)wk->ws_get<uint8_t>("big_pool", (size_t)ctx->n_big * 65535 * 16);
        (void)wk->ws_get<uint32_t>("big_busy", (size_t)ctx->n_big);
    }
}

// --------------------------------------------------------------- search stage -------
void batch_search(Batch &b)
{
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    require_device(ctx->device);
    b.tm = Timing();
    auto t0 = Clock::now();
    const int64_t N = b.rs.n;
    b.d_stats.zero(s);
    for (int t = 0; t < 3; ++t) b.n_overflow[t] = 0;
    if (b.d_class.n < (size_t)N) b.d_class.alloc((size_t)N);
    for (Bin &bin : b.bins) {
        const int n = (int)bin.ids.size();
        bin.host_alns_valid = false;
        const int cap1 = (bin.len <= 40 && ctx->aln_cap_short > ctx->aln_cap[0]) ? ctx->aln_cap_short : ctx->aln_cap[0];
        if (bin.d_alns.n < (size_t)n * cap1 || bin.aln_cap != cap1) { bin.d_alns.alloc((size_t)n * cap1); bin.d_n_aln.alloc(n); bin.d_status.alloc(n); }
        bin.aln_cap = cap1;
        run_search(b, bin.md, n, bin.bases.p, bin.nmask.p, bin.ragged ? bin.d_lens.p : nullptr, ctx->pool_cap[0], bin.aln_cap, bin.d_alns.p, bin.d_n_aln.p, bin.d_status.p, true);
        uint8_t *h_status = wk->pin_get<uint8_t>("status", n);
        PS_HIP(hipMemcpyAsync(h_status, bin.d_status.p, (size_t)n, hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(k_classify, dim3(std::min((n + 255) / 256, 4096)), dim3(256), 0, s, bin.d_alns.p, bin.aln_cap, bin.d_n_aln.p, bin.d_status.p,
                           bin.d_ids.p, n, ctx->opt.n_occ, b.d_class.p);
        PS_HIP(hipStreamSynchronize(s));
        bin.overflow.clear();
        std::vector<int32_t> todo;
        for (int r = 0; r < n; ++r) {
            if (h_status[r] == RS_OK) continue;
            if (h_status[r] == RS_BAD_SCORE) throw Error("internal: score outside the bucket range");
            todo.push_back(r);
        }
        // reads that need a deeper stack / a longer hit list: the second narrow tier, then the wide one.  A read whose stack outgrew
        // 65,535 entries already (RS_OVERFLOW_DEEP: on a large slot of the first launch) skips the second tier, which has no more than
        // that: on a repeat-rich genome those are the longest searches of the batch, and every tier starts them from scratch
        std::vector<int32_t> deep;
        { std::vector<int32_t> keep; for (int32_t r : todo) (h_status[r] == RS_OVERFLOW_DEEP ? deep : keep).push_back(r); todo.swap(keep); }
        for (int tier = 1; tier < 3; ++tier) {
            if (tier == 2) { todo.insert(todo.end(), deep.begin(), deep.end()); std::sort(todo.begin(), todo.end()); deep.clear(); }
            if (todo.empty()) continue;
            b.n_overflow[tier] += (int64_t)todo.size();
            const int m = (int)todo.size();
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
            run_search(b, bin.md, m, db.p, dm.p, bin.ragged ? dl.p : nullptr, ctx->pool_cap[tier], ctx->aln_cap[tier], ta.p, tn.p, ts.p);
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
    }
    KStats hs[3];
    b.d_stats.download(hs, 3, s);
    // classes to the host; the host-finished subset and its position in the tie-break stream
    auto tcl = Clock::now();
    b.h_class = (uint8_t *)b.p_class.get((size_t)N + 64);
    PS_HIP(hipMemcpyAsync(b.h_class, b.d_class.p, (size_t)N, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    b.st_width = hs[0]; b.st_backtrack = hs[1];
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
    {
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
        // hit lists of the subset: gathered on the device in subset order, one pinned download per bin
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
    b.tm.ms_classify = ms_since(tcl);
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
    auto t0 = Clock::now();
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
    auto t0 = Clock::now();
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
                    if (tot >= 0 && tot <= n_occ + 1)
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
    EvTimer t(s); launch_refine(ra, blocks, s); PS_HIP(hipGetLastError()); t.mark();
    cig.resize((size_t)n_it * PS_MAX_CIGAR); nc.resize(n_it);
    PS_HIP(hipMemcpyAsync(cig.data(), d_cig, cig.size() * 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(nc.data(), d_nc, (size_t)n_it * 4, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    b.tm.ms_refine += t.read();
}

void batch_locate(Batch &b)
{
    if (!b.selected) throw Error("locate before select");
    Ctx *ctx = b.ctx; Work *wk = b.wk; hipStream_t s = wk->stream;
    require_device(ctx->device);
    const int64_t N = b.rs.n, l_pac = ctx->ix.ref.l_pac;
    auto t0 = Clock::now();
    // ---- device-finished reads: SA walk, strand / MAPQ, queue of gapped hits ----
    // (the SA walk, k_post and the downloads go to the stream back to back; the walk's time is read after the one wait behind them)
    EvTimer t_sa(s); launch_sa2pos(ctx->ix.view, b.d_rows.p, b.d_pos.p, (int)N, b.d_stats.p + 2, s); PS_HIP(hipGetLastError()); t_sa.mark();
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
    b.tm.ms_sa2pos += t_sa.read();
    PS_HIP(hipMemcpy(&b.st_sa2pos, b.d_stats.p + 2, sizeof(KStats), hipMemcpyDeviceToHost));
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
            const int n_c = fix_cigar(c, nc[q], rb);
            if (n_c > PS_HIT_CIGAR) throw Error("CIGAR with more than 8 operations (raise PS_HIT_CIGAR for max_gapo > 2)");
            DevCigar dc; dc.g = g; dc.n = n_c; std::memcpy(dc.c, c, sizeof dc.c);
            b.dev_cigars.push_back(dc);
            b.h_fin[g].pos = rb;
            if (n_c == 0) b.h_fin[g].type = 0;
        }
    }
    std::sort(b.dev_cigars.begin(), b.dev_cigars.end(), [](const DevCigar &x, const DevCigar &y) { return x.g < y.g; });
    auto t1 = Clock::now();
    // ---- host-finished subset: its rows (main + alternatives) through the same SA kernel, then strand / MAPQ / DP ----
    const size_t M = b.sub.size(), n_rows = M + b.multis.size();
    if (n_rows) {
        std::vector<bwtint> rows(n_rows), pos(n_rows);
        par_for(M, ctx->host_threads, [&](size_t q0, size_t q1, int) { for (size_t q = q0; q < q1; ++q) rows[q] = b.sub[q].hit.type != 0 ? b.sub[q].hit.sa : 0; });
        par_for(b.multis.size(), ctx->host_threads, [&](size_t j0, size_t j1, int) { for (size_t j = j0; j < j1; ++j) rows[M + j] = b.multis[j].row; });
        bwtint *d_r = wk->ws_get<bwtint>("sub_rows", n_rows), *d_p = wk->ws_get<bwtint>("sub_pos", n_rows);
        PS_HIP(hipMemcpyAsync(d_r, rows.data(), n_rows * sizeof(bwtint), hipMemcpyHostToDevice, s));
        { EvTimer t(s); launch_sa2pos(ctx->ix.view, d_r, d_p, (int)n_rows, nullptr, s); PS_HIP(hipGetLastError()); b.tm.ms_sa2pos += t.stop(); }
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
                    h.n_cigar = fix_cigar(c, nc[q], rb);
                    if (h.n_cigar > PS_HIT_CIGAR) throw Error("CIGAR with more than 8 operations (raise PS_HIT_CIGAR for max_gapo > 2)");
                    std::memcpy(h.cigar, c, sizeof h.cigar);
                    h.pos = rb;
                    if (h.n_cigar == 0) h.type = 0;
                } else {
                    Multi &m = b.multis[h.multi_begin + bk.multi];
                    int64_t rb = m.pos;
                    m.n_cigar = fix_cigar(c, nc[q], rb);
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
