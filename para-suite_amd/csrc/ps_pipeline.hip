// ps_pipeline.hip -- host orchestration of one mapping job: the context, the cache of page-locked buffers, batch set-up.
//
// Replaces what the reference runs as two child processes,
//   bwa parasuite|aln ... -f P.sai     PARAsuiteMapping.java:63-77 / BWAMapping.java:51-61
//   bwa samse ref P.sai fq -f P.sam    PARAsuiteMapping.java:85-92 / BWAMapping.java:68-75
// by one pass: reads binned by length and 2-bit packed in HBM (here) -> width kernel -> backtracking kernel (ps_search.hip)
// -> tie-break selection (one drand48 stream in input order) -> SA-walk kernel -> banded-DP kernel for gapped hits
// (ps_samse.hip) -> SAM text (ps_records.hip).
// No stage has a CPU implementation of the kernels' work: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <thread>
#include "ps_pipeline.h"
#include "ps_par.h"

namespace ps {

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
    // tuning knobs of the context's lifetime (a search's own: ps_search_plan.h)
    env_int("PS_FETCH_MIN", fetch_min); env_int("PS_HIT_MIN", hit_min); env_int("PS_N_BIG", n_big); env_int("PS_BT_BLOCKS", bt_blocks);
    if (std::getenv("PS_READ_ITERS")) want_read_iters = true;
    if (std::getenv("PS_KSTATS")) want_kstats = true;
    int v = 0;
    if (env_int("PS_POOL_CAP", v)) pool_cap[0] = (uint32_t)v;
    if (env_int("PS_ALN_CAP", v)) { aln_cap[0] = std::max(1, v); aln_cap_short = 0; }   // hit intervals a read may list in the first tier (stated: for every length)
}
void Ctx::attach_device()
{
    require_device(device);
    if (stream) return;
    PS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    PS_HIP(hipEventCreate(&ref_event)); PS_HIP(hipEventRecord(ref_event, stream)); PS_HIP(hipEventSynchronize(ref_event));
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) cus = n_cu;
}
void Ctx::set_stock(const char *n_arg)
{
    Options o; set_stock_n(o, n_arg);
    if (o.max_diff < 0 && !(o.fnr > 0.0)) throw Error("bad -n argument");
    std::string err;
    if (!set_cost(o, err)) throw Error(err);
}
void Ctx::set_profile(const char *ep, const char *ip, const char *x_arg)
{
    double P[16], ins, del; std::string err;
    if (!read_profile_files(ep, ip, P, ins, del, err)) throw Error(err);
    set_profile_matrix(P, ins, del, x_arg ? std::atoi(x_arg) : -1);
}
void Ctx::set_profile_matrix(const double P[16], double ins, double del, int x)
{
    Options o; profile_costs(o, P, ins, del, x);
    std::string err;
    if (!set_cost(o, err)) throw Error(err);
}
void Ctx::set_search(const ps_search_opts *in)
{
    std::string err;
    if (!ps::set_search(*this, in, err)) throw Error(err);
}
Ctx::~Ctx() { if (ref_event) (void)hipEventDestroy(ref_event); if (stream) (void)hipStreamDestroy(stream); }
void ctx_release_device(Ctx &c)
{
    require_device(c.device);
    {
        std::lock_guard<std::mutex> l(c.work_mu);
        for (auto &w : c.work) w.reset();
        c.rec_tables.reset();
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
        bin.bases.release(); bin.nmask.release(); bin.d_lens.release(); bin.d_ids.release();
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

}  // namespace ps
