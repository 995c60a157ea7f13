// ps_map.hip -- the whole `map` step behind one call: the streaming pass, its outputs, and ps_map_route's sequence of passes.
//
// Stages run side by side on pieces of the input (whole records; the file is streamed, a window at a time): a parser thread
// (parse, bin, 2-bit pack), GPU workers (upload, search, samse stage) and a writer thread that hands every piece, in input order,
// to the outputs of the pass (SAM text, BAM records, the error profile, the route's own consumers).
// Devices: the first PARASUITE_GPUS devices (default 1), or the list in PARASUITE_GPU_IDS.  Every device holds ONE copy of
// the index: the first loads the files, the others receive the three blobs from it over xGMI (hipMemcpyPeerAsync).  Every
// device has PS_WORKERS_PER_GPU workers (default 1; 2 is allowed, and a device named twice in PARASUITE_GPU_IDS gets two), each
// with its own stream and workspace.  Two workers on one device were measured SLOWER end to end (4.6 s against 4.2 s for
// 10 M reads): two persistent search kernels share the CUs evenly instead of one refilling the other's tail, the later
// stages of one piece starve under the other's kernel, and the second 69 GB workspace costs its allocation.  The piece size
// follows from the input (ps_map_plan.h); PS_CHUNK_MB states a fixed size.
// Pieces go to whichever worker is free; the one sequential thing, the tie-break stream, is handed from piece to piece in
// input order (only the reads whose draw count is data dependent sit on that chain), so the SAM does not depend on the cut,
// on the number of workers or on the number of devices.  A finished piece gives its device memory back at once and at most
// a few finished pieces wait for the writer: memory does not grow with the input.
#include <hip/hip_runtime.h>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "ps_inflate.h"
#include "ps_map.h"
#include "ps_map_plan.h"
#include "ps_resident.h"
#include "ps_search_opts.h"
#include "ps_dev.h"

namespace ps {
namespace {

typedef std::chrono::steady_clock clk;
double secs_since(clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); }
struct Charge { double &to; const clk::time_point t0 = clk::now(); ~Charge() { to += secs_since(t0); } };   // the time of a scope, added to a counter

// Written pieces of ps_map are freed by threads of their own (gigabytes of host memory per piece: 0.18 s for 7.7 M reads), and the call
// does not wait for the last of them: they are joined by the next call, by ps_release_host_cache and when the process exits.
struct Trash { std::mutex mu; std::vector<std::thread> th; bool hooked = false; };
Trash &trash() { static Trash *t = new Trash(); return *t; }       // never destroyed: a thread may still run at exit

// ---- what a pass produces ---------------------------------------------------------------------------------------------------
// The writer hands every located piece, in input order, to each output of the pass in the order of its list (records, then
// the profile, then the route's consumer), then lets the piece go.  All calls come from the writer's thread, which also destroys
// the outputs when it is done or has failed: before the contexts of the pass (and their devices' memory) go.
struct PassOut {
    bool holds_device = false;             // works on the device until finish(): the contexts cannot give their memory back before
    virtual ~PassOut() {}
    virtual void start() {}                // before the first piece, while the writer has nothing to do
    virtual void piece(Batch &b) = 0;
    virtual void empty(const Ctx &) {}     // an input with no reads, instead of any piece(); the context is the first device's, its index resident
    virtual void finish() {}
};

struct SamText : PassOut {
    const char *const path; const int nthr; double &busy; bool first = true; SamScratch scratch;
    SamText(const char *p, int n, double &t) : path(p), nthr(n), busy(t) {}
    void start() override { const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644); if (fd >= 0) ::close(fd); }    // an output file that exists is emptied now: giving back 2 GB of cached pages takes 0.3 s
    void piece(Batch &b) override { Charge c{busy}; batch_write_sam(b, path, first, PS_PG_LINE, nthr, !first, &scratch); first = false; }
    void empty(const Ctx &c) override { write_text_file(path, sam_header(c.ix.ref, PS_PG_LINE)); }   // the header alone, as upstream's samse prints it before its read loop
};

// ps_map_to_bam: records go out as BAM, no SAM text at all.  by_name, keep (ps_map_route): sorted by read name; the sorted records also stay in memory
struct BamOut { int min_mapq = 0; bool sort = false, index = false; int level = 1; BamStats *stats = nullptr; bool by_name = false; BamFile *keep = nullptr; };
struct BamRecords : PassOut {
    const BamOut o; const char *const path; const int nthr; double &busy; std::unique_ptr<BamSink> sink;
    BamRecords(const BamOut &bo, const char *p, int n, double &t) : o(bo), path(p), nthr(n), busy(t) {}
    BamSink &sink_for(const Ctx &c)
    {
        if (!sink) {
            std::vector<std::pair<std::string, uint32_t>> refs;
            for (const Contig &ct : c.ix.ref.contigs) refs.emplace_back(ct.name, (uint32_t)ct.len);
            sink.reset(new BamSink(sam_header(c.ix.ref, PS_PG_LINE), refs, path, o.sort, o.index, nthr, o.level, o.by_name));
        }
        return *sink;
    }
    void piece(Batch &b) override
    {
        Charge c{busy};
        BamSink &s = sink_for(*b.ctx);
        if (b.dev_records && b.dev_records_mapq == o.min_mapq) {      // built on the device by the piece's worker (ps_bamrec.hip)
            DevRecords &r = *b.dev_records;
            s.add((const char *)r.bytes, r.n_bytes, r.recs, (uint64_t)b.rs.n);
            b.dev_records.reset();
            return;
        }
        std::vector<std::string> enc; std::vector<std::vector<BamRec>> recs;
        batch_bam_records(b, o.min_mapq, nthr, enc, recs);
        s.add(enc, recs, (uint64_t)b.rs.n);
    }
    void empty(const Ctx &c) override { sink_for(c); }       // the header-only BAM is written by finish()
    void finish() override { Charge c{busy}; sink->finish(o.stats, o.keep); sink.reset(); }
};

// ps_map_profiled: the pass also counts its error profile -- the same records, straight from memory, into the profile histograms
struct ProfileOut : PassOut {
    const int min_mapq, max_len; const std::string prefix; const int nthr; double &busy; std::unique_ptr<ProfileAccum> accum;
    ProfileOut(int q, int len, const std::string &pre, int n, double &t) : min_mapq(q), max_len(len), prefix(pre), nthr(n), busy(t) { holds_device = true; }
    void piece(Batch &b) override
    {
        Charge c{busy};
        if (!accum) accum.reset(new ProfileAccum(b.ctx->device, b.ctx->ix, max_len));     // on the device of the first piece, whose index stays resident until the writer is done
        ProfRecords pr;
        batch_profile_records(b, min_mapq, nthr, pr);
        accum->add(pr);
    }
    void finish() override
    {
        ProfileCounts pc;
        if (accum) accum->finish(pc);
        else { pc.max_len = max_len; pc.conv.assign((size_t)max_len * 16, 0); pc.ins.assign((size_t)max_len, 0); pc.del.assign((size_t)max_len, 0); }
        error_profile_write(pc, prefix);
        accum.reset();
    }
};

struct PieceFn : PassOut {                 // ps_map_route: what the call keeps of a piece for its next pass
    const std::function<void(Batch &)> fn;
    explicit PieceFn(std::function<void(Batch &)> f) : fn(std::move(f)) {}
    void piece(Batch &b) override { fn(b); }
};

// ---- the pass ---------------------------------------------------------------------------------------------------------------
// The contexts of a pass, one per device, each with its index, jump table and lanes of work.  A pass owns the set it makes; a
// set handed in (MapJob::resident) belongs to the caller and outlives the pass.
struct CtxSet { std::vector<std::unique_ptr<Ctx>> xs; bool loaded = false; int n_index_loads = 0; };
struct MapJob {
    MapArgs a;
    std::vector<ReadSet> *reads = nullptr; // the input, already parsed, instead of the file a.reads (consumed)
    bool bam_out = false;                  // the piece plan's: the records are compressed, which wants early pieces
    bool records_out = false; int records_mapq = 0;   // the pass has a BamRecords output, with this MAPQ filter (the device route of the records builds for it)
    std::vector<std::unique_ptr<PassOut>> outs;
    CtxSet *resident = nullptr;            // ps_map_route, the resident scope: the contexts are taken from there (made and loaded by the first pass that finds none) and left open
    std::vector<CtxSet *> lanes_from;      // the lanes of work (streams, search workspace) of these contexts, which search no more, move to this pass's contexts on the same devices
    int64_t n_reads = 0; double s_parse = 0, s_index = 0, s_write = 0, s_profile = 0;      // results
};

struct Piece { int64_t seq = 0; std::unique_ptr<Batch> b; };

struct Pass {
    explicit Pass(MapJob &j);              // plans, makes the contexts and sets their options: no thread yet, no device call
    void run();
    MapJob &job;
    const bool verbose = std::getenv("PS_VERBOSE") != nullptr;
    const clk::time_point t_begin = clk::now();
    const int nthr;
    DevicePlan dev; PiecePlan cut; int G = 0, n_workers = 0;
    // What becomes of the contexts at the end, one rule: resident ones are left open; a clean pass with no output that holds the
    // device releases the devices' memory while the writer formats the last piece and closes the rest on a trash thread; every
    // other pass closes them on the spot.
    CtxSet own, &set; const bool preloaded; bool holds_device = false;
    Ctx &ctx(int g) { return *set.xs[(size_t)g]; }
    Chan<Piece> parsed;
    std::mutex mu; std::condition_variable cv;       // guards: failure, the tie-break chain, the finished pieces, index hand-out
    struct Guarded {
        bool failed = false; std::string msg;
        int64_t next_select = 0; uint64_t draws = 0;                 // the tie-break chain
        std::map<int64_t, std::unique_ptr<Batch>> done; int64_t write_next = 0; int workers_left = 0;    // finished pieces waiting for the writer
        std::vector<int> index_state;      // per device: 0 not there, 1 resident
        std::vector<int> attached;         // per device: the device side of the context exists (made by the device's first worker)
        int64_t n_reads = 0, n_pieces = 0;
    } gd;
    size_t done_cap = 0;                   // finished pieces that may wait for the writer
    double t_parse = 0, t_release = 0, t_index = 0, t_index_all = 0; std::vector<double> t_gpu;
    double since() const { return secs_since(t_begin); }
    template <class F> bool wait_for(std::unique_lock<std::mutex> &l, F ready) { cv.wait(l, [&] { return gd.failed || ready(); }); return !gd.failed; }
    void fail_all(const std::string &m) { { std::lock_guard<std::mutex> l(mu); if (!gd.failed) { gd.failed = true; gd.msg = m; } } cv.notify_all(); parsed.abort(); }
    void parse();
    void write();
    void work(int g, int j, int slot);
};

int env_mb(const char *name) { const char *e = std::getenv(name); return e ? std::max(1, std::atoi(e)) : 0; }

// the devices and workers of a pass, from the environment (also a part of the resident scope's key)
DevicePlan devices_from_env()
{
    int per_dev = 1, want = 1, have = 1;
    if (const char *e = std::getenv("PS_WORKERS_PER_GPU")) per_dev = std::atoi(e);
    if (const char *e = std::getenv("PARASUITE_GPUS")) want = std::max(1, std::atoi(e));
    const char *ids = std::getenv("PARASUITE_GPU_IDS");
    if (!ids && want > 1 && (hipGetDeviceCount(&have) != hipSuccess || have < 1)) throw Error("no HIP device available");   // one device: found out (loudly) when the worker attaches it
    return plan_devices(ids, want, per_dev, have, (int)Ctx::N_WORK);
}
// the lanes of work that `from` holds go to the contexts of `to` on the same devices, where those have none
void move_lanes(CtxSet &from, CtxSet &to)
{
    for (auto &t : to.xs) for (auto &f : from.xs) {
        if (!t || !f || t.get() == f.get() || f->device != t->device) continue;
        std::lock_guard<std::mutex> l1(f->work_mu), l2(t->work_mu);
        for (int w = 0; w < (int)Ctx::N_WORK; ++w) if (f->work[w] && !t->work[w]) t->work[w] = std::move(f->work[w]);
    }
}

Pass::Pass(MapJob &j) : job(j), nthr(j.a.threads > 0 ? j.a.threads : 1), set(j.resident ? *j.resident : own), preloaded(j.resident && j.resident->loaded)
{
    dev = devices_from_env();
    G = (int)dev.devs.size(); n_workers = dev.n_workers();
    struct stat st;
    const size_t file_bytes = !job.reads && ::stat(job.a.reads, &st) == 0 && st.st_size > 0 && !is_gzip_file(job.a.reads) ? (size_t)st.st_size : 0;   // compressed: the text's size is unknown
    cut = plan_pieces(file_bytes, n_workers, job.bam_out, env_mb("PS_CHUNK_MB"), env_mb("PS_HUNGRY_MIN_MB"), env_mb("PS_FIRST_MB"));
    parsed.cap = (size_t)std::max(2, n_workers);
    done_cap = (size_t)n_workers + 2;
    gd.workers_left = n_workers; gd.index_state.assign((size_t)G, preloaded ? 1 : 0); gd.attached.assign((size_t)G, 0);
    t_gpu.assign((size_t)n_workers, 0.0);
    for (const auto &o : job.outs) holds_device = holds_device || o->holds_device;
    // the contexts (options) exist before any index is loaded: the parser stage needs the cost model to bin and pack the reads,
    // not the index; the device side is attached by the device's first worker, beside the parser
    if (set.xs.empty()) set.xs.resize((size_t)G);
    if (set.xs.size() != (size_t)G) throw Error("internal: the resident contexts do not match the devices");
    for (int g = 0; g < G; ++g) {
        if (!set.xs[g]) set.xs[g].reset(new Ctx(dev.devs[g]));
        ctx(g).set_options(job.a.mm, job.a.error_profile, job.a.indel_profile);
        ctx(g).set_search(job.a.search);                   // after the cost part: checked under it.  Every device's context, so every worker
        ctx(g).host_threads = nthr;
        ctx(g).n_work = dev.workers[g];
    }
    for (CtxSet *from : job.lanes_from) if (from && from != &set) move_lanes(*from, set);
}

// the parser (starts at once)
void Pass::parse()
{
    try {
        int64_t seq = 0;
        int pthr = nthr;                                       // all of them: the GPU waits for the first piece, and sharing the cores with the writer later cost nothing measurable (2.78-2.90 -> 2.67-2.80 s per 10 M reads against half of them)
        if (const char *e = std::getenv("PS_PARSE_THREADS")) pthr = std::max(1, std::atoi(e));
        const std::function<void(ReadSet &&)> hand_over = [&](ReadSet &&rs) {
            Piece p; p.seq = seq++; p.b = batch_prepare(&ctx(0), std::move(rs), pthr);     // host only
            parsed.push(std::move(p));
        };
        if (job.reads) {                                       // parsed by an earlier pass: binned and packed again under this pass's cost model
            for (ReadSet &rs : *job.reads) if (rs.n) hand_over(std::move(rs));
            job.reads->clear();
        } else {
            const std::function<bool()> hungry = [&]() { return parsed.hungry(); };
            load_reads_chunked(job.a.reads, pthr, cut.chunk_bytes, hand_over, cut.first_bytes, &hungry, cut.hungry_min);
        }
        t_parse = since();
    } catch (const std::exception &e) { fail_all(e.what()); }
    parsed.close();
}

// the writer: pieces in input order
void Pass::write()
{
    struct Done { std::vector<std::unique_ptr<PassOut>> &outs; ~Done() { outs.clear(); } } done_with{job.outs};
    try {
        for (auto &o : job.outs) o->start();
        bool first = true;
        for (;;) {
            std::unique_ptr<Batch> b;
            {
                std::unique_lock<std::mutex> l(mu);
                if (!wait_for(l, [&] { return gd.done.count(gd.write_next) || (gd.workers_left == 0 && gd.done.empty()); })) return;
                auto it = gd.done.find(gd.write_next);
                if (it == gd.done.end()) break;                    // all workers finished and nothing is left
                b = std::move(it->second); gd.done.erase(it);
            }
            for (auto &o : job.outs) o->piece(*b);
            first = false;
            { std::lock_guard<std::mutex> l(mu); ++gd.write_next; }
            cv.notify_all();
            Charge c{t_release};
            Batch *q = b.release(); trash_add(std::thread([q]() { delete q; }));   // pinned record buffers, the reads (~40 ms per piece): released on a thread of its own, neither on the GPU worker's time nor on the writer's
        }
        if (first) {                       // no reads at all
            { std::unique_lock<std::mutex> l(mu); if (!wait_for(l, [&] { return gd.index_state[0] == 1; })) return; }
            for (auto &o : job.outs) o->empty(ctx(0));
        }
        for (auto &o : job.outs) o->finish();
    } catch (const std::exception &e) { fail_all(e.what()); }
}

// a worker: lane j of device g's context
void Pass::work(int g, int j, int slot)
{
    try {
        Ctx &c = ctx(g);
        if (j == 0) { c.attach_device(); { std::lock_guard<std::mutex> l(mu); gd.attached[g] = 1; } cv.notify_all(); }
        else { std::unique_lock<std::mutex> l(mu); if (!wait_for(l, [&] { return gd.attached[g] == 1; })) return; }
        require_device(c.device);
        // The worker's big allocations (69 GB of stack slices + the large slots) are made NOW, on a thread of their own, while the
        // index loads and the parser works on the first piece: a hipMalloc that is handed memory another call or process has
        // just freed waits for the driver to clear it (seconds for this size, tools/microbench_malloc) -- behind the index load
        // that wait is hidden, in front of the first search launch (where the first ws_get used to make it) it is not.  With
        // several workers on one device it also keeps a worker's allocation from waiting for another worker's running kernel.
        std::thread reserve([&c, j]() { try { reserve_search_workspace(&c, j); } catch (...) {} });
        struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } reserve_joiner{reserve};
        if (j == 0 && preloaded) { /* resident since an earlier pass of the call */ }
        else if (j == 0) {                                     // this device's index: from the files, or from the first device
            if (g == 0) { index_load(job.a.ref_fa, c.ix, c.stream); t_index = since(); ++set.n_index_loads; }
            else {
                { std::unique_lock<std::mutex> l(mu); if (!wait_for(l, [&] { return gd.index_state[0] == 1; })) return; }
                index_clone(ctx(0).ix, ctx(0).device, c.ix, c.device, c.stream);
            }
            { std::lock_guard<std::mutex> l(mu); gd.index_state[g] = 1; t_index_all = since(); }
            cv.notify_all();
        } else { std::unique_lock<std::mutex> l(mu); if (!wait_for(l, [&] { return gd.index_state[g] == 1; })) return; }
        if (reserve.joinable()) reserve.join();
        Piece p;
        while (parsed.pop(p)) {
            { std::lock_guard<std::mutex> l(mu); if (gd.failed) return; gd.n_reads += p.b->rs.n; ++gd.n_pieces; }
            const auto t0 = clk::now();
            Batch &b = *p.b;
            b.ctx = &c;                                        // the piece was packed with the (identical) options of context 0
            b.work_index = j;
            batch_upload(b);
            const double w_up = secs_since(t0);
            batch_search(b);
            const double w_search = secs_since(t0) - w_up;
            {                                                   // the tie-break stream: pieces take their turn in input order
                std::unique_lock<std::mutex> l(mu);
                if (!wait_for(l, [&] { return gd.next_select == p.seq; })) return;
                uint64_t after = 0;
                batch_select_hard(b, gd.draws, &after);
                gd.draws = after; ++gd.next_select;
            }
            cv.notify_all();
            batch_select_easy(b, nthr);
            batch_locate(b);
            if (job.records_out && bam_records_device_on()) {     // the BAM records while d_sel and d_fin are still in HBM; a HIP error fails the call
                b.dev_records.reset(new DevRecords());
                b.dev_records_mapq = job.records_mapq;
                batch_bam_records_device(b, job.records_mapq, nthr, *b.dev_records);
            }
            b.release_device();                               // what is left to do (SAM text) reads host memory only
            if (verbose) {
                const Timing &t = b.tm;
                std::fprintf(stderr, "[parasuite-hip]   piece %lld on device %d worker %d: %lld reads; upload %.0f ms, search stage %.0f ms wall (width %.0f backtrack %.0f classify %.0f), select %.0f+%.0f sa2pos %.0f refine %.0f host_post %.0f ms\n",
                             (long long)p.seq + 1, c.device, j, (long long)b.rs.n, 1e3 * w_up, 1e3 * w_search, t.ms_width, t.ms_backtrack, t.ms_classify, t.ms_sel_hard, t.ms_sel_easy, t.ms_sa2pos, t.ms_refine, t.ms_host_post);
            }
            t_gpu[slot] += secs_since(t0);
            {
                // at most done_cap finished pieces wait for the writer -- but the piece the writer wants next always gets in
                std::unique_lock<std::mutex> l(mu);
                if (!wait_for(l, [&] { return gd.done.size() < done_cap || p.seq == gd.write_next; })) return;
                gd.done[p.seq] = std::move(p.b);
            }
            cv.notify_all();
        }
    } catch (const std::exception &e) { fail_all(e.what()); }
}

void Pass::run()
{
    trash_collect();                                           // what an earlier call left to be freed
    std::thread parser(&Pass::parse, this), writer(&Pass::write, this);
    bool have_index = true;
    try {
        if (!index_files_exist(job.a.ref_fa)) {               // the Java probes <ref>.bwt and indexes first; be lenient if it did not
            ctx(0).attach_device();
            Index tmp; index_build(job.a.ref_fa, tmp, ctx(0).stream); index_save(tmp, job.a.ref_fa);
        }
    } catch (const std::exception &e) { have_index = false; fail_all(e.what()); }
    std::vector<std::thread> workers;
    auto worker = [this](int g, int j, int slot) { work(g, j, slot); { std::lock_guard<std::mutex> l(mu); --gd.workers_left; } cv.notify_all(); };
    if (have_index) { int slot = 0; for (int g = 0; g < G; ++g) for (int j = 0; j < dev.workers[g]; ++j) workers.emplace_back(worker, g, j, slot++); }
    else { std::lock_guard<std::mutex> l(mu); gd.workers_left = 0; }
    for (auto &t : workers) t.join();
    const double t_workers = since();
    cv.notify_all();
    parsed.abort();                                            // a parser still waiting to hand over a piece must not wait forever
    // The devices' memory (index, 69-GB workspaces: ~0.1 s of hipFree) goes back while the writer formats the last piece, which
    // reads host memory only; a pass with an output that holds the device (ProfileAccum counts on it until the writer is done) keeps it.
    const bool early = !holds_device && !job.resident;
    std::thread early_release;
    double t_release_dev = 0;
    if (early) early_release = std::thread([&]() { for (auto &c : set.xs) if (c) { try { ctx_release_device(*c); } catch (...) {} } t_release_dev = since(); });
    parser.join(); writer.join();
    const double t_written = since();
    if (early_release.joinable()) early_release.join();
    gd.done.clear();
    job.n_reads = gd.n_reads; job.s_parse = t_parse; job.s_index = t_index_all;
    // what is left of the contexts (streams, events, the mapped packed text: 0.05 s) goes the way of the written pieces when the
    // device memory has been given back already; a failed pass and one that held the device close them here
    if (job.resident) set.loaded = set.loaded || !gd.failed;
    else if (early && !gd.failed) trash_add(std::thread([gone = std::move(own.xs)]() mutable { gone.clear(); }));
    else own.xs.clear();
    const double t_closed = since();
    if (gd.failed) throw Error(gd.msg);
    if (!verbose) return;
    double busy = 0; for (double v : t_gpu) busy += v;
    std::fprintf(stderr, "[parasuite-hip] ps_map: %lld reads in %lld piece(s) of <= %.0f MB, %d device(s) x %d worker(s), %.3f s; index resident after %.3f s (all devices %.3f s), "
                         "parser done after %.3f s, GPU stages busy %.3f s (summed over workers) and done after %.3f s, SAM writer busy %.3f s (+ %.3f s handing pieces back, %.3f s error profile) and done after %.3f s, device memory released after %.3f s, contexts closed after %.3f s\n", (long long)gd.n_reads, (long long)gd.n_pieces, cut.chunk_bytes / 1048576.0,
                         G, dev.workers[0], since(), t_index, t_index_all, t_parse, busy, t_workers, job.s_write, t_release, job.s_profile, t_written, t_release_dev, t_closed);
}

// ---- the resident scope -------------------------------------------------------------------------------------------------------
// The entries (ps_resident.h) hold the CtxSet a pass takes as MapJob::resident.  Calls inside a scope take their turn (call_mu is
// held for the whole call); mu guards the books, so that ps_resident_info answers while a call runs.
typedef ResidentCache<CtxSet> Residents;
struct ResidentScope { std::mutex call_mu, mu; Residents cache; };
// Everything a set holds goes back before this returns, on the calling thread: device memory (blobs, jump table, the lanes'
// workspace), then streams, events and the mapped .pac.  The lanes of the devices an heir shares move to it first.
void close_set(CtxSet &gone, CtxSet *heir)
{
    trash_collect();
    if (heir) move_lanes(gone, *heir);
    for (auto &c : gone.xs) if (c && c->stream) { try { ctx_release_device(*c); } catch (...) {} }     // no stream: the device side was never attached
    gone.xs.clear(); gone.loaded = false;
}
ResidentScope &scope()                     // never destroyed: a process that exits inside a scope makes no device call from an exit handler
{
    static ResidentScope *s = [] { ResidentScope *x = new ResidentScope(); x->cache.close = close_set; return x; }();
    return *s;
}
ResidentKnobs knobs_from_env()
{
    ResidentKnobs k;
    const Ctx probe(0);                    // PS_POOL_CAP, PS_N_BIG, PS_BT_BLOCKS as a context of the pass reads them (no device call)
    k.pool_cap = (int)probe.pool_cap[0]; k.n_big = probe.n_big; k.bt_blocks = probe.bt_blocks;
    k.jump_levels = jump_levels_stated();  // as index_build_jump reads it
    if (const char *e = std::getenv("PS_JUMP")) k.jump = std::atoi(e) == 0 ? 0 : 1;     // as launch_backtrack reads it
    return k;
}
uint64_t index_blob_bytes(const CtxSet &s)
{
    uint64_t b = 0;
    for (const auto &c : s.xs) if (c) b += c->ix.blocks.n * sizeof(OccBlock) + c->ix.sa.n * sizeof(uint32_t) + c->ix.pac.n;
    return b;
}
// A mapping call's part in the scope.  Outside a scope it does nothing and holds nothing.  Inside, entry() looks a reference up
// (pinned for the call), lend() hands it to a pass, done() settles a call that ended well; a call that ends any other way drops
// every entry it used when this goes out of scope.
struct ResidentUse {
    ResidentScope &rs = scope();
    std::unique_lock<std::mutex> turn{rs.call_mu};
    bool on = false, settled = false;
    struct Used { Residents::Entry *e; int loads_before; };
    std::vector<Used> used;
    ResidentUse()
    {
        { std::lock_guard<std::mutex> l(rs.mu); on = rs.cache.active; if (on) ++rs.cache.n.n_calls; }
        if (!on) turn.unlock();
    }
    Residents::Entry *entry(const char *ref_fa)
    {
        const DevicePlan plan = devices_from_env();
        const ResidentKey key = resident_key(ref_fa, plan, knobs_from_env());
        const ResidentIdent id = resident_ident(ref_fa);
        std::lock_guard<std::mutex> l(rs.mu);
        Residents::Entry *e = rs.cache.acquire(key, id, [&plan](CtxSet &s) {         // the contexts exist at once, so that they can inherit lanes: options only, no device call
            s.xs.resize(plan.devs.size());
            for (size_t g = 0; g < plan.devs.size(); ++g) s.xs[g].reset(new Ctx(plan.devs[g]));
        });
        for (const Used &u : used) if (u.e == e) return e;
        used.push_back(Used{e, e->payload.n_index_loads});
        return e;
    }
    void lend(Residents::Entry *e, MapJob &job)
    {
        job.resident = &e->payload; job.lanes_from.clear();
        std::lock_guard<std::mutex> l(rs.mu);
        for (Residents::Entry *f : rs.cache.take_lanes(e)) job.lanes_from.push_back(&f->payload);
    }
    void settle(bool ok)
    {
        if (!on || settled) return;
        settled = true;
        std::lock_guard<std::mutex> l(rs.mu);
        for (const Used &u : used) {
            rs.cache.n.n_index_loads += (uint64_t)(u.e->payload.n_index_loads - u.loads_before);
            if (ok) {
                u.e->bytes = index_blob_bytes(u.e->payload);
                if (!u.e->id.complete()) u.e->id = resident_ident(u.e->key.path);      // the pass built the index files itself
                rs.cache.release(u.e);
            } else rs.cache.drop(u.e);
        }
    }
    void done() { settle(true); }
    ~ResidentUse() { settle(false); }
};
// one pass of a mapping call that is a single pass: inside a scope over the entry of its reference
void run_single(MapJob &job)
{
    ResidentUse use;
    if (use.on) use.lend(use.entry(job.a.ref_fa), job);
    Pass(job).run();
    use.done();
}

}  // namespace

void resident_begin(const ps_resident_opts *o)
{
    ps_resident_opts r; std::string err;
    if (!resident_opts_read(o, r, err)) throw Error(err);
    ResidentScope &s = scope();
    std::lock_guard<std::mutex> t(s.call_mu), l(s.mu);
    if (!s.cache.begin(r.max_references, err)) throw Error(err);
}
void resident_end()
{
    ResidentScope &s = scope();
    std::string err;
    std::lock_guard<std::mutex> t(s.call_mu), l(s.mu);
    const bool open = s.cache.active;
    if (open) trash_collect();             // what calls before the scope left to be freed: no thread of the library is left behind
    if (!s.cache.end(err)) throw Error(err);
}
void resident_info(ps_resident_stats &out)
{
    ResidentScope &s = scope();
    std::lock_guard<std::mutex> l(s.mu);
    const ResidentCounters &n = s.cache.n;
    std::memset(&out, 0, sizeof out);
    out.active = s.cache.active ? 1 : 0; out.n_references = (uint32_t)s.cache.entries.size();
    out.n_calls = n.n_calls; out.n_index_loads = n.n_index_loads; out.n_index_reuses = n.n_index_reuses; out.n_stale_reloads = n.n_stale_reloads;
    out.n_evictions = n.n_evictions; out.n_dropped_after_error = n.n_dropped_after_error; out.bytes_index_resident = s.cache.bytes();
}
void resident_invalidate(const char *ref_fa)
{
    ResidentScope &s = scope();
    { std::lock_guard<std::mutex> l(s.mu); if (!s.cache.active) return; }
    std::lock_guard<std::mutex> t(s.call_mu), l(s.mu);
    s.cache.invalidate(resident_path(ref_fa));
}

void trash_add(std::thread &&t) { Trash &x = trash(); std::lock_guard<std::mutex> l(x.mu); x.th.push_back(std::move(t)); if (!x.hooked) { x.hooked = true; std::atexit(trash_collect); } }
void trash_collect() { Trash &x = trash(); std::vector<std::thread> all; { std::lock_guard<std::mutex> l(x.mu); all.swap(x.th); } for (auto &t : all) if (t.joinable()) t.join(); }

void map_to_sam(const MapArgs &a, const char *out_sam)
{
    MapJob job; job.a = a;
    job.outs.emplace_back(new SamText(out_sam, a.threads > 0 ? a.threads : 1, job.s_write));
    run_single(job);
}
// ps_map + the error profile of its own alignments (those with MAPQ >= min_mapq: what the filtered BAM of the pass would
// hold), counted from the records in memory while the SAM is being written: <profile_prefix>.errorprofile / .indelprofile
void map_profiled(const MapArgs &a, const char *out_sam, int min_mapq, int max_read_len, const char *profile_prefix)
{
    const int nthr = a.threads > 0 ? a.threads : 1;
    MapJob job; job.a = a;
    job.outs.emplace_back(new SamText(out_sam, nthr, job.s_write));
    job.outs.emplace_back(new ProfileOut(min_mapq, max_read_len, profile_prefix, nthr, job.s_profile));
    run_single(job);
}
// ps_map with the records going straight into a BAM file: what PARAsuiteMapping.java:102-152 makes of <prefix>.sam with three
// samtools calls (view -bS, view -q, and -- Mapping.java:85-108 -- sort + index), without the 2 GB of SAM text in between.  Records
// with MAPQ < min_mapq are left out; sort_by_coordinate / write_index as in ps_sam_to_bam.  Unsorted output is compressed and written
// piece by piece while later pieces are searched.  zlib level 1 by default (the BAM is 10 % larger than at samtools' level 6 and the call
// 0.7 s shorter per 10 M reads: compression, not mapping, is what the host spends its time on); PS_BAM_LEVEL=6 for samtools' own.
void map_to_bam(const MapArgs &a, const char *out_bam, int min_mapq, bool sort_by_coordinate, bool write_index, BamStats *stats)
{
    BamOut bo; bo.min_mapq = min_mapq; bo.sort = sort_by_coordinate; bo.index = write_index; bo.stats = stats;
    if (const char *e = std::getenv("PS_BAM_LEVEL")) bo.level = std::atoi(e);
    MapJob job; job.a = a; job.bam_out = true; job.records_out = true; job.records_mapq = min_mapq;
    job.outs.emplace_back(new BamRecords(bo, out_bam, a.threads > 0 ? a.threads : 1, job.s_write));
    run_single(job);
}

// ---- the whole `map` mode (Main.java:249-420) in one call ---------------------------------------------------------------------
// The passes are the one above, over contexts that stay open from pass to pass: the genome's index is loaded once and keeps its lanes of
// work; the reads are parsed once and kept (up to PS_ROUTE_KEEP_MB of host memory) for the profile pass; the first pass's profile is
// counted from its records in memory (ps_map_profiled's path); the weak reads of the last genomic pass go to the transcript pass as a
// ReadSet, not as FASTQ text; the sorted records of the last genomic pass and of the transcript pass stay in memory for the lift.
namespace {
size_t readset_bytes(const ReadSet &rs)
{
    return rs.len.size() * 4 + rs.off.size() * 8 + rs.name_off.size() * 8 + rs.seq.size() + rs.qual.size() + rs.names.size();
}
// ExtractWeakMappingReads on a located piece: the reads whose record has MAPQ < threshold, as a second parse of their FASTQ text would return
// them (the read as it was sequenced is what the ReadSet holds; the parser takes one more trailing /1 or /2 off the name)
// fq (--unaligned): also the four FASTQ lines ps_extract_weak_reads writes for the record -- its name as the record carries it, the bases as
// BAM's nibbles give them back (A C G T N), the read as it was sequenced
void gather_weak(const Batch &b, int threshold, ReadSet &w, uint64_t &n_weak, std::string *fq)
{
    const ReadSet &rs = b.rs;
    if (w.off.empty()) { w.off.push_back(0); w.name_off.push_back(0); }
    for (int64_t g = 0; g < rs.n; ++g) {
        Hit h; b.hit_of(g, h);
        if ((h.type ? h.mapq : 0) >= threshold) continue;
        size_t nl; const char *nm = rs.name(g, nl);
        if (rs.len[g] == 0) throw Error("extract: record " + std::string(nm, nl) + " has MAPQ below " + std::to_string(threshold) + " and no SEQ ('*'): it cannot be mapped again");
        if (!rs.has_qual) throw Error("extract: record " + std::string(nm, nl) + " has MAPQ below " + std::to_string(threshold) + " and no QUAL ('*'): it cannot be written as FASTQ");
        if (fq) {
            const int64_t l = rs.off[g + 1] - rs.off[g];
            fq->push_back('@'); fq->append(nm, nl); fq->push_back('\n');
            for (int64_t i = 0; i < l; ++i) { const uint8_t c = rs.seq[(size_t)(rs.off[g] + i)]; fq->push_back("ACGTN"[c < 4 ? c : 4]); }
            fq->append("\n+\n"); fq->append(rs.qual.data() + rs.off[g], (size_t)l); fq->push_back('\n');
        }
        if (nl > 2 && nm[nl - 2] == '/' && (nm[nl - 1] == '1' || nm[nl - 1] == '2')) nl -= 2;
        w.names.insert(w.names.end(), nm, nm + nl); w.name_off.push_back((int64_t)w.names.size());
        w.seq.insert(w.seq.end(), rs.seq.data() + rs.off[g], rs.seq.data() + rs.off[g + 1]);
        w.qual.insert(w.qual.end(), rs.qual.data() + rs.off[g], rs.qual.data() + rs.off[g + 1]);
        w.len.push_back(rs.len[g]); w.off.push_back((int64_t)w.seq.size());
        ++w.n; ++n_weak;
    }
    w.has_qual = true;
}
bool has(const char *s) { return s && s[0]; }

// the call's state between its passes, and one pass of it
struct Route {
    const ps_route_opts2 &o; const int threads, gm; int bam_level = 1;
    const char *const ref_genome, *const ref_refine;     // the reference of the genomic passes; that of the refine pass where it is another one (by realpath), else null
    OutFiles &files; CtxSet genome, genome_refine, transcripts;    // the call's outputs (published step by step); its own contexts: open from pass to pass, closed when it returns
    ResidentUse use; Residents::Entry *ent[3] = {nullptr, nullptr, nullptr}; int loads0[3] = {0, 0, 0};    // inside a resident scope: the scope's entries instead, which stay
    std::vector<ReadSet> kept, weak; size_t kept_bytes = 0, keep_bound = (size_t)8192 << 20; bool kept_all = true;
    uint64_t n_weak = 0; std::string weak_fq;       // weak_fq: <P>.unaligned.fastq of a transcript route with keep_unaligned
    BamFile G, T;
    enum Ref { kGenome = 0, kRefine = 1, kTranscripts = 2 };
    Route(const ps_route_opts2 &opts, const char *rg, const char *rr, int thr, int mapq_genomic, OutFiles &outs) : o(opts), threads(thr), gm(mapq_genomic), ref_genome(rg), ref_refine(rr), files(outs)
    {
        if (const char *e = std::getenv("PS_ROUTE_KEEP_MB")) keep_bound = (size_t)std::max(0, std::atoi(e)) << 20;
        if (const char *e = std::getenv("PS_BAM_LEVEL")) bam_level = std::atoi(e);
    }
    void weak_of(Batch &b) { weak.emplace_back(); gather_weak(b, gm, weak.back(), n_weak, o.keep_unaligned ? &weak_fq : nullptr); }
    void keep(Batch &b)                    // the parsed piece stays for the profile pass, within the bound
    {
        if (!kept_all) return;
        const size_t bytes = readset_bytes(b.rs);
        if (kept_bytes + bytes > keep_bound) { kept_all = false; kept.clear(); kept.shrink_to_fit(); kept_bytes = 0; return; }
        kept_bytes += bytes; kept.push_back(std::move(b.rs));
    }
    // one pass: a sorted BAM (+ index, or by name) under its temporary name, published when the pass is done.  job: the input source,
    // the contexts and the outputs that follow the records
    void pass(MapJob &job, const char *mm, const char *ep, const char *ip, const char *ref, const std::string &out, int min_mapq, bool by_name, BamFile *keep_recs, ps_bam_stats &bs_out,
              bool publish = true)
    {
        BamStats bs; BamOut bo; bo.min_mapq = min_mapq; bo.sort = !by_name; bo.index = !by_name; bo.by_name = by_name; bo.keep = keep_recs; bo.stats = &bs; bo.level = bam_level;
        const std::string t = files.tmp(out);
        job.a = MapArgs{threads, mm, ep, ip, ref, o.reads_fq, o.search}; job.bam_out = true; job.records_out = true; job.records_mapq = min_mapq;
        job.outs.emplace(job.outs.begin(), new BamRecords(bo, t.c_str(), threads, job.s_write));
        Pass(job).run();
        if (publish) { files.publish(out); if (!by_name) files.publish(out + ".bai"); }
        bs_out.n_in = bs.n_in; bs_out.n_out = bs.n_out; bs_out.bam_bytes = bs.bam_bytes;
    }
    // the contexts of a pass; a later reference takes over the lanes of work of the passes before it
    const char *path_of(Ref w) const { return w == kTranscripts ? o.transcripts_fa : w == kRefine ? ref_refine : ref_genome; }
    CtxSet &own_set(Ref w) { return w == kTranscripts ? transcripts : w == kRefine ? genome_refine : genome; }
    void lend(MapJob &job, Ref w)
    {
        if (w == kRefine && !ref_refine) w = kGenome;
        if (!use.on) {
            job.resident = &own_set(w);
            if (w == kRefine) job.lanes_from = {&genome}; else if (w == kTranscripts) job.lanes_from = {&genome, &genome_refine};
            return;
        }
        if (!ent[w]) { ent[w] = use.entry(path_of(w)); loads0[w] = ent[w]->payload.n_index_loads; }
        use.lend(ent[w], job);
    }
    const CtxSet &set_of(Ref w) const { return ent[w] ? ent[w]->payload : const_cast<Route *>(this)->own_set(w); }
    int loads_of(Ref w) const { return set_of(w).n_index_loads - loads0[w]; }
    void close() { transcripts.xs.clear(); genome_refine.xs.clear(); genome.xs.clear(); }
};

// the caller's struct as this library's (ps_search_opts' rules): the fields behind struct_size keep their defaults, all zero here
void route_opts_read(const ps_route_opts2 *in, ps_route_opts2 &o)
{
    std::memset(&o, 0, sizeof o);
    if (!in) throw Error("ps_map_route_opts: no options");
    const size_t sz = in->struct_size, p0 = offsetof(ps_route_opts2, reads_fq), p1 = offsetof(ps_route_opts2, keep_unaligned);
    if (sz < sizeof(uint32_t) || sz % sizeof(int32_t) != 0 || sz > sizeof o || (sz > p0 && sz < p1 && (sz - p0) % sizeof(void *) != 0))
        throw Error("ps_map_route_opts: struct_size " + std::to_string(sz) + " must be a multiple of 4 from 4 to " + std::to_string(sizeof o) + " that does not end inside a pointer");
    std::memcpy(&o, in, sz);
    o.struct_size = (uint32_t)sizeof o;
}

void route_run(const ps_route_opts2 &o, const std::string &who, ps_route_stats *stats_out)
{
    if (!has(o.reads_fq)) throw Error(who + "the reads file (-q) is required");
    if (!has(o.ref_fa)) throw Error(who + "the reference (-r) is required");
    if (!has(o.out_prefix)) throw Error(who + "the output prefix (-o) is required");
    const bool refine = o.refine != 0, with_t = has(o.transcripts_fa), given = has(o.error_profile), keep_un = o.keep_unaligned != 0;
    if (given && !refine) throw Error(who + "an error profile without refine: nothing to map");
    if (has(o.indel_profile) && !given) throw Error(who + "an indel profile without an error profile");
    const int threads = o.threads > 0 ? o.threads : 1, max_len = o.max_read_len > 0 ? o.max_read_len : 101;
    const int gm = o.mapq_genomic > 0 ? o.mapq_genomic : 10, tm = o.mapq_transcript > 0 ? o.mapq_transcript : 1;
    const char *bwa_mm = has(o.bwa_mm) ? o.bwa_mm : "2", *para_mm = has(o.parasuite_mm) ? o.parasuite_mm : "-1";
    if (max_len > profile_max_len(0)) throw Error(who + "maximum read length out of range (1.." + std::to_string(profile_max_len(0)) + ")");
    const bool first_pass = !given;
    if (o.search) {                        // a stock pass runs iff there is a first pass, a profile pass iff refine
        std::string err;
        if ((first_pass && !search_opts_check(o.search, false, err)) || (refine && !search_opts_check(o.search, true, err))) throw Error(who + err);
    }
    // --ref-refine (Main.java:318): without refine it is never read.  With a given profile no pass maps against ref_fa at all
    const bool other_ref = refine && has(o.ref_refine) && resident_path(o.ref_refine) != resident_path(o.ref_fa);
    const char *const ref_genome = other_ref && !first_pass ? o.ref_refine : o.ref_fa;
    const char *const ref_refine = other_ref && first_pass ? o.ref_refine : nullptr;
    const char *const ref_last = ref_refine ? ref_refine : ref_genome;     // what the refine pass maps against
    const std::string P = o.out_prefix;
    const std::string f_bwa = P + ".BWA-genomic.bam", f_para = P + ".PARAsuite-genomic.bam", f_comb = P + ".combined.bam";
    const std::string f_tr = P + (refine ? ".PARAsuite-transcript.bam" : ".BWA-transcript.bam");
    const std::string f_ep = f_bwa + ".errorprofile", f_ip = f_bwa + ".indelprofile", f_un = P + ".unaligned.fastq";
    OutFiles files(".route-tmp");          // every output of the steps this call will run; ProfileOut writes <prefix>.errorprofile and .indelprofile
    const std::string profile_tmp = f_bwa + ".profile.route-tmp";
    if (first_pass) add_bam(files, f_bwa, true);
    if (first_pass && refine) { files.add(f_ep, profile_tmp + ".errorprofile"); files.add(f_ip, profile_tmp + ".indelprofile"); }
    if (refine) add_bam(files, f_para, true);
    if (with_t) { add_bam(files, f_tr, false); add_bam(files, f_comb, true); }
    if (keep_un) files.add(f_un);
    files.refuse_inputs({o.reads_fq, o.ref_fa, refine ? o.ref_refine : nullptr, o.transcripts_fa, o.error_profile, o.indel_profile}, who);
    { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error(who + "no HIP device available: parasuite-hip has no CPU path"); }

    const auto t_begin = clk::now();
    ps_route_stats st; std::memset(&st, 0, sizeof st);
    Route r(o, ref_genome, ref_refine, threads, gm, files);
    std::string step = "first pass";
    try {
        const bool weak_after_first = with_t && !refine;
        std::string ep = given ? o.error_profile : "", ip = has(o.indel_profile) ? o.indel_profile : "";
        if (first_pass) {
            const auto t0 = clk::now();
            MapJob job; r.lend(job, Route::kGenome);
            if (refine && !ref_refine) job.outs.emplace_back(new ProfileOut(gm, max_len, profile_tmp, threads, job.s_profile));
            if (weak_after_first) job.outs.emplace_back(new PieceFn([&r](Batch &b) { r.weak_of(b); }));
            else if (refine) job.outs.emplace_back(new PieceFn([&r](Batch &b) { r.keep(b); }));
            r.pass(job, bwa_mm, nullptr, nullptr, ref_genome, f_bwa, gm, false, weak_after_first ? &r.G : nullptr, st.first);
            st.n_reads = (uint64_t)job.n_reads; st.s_parse = job.s_parse; st.s_index_genome = job.s_index; st.n_fastq_parses = 1;
            st.s_first = secs_since(t0);
            if (refine) {
                step = "profile";
                const auto t1 = clk::now();
                if (ref_refine) {          // the profile of the written file against the other reference, contigs by name: ps_error_profile's path
                    const int dev = r.set_of(Route::kGenome).xs[0]->device;
                    if (!index_files_exist(ref_refine)) {
                        require_device(dev);
                        StreamGuard sg; Index tmp; index_build(ref_refine, tmp, sg.s); index_save(tmp, ref_refine);
                    }
                    ProfileCounts pc;
                    error_profile_count(f_bwa.c_str(), ref_refine, max_len, dev, threads, pc, 0, nullptr);
                    error_profile_write(pc, profile_tmp);
                }
                files.publish(f_ep); files.publish(f_ip);
                ep = f_ep; ip = f_ip;
                st.s_profile = secs_since(t1);
            }
        }
        if (refine) {
            step = "refine pass";
            const auto t0 = clk::now();
            MapJob job; r.lend(job, Route::kRefine);
            if (first_pass && r.kept_all) job.reads = &r.kept; else ++st.n_fastq_parses;
            if (with_t) job.outs.emplace_back(new PieceFn([&r](Batch &b) { r.weak_of(b); }));
            const bool extract_sorted = keep_un && !with_t;      // Main.java:354-357, :382-388
            r.pass(job, para_mm, ep.c_str(), ip.empty() ? nullptr : ip.c_str(), ref_last, f_para, extract_sorted ? 0 : gm, false, with_t ? &r.G : nullptr, st.refine, !extract_sorted);
            if (!first_pass) { st.n_reads = (uint64_t)job.n_reads; st.s_parse = job.s_parse; st.s_index_genome = job.s_index; }
            if (extract_sorted) {          // the sorted, unfiltered file under its temporary name -> the records it keeps + U, then the index of the file as it ends up
                const std::string t = files.tmp(f_para), t_kept = t + ".kept";
                ExtractStats es;
                extract_weak_reads(t.c_str(), t_kept.c_str(), files.tmp(f_un).c_str(), gm, threads, &es);
                if (std::rename(t_kept.c_str(), t.c_str()) != 0) { ::unlink(t_kept.c_str()); throw Error("cannot rename " + t_kept + " to " + t); }
                bam_index(t.c_str(), threads);
                files.publish(f_para); files.publish(f_para + ".bai"); files.publish(f_un);
                st.refine.n_out = es.n_kept; st.refine.bam_bytes = es.bam_bytes;
                st.extract.n_records = es.n_records; st.extract.n_weak = es.n_weak; st.extract.n_kept = es.n_kept;
            }
            st.s_refine = secs_since(t0);
        }
        r.kept.clear();
        if (keep_un && with_t) { write_text_file(files.tmp(f_un), r.weak_fq); files.publish(f_un); r.weak_fq = std::string(); }    // the first extraction's, kept (:405-407)
        if (keep_un && !with_t && !refine) { write_text_file(files.tmp(f_un), ""); files.publish(f_un); }     // the first pass has dropped MAPQ < Q already: empty, as in the Java
        if (with_t) {
            step = "transcript pass";
            const auto t0 = clk::now();
            st.extract.n_records = st.n_reads; st.extract.n_weak = r.n_weak; st.extract.n_kept = st.n_reads - r.n_weak;
            MapJob job; r.lend(job, Route::kTranscripts); job.reads = &r.weak;
            r.pass(job, refine ? para_mm : bwa_mm, refine ? ep.c_str() : nullptr, refine && !ip.empty() ? ip.c_str() : nullptr, o.transcripts_fa, f_tr, tm, true, &r.T, st.transcript);
            st.s_index_transcripts = job.s_index; st.s_transcript = secs_since(t0);
            step = "combine";
            const auto t1 = clk::now();
            const int dev = r.set_of(refine && ref_refine ? Route::kRefine : Route::kGenome).xs[0]->device;      // the first device of the passes
            combine_records(r.G, r.T, f_tr.c_str(), files.tmp(f_comb).c_str(), true, true, threads, dev, &st.combine);
            files.publish(f_comb); files.publish(f_comb + ".bai");
            st.s_combine = secs_since(t1);
        }
        step = "closing";
        st.n_index_loads_genome = (uint32_t)(r.loads_of(Route::kGenome) + r.loads_of(Route::kRefine)); st.n_index_loads_transcripts = (uint32_t)r.loads_of(Route::kTranscripts);
        r.close();
        r.use.done();
        files.keep();
    } catch (const std::exception &e) {
        const std::string m = e.what();
        r.close();
        throw Error(who + step + ": " + m);      // what the call wrote goes with `files`
    }
    st.s_total = secs_since(t_begin);
    if (stats_out) *stats_out = st;
    if (std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip] ps_map_route: %llu reads, %.3f s: parse %.3f s (the file was parsed %u time(s)), genome index resident after %.3f s (%u load(s)), first pass %.3f s, "
                             "profile files %.3f s, refine pass %.3f s, %llu weak reads, transcript index after %.3f s (%u load(s)), transcript pass %.3f s, combine %.3f s\n",
                     (unsigned long long)st.n_reads, st.s_total, st.s_parse, st.n_fastq_parses, st.s_index_genome, st.n_index_loads_genome, st.s_first, st.s_profile, st.s_refine,
                     (unsigned long long)st.extract.n_weak, st.s_index_transcripts, st.n_index_loads_transcripts, st.s_transcript, st.s_combine);
}
}

void map_route(const ps_route_opts *in, ps_route_stats *stats_out)
{
    if (!in) throw Error("ps_map_route: no options");
    ps_route_opts2 o; std::memset(&o, 0, sizeof o);          // ref_refine NULL, keep_unaligned 0, search NULL
    o.struct_size = (uint32_t)sizeof o;
    o.reads_fq = in->reads_fq; o.ref_fa = in->ref_fa; o.out_prefix = in->out_prefix; o.transcripts_fa = in->transcripts_fa;
    o.bwa_mm = in->bwa_mm; o.parasuite_mm = in->parasuite_mm; o.error_profile = in->error_profile; o.indel_profile = in->indel_profile;
    o.threads = in->threads; o.refine = in->refine; o.max_read_len = in->max_read_len; o.mapq_genomic = in->mapq_genomic; o.mapq_transcript = in->mapq_transcript;
    route_run(o, "ps_map_route: ", stats_out);
}
void map_route_opts(const ps_route_opts2 *in, ps_route_stats *stats_out)
{
    ps_route_opts2 o;
    route_opts_read(in, o);
    route_run(o, "ps_map_route_opts: ", stats_out);
}

}  // namespace ps

