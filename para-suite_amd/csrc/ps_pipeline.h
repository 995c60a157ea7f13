// ps_pipeline.h -- batch pipeline behind the C ABI (host orchestration of the gfx950 kernels): the one interface of
// ps_pipeline.hip (context, batch set-up), ps_search.hip (search stage) and ps_samse.hip (selection, locate).
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include "ps_host.h"
#include "ps_search_opts.h"
#include "ps_reads.h"
#include "ps_bam.h"

namespace ps {

static const int PS_HIT_CIGAR = PS_MAX_CIGAR;   // what the banded alignment hands back and a ps_hit holds: 2 * max_gapo + 1 operations for every accepted -o
struct Multi { int64_t pos; bwtint row; int32_t gap, mm, ref_shift, strand, n_cigar; uint32_t cigar[PS_MAX_CIGAR]; };
struct Hit {
    int64_t pos; bwtint sa;
    int32_t type, strand, mapq, n_mm, n_gapo, n_gape, ref_shift, score, c1, c2, n_cigar;
    int32_t multi_begin, n_multi;
    uint32_t cigar[PS_HIT_CIGAR];    // a gapped hit whose alignment has more operations fails the call (ps_samse.hip: take_cigar)
};

static const uint8_t PS_CLS_HOST = 4;   // bit of a read's class (Batch::h_class): finished on the host (Batch::sub), not by the device records below
// per-read records of the samse stage for reads finished on the device
struct SelRec { bwtint sa; int32_t c1, c2; uint8_t type, n_mm, n_gapo, n_gape; int8_t ref_shift; uint8_t score, pad[2]; };   // 24 B
struct FinRec { int64_t pos; uint8_t strand, mapq, type, pad[5]; };                                                        // 16 B
struct DevCigar { int64_t g; int32_t n; uint32_t c[PS_HIT_CIGAR]; };
// a read finished on the host: several best-score intervals (sequential tie-break), alternative hits, or a larger tier
struct SubRead { int64_t g = 0, easy_before = 0, hard_before = 0; uint8_t cls = 0; const AlnRec *alns = nullptr; int32_t n_alns = 0; Hit hit; };   // alns: into Batch::sub_alns or a Bin's overflow list

struct Timing {
    double ms_width = 0, ms_backtrack = 0, ms_select = 0, ms_sa2pos = 0, ms_refine = 0, ms_host_post = 0, ms_total = 0, ms_classify = 0, ms_sel_hard = 0, ms_sel_easy = 0;
    int n_width_launches = 0, n_backtrack_launches = 0;
    double bt_begin_ms = 0, bt_end_ms = 0;   // first search launch's start / last one's end on the context's clock (overlapping batches: the union)
};

// Page-locked host memory is dear to get and to give back (hundreds of MB per piece of a ps_map call: ~50 ms to lock, as much to
// unlock): buffers that are let go are kept, up to a bound, and handed to the next taker (the pieces of one call, the next
// call of the process).  pin_cache_release() gives everything kept back to the system.
void *pin_cache_take(size_t need, size_t &got);
void pin_cache_give(void *p, size_t bytes);
void pin_cache_release();
struct PinBuf {                     // page-locked host staging (D2H at PCIe rate instead of pageable copies)
    void *p = nullptr; size_t bytes = 0;
    PinBuf() {}
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { if (p) pin_cache_give(p, bytes); }
    void *get(size_t need) { if (need > bytes) { if (p) pin_cache_give(p, bytes); p = nullptr; bytes = 0; p = pin_cache_take(need, bytes); } return p; }
};

// One lane of work on the device: a stream with its own grow-only device workspace and pinned staging (hipMalloc /
// hipFree of GBs per call is slow).  A context has two, so that two batches can be in flight -- one batch's kernel tail
// and host-side stages overlap with the other's search kernel.
struct Work {
    hipStream_t stream = nullptr;
    std::map<std::string, DevBuf<uint8_t>> ws; std::map<std::string, PinBuf> pin;
    template <class T> T *ws_get(const std::string &name, size_t count) {
        DevBuf<uint8_t> &b = ws[name];
        const size_t need = count * sizeof(T);
        if (b.n < need) b.alloc(need + need / 8);
        return reinterpret_cast<T *>(b.p);
    }
    template <class T> T *pin_get(const std::string &name, size_t count) { return reinterpret_cast<T *>(pin[name].get(count * sizeof(T) + 64)); }
    Work() {}
    Work(const Work &) = delete;
    Work &operator=(const Work &) = delete;
    ~Work() { if (stream) (void)hipStreamDestroy(stream); }
};

struct Ctx : OptionParts {          // opt, search: the options in their two parts (ps_model.h)
    int device = 0;
    hipStream_t stream = nullptr;    // index build / load
    hipEvent_t ref_event = nullptr;  // the context's clock: recorded once at creation
    Index ix;
    int cus = 256;                 // compute units of the device, read once by attach_device()
    int bt_blocks = 0;             // grid of the backtracking kernel (0 = 4 blocks per CU)
    uint32_t pool_cap[3] = {16384, 65535, 2000064};   // stack entries per lane: 16-byte narrow tiers, then the wide tier
    int aln_cap[3] = {8, 256, 65536};
    int aln_cap_short = 32;        // first tier, bins whose longest read has at most 40 bases (adapter-trimmed PAR-CLIP reads, the transcript pass): short reads
                                   // hit many places by chance -- 1.7 % of 18-40 bp reads list more than 8 intervals, 0.3 % more than 32; 0 = as aln_cap[0]
    bool want_kstats = false;      // search kernel with counters (KStats of the backtracking stage): measurement runs only
    bool want_read_iters = false; std::vector<uint32_t> read_iters;   // profiling aid: last launch's per-read profile (ps_types.h: BtArgs::read_iters), PS_RI_WORDS words per read, in the order the launch held the reads (a bin's leading-base order)
    // ... and, in the same mode, what that launch was prepared with (ps_search.hip: search_order), by the same read index; empty where the launch made no order
    struct LaunchOrder { std::vector<uint8_t> est, key; std::vector<float> pred; std::vector<int32_t> order, ids; void clear() { est.clear(); key.clear(); pred.clear(); order.clear(); ids.clear(); } } launch_order;
    int n_big = 4096;              // 1 MB stack slots a launch may hand to reads that outgrow their private slice
    int fetch_min = 8, hit_min = 1;    // batching hits costs more in idle lanes than it saves (measured)
    int host_threads = 8;
    int collapse_mode = -1;        // identical reads of a bin searched once (ps_collapse.h): -1 as PS_COLLAPSE says at search time, 0 off, 1 on
    static const int N_WORK = 4;
    std::unique_ptr<Work> work[N_WORK];
    int n_work = 1, next_work = 0; // lanes in use (1: every batch shares one workspace and stream); batches take them in turn
    Work *take_work();             // creates the lane's stream on first use
    Work *work_at(int i);          // lane i (ps_map: one per worker thread of the device); thread safe
    std::mutex work_mu;
    std::shared_ptr<void> rec_tables;   // the device route of the BAM records (ps_bamrec.hip): contig and hole tables on the device, uploaded once per context (work_mu)
    // A context in two steps: options and knobs (no device call: ps_map's parser needs nothing else and starts before the runtime is
    // up, which takes 0.2-0.3 s in a fresh process), then the device side (stream, clock).
    explicit Ctx(int device);      // reads the tuning knobs from the environment (PS_FETCH_MIN, PS_N_BIG, ...)
    void attach_device();          // needs a HIP device (stream, clock, CU count); a second call does nothing
    void set_stock(const char *n_arg);                                            // bwa aln's -n
    void set_profile(const char *ep, const char *ip, const char *x_arg);          // the two profile files and -X
    void set_profile_matrix(const double P[16], double ins, double del, int x);
    void set_search(const ps_search_opts *o);                                     // NULL: the defaults; throws what ps_search_opts_check names
    void set_options(const char *mm, const char *ep, const char *ip) { if (ep && ep[0]) set_profile(ep, ip, mm); else set_stock(mm && mm[0] ? mm : "0.04"); }   // a mapping call's three arguments
    ~Ctx();
};

// Reads of one *cost class* -- lengths that get the same difference budget, seed rule and local-memory layout --
// share a bin and a launch; len is the longest of them, lens the length of every read (adapter-trimmed input has
// dozens of lengths: one launch per length would leave the device mostly idle).
struct Bin {
    int len = 0; Model md;
    bool ragged = false;                      // more than one length present
    std::vector<int32_t> lens; DevBuf<int32_t> d_lens;     // bin-local; d_lens allocated only when ragged
    std::vector<int32_t> ids;                 // global read index of every local read
    DevBuf<uint32_t> bases, nmask;
    RawVec<uint32_t> h_bases, h_nmask;        // host copy (tier re-runs gather from it); every word is written by the packing threads, none zero-filled first
    DevBuf<int32_t> d_ids;                     // ids on the device (bin-local -> input order)
    DevBuf<AlnRec> d_alns; DevBuf<int32_t> d_n_aln; DevBuf<uint8_t> d_status; int aln_cap = 0;   // first-tier hit lists stay in HBM
    bool host_alns_valid = false;             // compact host copy, downloaded on demand (tests, ps_batch_alns)
    std::vector<int32_t> h_n_aln; std::vector<uint32_t> h_off; std::vector<AlnRec> h_alns;
    std::map<int32_t, std::vector<AlnRec>> overflow;                                          // reads that needed a larger tier
    int n_bw = 0, n_mw = 0;
    std::vector<int32_t> h_rep_of;            // collapsed search: bin-local read -> its group's representative; empty: every read stands for itself
};

// The BAM records of a located batch as the device route makes them (ps_bamrec.hip): one page-locked buffer with every kept record in
// input order, recs[i].off / len into it (part 0), origin[i] 1 where the host built the record (a PS_CLS_HOST read) and 0 where the device did
struct DevRecords {
    PinBuf pin; const uint8_t *bytes = nullptr; size_t n_bytes = 0;
    std::vector<BamRec> recs; std::vector<uint8_t> origin;
    uint64_t n_reads = 0, n_device = 0, n_host = 0;
    double ms_upload = 0, ms_kernels = 0, ms_host_records = 0, ms_download = 0;
};

struct Batch {
    Ctx *ctx = nullptr;
    Work *wk = nullptr;            // the lane of work this batch runs on
    int work_index = -1;           // >= 0: the lane to use (ps_map's workers); -1: the context's next one
    ReadSet rs;
    std::vector<Bin> bins;
    std::vector<int32_t> read_bin, read_local;
    // samse stage: classes and device records in input order; the host-finished subset
    DevBuf<uint8_t> d_class; DevBuf<uint32_t> d_eb, d_hb; DevBuf<bwtint> d_rows, d_pos; DevBuf<SelRec> d_sel; DevBuf<FinRec> d_fin;
    PinBuf p_class, p_sel, p_fin, p_grp;
    uint8_t *h_class = nullptr; SelRec *h_sel = nullptr; FinRec *h_fin = nullptr;
    uint32_t *h_grp = nullptr;     // class-1 / class-2 reads in front of every group of 64 reads (input order), pairs
    std::vector<SubRead> sub; std::vector<Multi> multis; std::vector<DevCigar> dev_cigars;
    std::vector<std::unique_ptr<PinBuf>> sub_alns;   // per bin: hit lists of the host-finished reads (stride aln_cap)
    int64_t n_class1 = 0, n_hard = 0;
    std::vector<uint64_t> hard_draws_cum;  // draws consumed by the several-best reads up to and including each
    uint64_t draws_in = 0, draws_out = 0;
    DevBuf<KStats> d_stats; KStats st_width{}, st_backtrack{}, st_sa2pos{};
    Timing tm;
    int64_t n_overflow[3] = {0, 0, 0};
    bool collapse_known = false, collapse_on = false; ps_collapse_info collapse{};   // the last search: identical reads searched once, and what that saved
    bool searched = false, selected_hard = false, selected = false, located = false;
    const AlnRec *alns_of(int64_t g, int &n);      // downloads the hit lists on first use
    void ensure_host_alns();
    void hit_of(int64_t g, Hit &h) const;
    std::unique_ptr<DevRecords> dev_records; int dev_records_mapq = 0;   // ps_map with the device route on: the worker's result for the pass's BamRecords output (its MAPQ filter)
    void release_device();         // after batch_locate: everything batch_write_sam / hit_of read is in host memory
};

std::unique_ptr<Batch> batch_create(Ctx *ctx, ReadSet &&rs);   // bins by cost class, packs 2-bit, uploads (= prepare + upload)
std::unique_ptr<Batch> batch_prepare(Ctx *ctx, ReadSet &&rs, int threads);   // host half: needs ctx->opt only, no device call
void batch_upload(Batch &b);                                                  // device half
void batch_search(Batch &b);                                    // width + backtracking kernels (+ larger tiers), hit lists to host
void batch_select_hard(Batch &b, uint64_t draws_before, uint64_t *draws_after);
void batch_select_easy(Batch &b, int threads);
void ctx_release_device(Ctx &c);                               // every device allocation of the context (index blobs, lanes of work) freed; host-side reference data stays
void reserve_search_workspace(Ctx *ctx, int work_index);        // the big device allocations of a lane of work, ahead of its first search
void batch_locate(Batch &b);                                    // SA walk kernel, strand / MAPQ, banded DP of gapped hits
void batch_bam_records(const Batch &b, int min_mapq, int threads, std::vector<std::string> &enc, std::vector<std::vector<BamRec>> &recs);   // the located batch as BAM records (MAPQ >= min_mapq): one buffer per thread, buffers in input order
// the records of the host-finished reads alone (Batch::sub, in its order), for the device route to splice in: recs[i] is sub[i]'s record -- part: its
// buffer, off / len into that buffer, len 0: below the MAPQ filter
void batch_bam_records_sub(const Batch &b, int min_mapq, int threads, std::vector<std::string> &enc, std::vector<BamRec> &recs);
// The same records built on the device that mapped the batch (ps_bamrec.hip), after batch_locate and before Batch::release_device, on the
// batch's own lane: the device builds the record of every read it finished itself, the host those of the PS_CLS_HOST reads (on `threads`
// threads, while the size kernel runs), and one buffer in input order comes down.  A HIP error throws; there is no fallback to the host route.
void batch_bam_records_device(Batch &b, int min_mapq, int threads, DevRecords &out);
// the switch of ps_bam_records_device / PS_BAM_RECORDS_GPU (off by default) and the counters since it was last set
bool bam_records_device_on();
void bam_records_device_set(bool on);
void bam_records_info(ps_bam_records_stats &out);
void bam_records_count(const ps_bam_records_stats &add);
std::string sam_header(const RefSeq &ref, const char *pg_line);      // @SQ lines in FASTA order + the @PG line
// text buffers of the SAM writer, kept from piece to piece by ps_map: fresh ones are first touched page by page, and a page fault waits
// while another thread gives a finished piece's gigabytes back to the system (0.2 s per piece, measured)
struct SamScratch { std::vector<std::string> bufs[2]; };
void batch_write_sam(Batch &b, const char *path, bool header, const char *pg_line, int threads, bool append = false, SamScratch *scratch = nullptr);
// the located hits with MAPQ >= min_mapq as records for the error-profile kernel (what the MAPQ-filtered BAM of the first pass holds:
// PARAsuiteMapping.java:124-133 -> ErrorProfiling.java:145-172), appended to `out`; host memory only
void batch_profile_records(const Batch &b, int min_mapq, int threads, ProfRecords &out);

}  // namespace ps
