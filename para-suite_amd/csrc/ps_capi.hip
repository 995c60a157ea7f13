// ps_capi.hip -- extern "C" boundary (include/parasuite_hip.h).  Exceptions stop here: every entry point converts its structs, checks
// its arguments, makes one call into the library (which throws ps::Error) and turns what is thrown into a status and ps_last_error().
#include <hip/hip_runtime.h>
#include <chrono>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/parasuite_hip.h"
#include "ps_pipeline.h"
#include "ps_map.h"
#include "ps_bam.h"
#include "ps_host.h"
#include "ps_bgzf.h"
#include "ps_bamsort.h"
#include "ps_namesort.h"

using namespace ps;

static thread_local std::string g_err;
static int fail(const std::string &m) { g_err = m; std::fprintf(stderr, "[parasuite-hip] error: %s\n", m.c_str()); return 1; }
#define PS_TRY try {
#define PS_CATCH_INT } catch (const std::exception &e) { return fail(e.what()); } catch (...) { return fail("unknown error"); }
#define PS_CATCH_PTR } catch (const std::exception &e) { fail(e.what()); return nullptr; } catch (...) { fail("unknown error"); return nullptr; }

struct ps_ctx { Ctx c; explicit ps_ctx(int device) : c(device) {} };
struct ps_batch { std::unique_ptr<Batch> b; };

static_assert(sizeof(ps_aln) == sizeof(AlnRec), "ps_aln layout");
static void put(ps_bam_stats *st, const BamStats &s) { if (st) { st->n_in = s.n_in; st->n_out = s.n_out; st->bam_bytes = s.bam_bytes; } }
static int first_device() { const char *e = std::getenv("PARASUITE_GPU_IDS"); return e ? std::atoi(e) : 0; }     // the calls that use one device
// what ps_error_profile (quals 0: the mapper's two files) and ps_error_profile_full (1, 2: all six) do: count, write, publish together
static void profile_files(const std::string &who, const char *mapping, const char *ref_fa, int max_len, const char *out_prefix, int quals, ProfileCounts &c, double *ms_parse)
{
    static const char *const ext[6] = {".errorprofile", ".indelprofile", ".errorprofile.vcf", ".qualityPerMismatch", ".indels", ".qualities"};
    if (!mapping || !ref_fa) throw Error(who + "mapping and reference are required");
    const std::string ref = ref_fa, prefix = out_prefix && out_prefix[0] ? out_prefix : mapping, tmp = prefix + ".profile-tmp";
    OutFiles files(".profile-tmp");
    for (int k = 0; k < (quals ? 6 : 2); ++k) files.add(prefix + ext[k], tmp + ext[k]);
    files.refuse_inputs({mapping, ref_fa, (ref + ".ann").c_str(), (ref + ".pac").c_str()}, who);
    error_profile_count(mapping, ref_fa, max_len, first_device(), 8, c, quals, ms_parse);
    error_profile_write(c, tmp);
    if (quals) error_profile_write_extra(c, tmp);
    files.publish_all(); files.keep();
}

extern "C" {

const char *ps_version(void) { return "parasuite-hip 0.1 (gfx950)"; }
const char *ps_last_error(void) { return g_err.c_str(); }

static ps_ctx *new_ctx(int device)                 // options and knobs, then the device side (ps_pipeline.h: Ctx)
{
    std::unique_ptr<ps_ctx> x(new ps_ctx(device));
    x->c.attach_device();
    return x.release();
}

// a second context on `device` holding a COPY of src's index (blobs + jump table, device to device: the route ps_map takes for every
// device after the first; src and the new context may be on the same device)
ps_ctx *ps_ctx_clone(ps_ctx *src, int device)
{
    PS_TRY
        std::unique_ptr<ps_ctx> x(new_ctx(device));
        index_clone(src->c.ix, src->c.device, x->c.ix, device, x->c.stream);
        return x.release();
    PS_CATCH_PTR
}

ps_ctx *ps_ctx_open(const char *ref_fa, int device)
{
    PS_TRY
        std::unique_ptr<ps_ctx> x(new_ctx(device));
        index_load(ref_fa, x->c.ix, x->c.stream);
        return x.release();
    PS_CATCH_PTR
}
ps_ctx *ps_ctx_build(const char *ref_fa, int device, int save_files)
{
    PS_TRY
        std::unique_ptr<ps_ctx> x(new_ctx(device));
        index_build(ref_fa, x->c.ix, x->c.stream);
        if (save_files) index_save(x->c.ix, ref_fa);
        return x.release();
    PS_CATCH_PTR
}
void ps_ctx_close(ps_ctx *x) { delete x; }

int ps_index(const char *ref_fa)
{
    PS_TRY
        resident_invalidate(ref_fa);                 // inside a resident scope: the entries of this path go before its files are written
        ps_ctx *x = ps_ctx_build(ref_fa, 0, 1);
        if (!x) return 1;
        delete x;
        return 0;
    PS_CATCH_INT
}

int ps_ctx_set_stock(ps_ctx *x, const char *n_arg) { PS_TRY x->c.set_stock(n_arg); return 0; PS_CATCH_INT }
int ps_ctx_set_profile_matrix(ps_ctx *x, const double P[16], double ins, double del, int xarg)
{
    PS_TRY
        x->c.set_profile_matrix(P, ins, del, xarg); return 0;
    PS_CATCH_INT
}
int ps_ctx_set_profile(ps_ctx *x, const char *ep, const char *ip, const char *x_arg) { PS_TRY x->c.set_profile(ep, ip, x_arg); return 0; PS_CATCH_INT }
void ps_search_opts_default(ps_search_opts *o) { if (o) search_opts_default(*o); }
int ps_search_opts_check(const ps_search_opts *o, int profile_mode)
{
    PS_TRY
        std::string err;
        if (!search_opts_check(o, profile_mode != 0, err)) throw Error(err);
        return 0;
    PS_CATCH_INT
}
int ps_ctx_set_search(ps_ctx *x, const ps_search_opts *o) { PS_TRY x->c.set_search(o); return 0; PS_CATCH_INT }
// SA[row] for arbitrary rows of the BW matrix (LF walk to a sampled row: the kernel the samse stage uses): index checks
// every row of the index against the text (ps_kernels.hip: k_index_check): out = rows visited (must be seq_len + 1), BWT symbols that differ
// from the text, SA samples that differ from the position counted along the LF cycle, longest arc between two samples
int ps_ctx_index_check(ps_ctx *x, uint64_t out[4])
{
    PS_TRY
        Ctx &c = x->c;
        require_device(c.device);
        DevBuf<unsigned long long> d; d.alloc(4);
        PS_HIP(hipMemsetAsync(d.p, 0, 32, c.stream));
        launch_index_check(c.ix.view, d.p, c.stream);
        PS_HIP(hipGetLastError());
        unsigned long long h[4];
        d.download(h, 4, c.stream);
        PS_HIP(hipStreamSynchronize(c.stream));
        for (int j = 0; j < 4; ++j) out[j] = h[j];
        return 0;
    PS_CATCH_INT
}
int ps_ctx_order_sort(ps_ctx *x, const uint8_t *keys, int64_t n, int32_t *order)
{
    PS_TRY
        Ctx &c = x->c;
        require_device(c.device);
        if (n < 0 || n > 0x7fffffff) throw Error("order sort: bad count");
        if (n) {
            DevBuf<uint8_t> d_k; DevBuf<int32_t> d_o; DevBuf<uint32_t> d_t;
            d_k.alloc((size_t)n); d_o.alloc((size_t)n); d_t.alloc(order_sort_tmp_words((int)n));
            d_k.upload(keys, (size_t)n, c.stream);
            launch_order_sort(d_k.p, (int)n, d_t.p, d_o.p, c.stream);
            PS_HIP(hipGetLastError());
            d_o.download(order, (size_t)n, c.stream);
            PS_HIP(hipStreamSynchronize(c.stream));
        }
        return 0;
    PS_CATCH_INT
}
int ps_ctx_sa_lookup(ps_ctx *x, const uint64_t *rows, int64_t n, uint64_t *out)
{
    PS_TRY
        Ctx &c = x->c;
        require_device(c.device);
        if (n < 0 || n > 0x7fffffff) throw Error("sa lookup: bad count");
        for (int64_t i = 0; i < n; ++i) if (rows[i] < 1 || rows[i] > c.ix.view.seq_len) throw Error("sa lookup: row outside [1, n]");
        DevBuf<bwtint> d_r, d_p; d_r.alloc((size_t)std::max<int64_t>(1, n)); d_p.alloc((size_t)std::max<int64_t>(1, n));
        if (n) {
            d_r.upload((const bwtint *)rows, (size_t)n, c.stream);
            launch_sa2pos(c.ix.view, d_r.p, d_p.p, (int)n, nullptr, c.stream);
            PS_HIP(hipGetLastError());
            d_p.download((bwtint *)out, (size_t)n, c.stream);
        }
        PS_HIP(hipStreamSynchronize(c.stream));
        return 0;
    PS_CATCH_INT
}
int ps_ctx_set_lanes(ps_ctx *x, int n)
{
    PS_TRY
        if (n < 1 || n > (int)Ctx::N_WORK) throw Error("lanes: 1 to 4");
        x->c.n_work = n; return 0;
    PS_CATCH_INT
}
int ps_ctx_set_stats(ps_ctx *x, int on)
{
    PS_TRY
        x->c.want_kstats = on != 0; return 0;
    PS_CATCH_INT
}
int ps_ctx_set_tiers(ps_ctx *x, const uint32_t pool_cap[3], const int32_t aln_cap[3], int bt_blocks)
{
    PS_TRY
        for (int t = 0; t < 3; ++t) { if (pool_cap) x->c.pool_cap[t] = pool_cap[t]; if (aln_cap) x->c.aln_cap[t] = aln_cap[t]; }
        if (aln_cap) x->c.aln_cap_short = (aln_cap[0] == 8) ? 32 : 0;                  // stated sizes hold for every length; the default gets its short-read rule back
        x->c.bt_blocks = bt_blocks; return 0;
    PS_CATCH_INT
}
int ps_ctx_info(ps_ctx *x, ps_index_info *o)
{
    PS_TRY
        const Index &ix = x->c.ix;
        o->seq_len = ix.view.seq_len; o->l_pac = ix.view.l_pac; o->primary = ix.view.primary;
        for (int j = 0; j < 5; ++j) o->L2[j] = ix.view.L2[j];
        o->n_blocks = ix.view.n_blocks; o->n_sa = ix.view.n_sa; o->device_bytes = ix.device_bytes();
        o->n_contigs = (int)ix.ref.contigs.size(); o->n_holes = (int)ix.ref.holes.size(); o->sa_rounds = ix.sa_rounds; o->sa_intv = ix.view.sa_intv;
        o->build_ms = ix.build_ms; o->jump_levels = ix.jump_levels; o->pad_ = 0; return 0;
    PS_CATCH_INT
}
int ps_ctx_blob(ps_ctx *x, int which, void **p, uint64_t *bytes)
{
    PS_TRY
        Index &ix = x->c.ix;
        if (which == 0) { *p = ix.blocks.p; *bytes = ix.blocks.n * sizeof(OccBlock); }
        else if (which == 1) { *p = ix.sa.p; *bytes = ix.sa.n * sizeof(uint32_t); }
        else if (which == 2) { *p = ix.pac.p; *bytes = ix.pac.n; }
        else throw Error("blob index out of range");
        return 0;
    PS_CATCH_INT
}
int64_t ps_ctx_meta(ps_ctx *x, char *buf, int64_t cap)
{
    try {
        std::string m = index_meta_serialize(x->c.ix);
        if (buf && cap >= (int64_t)m.size()) std::memcpy(buf, m.data(), m.size());
        return (int64_t)m.size();
    } catch (const std::exception &e) { fail(e.what()); return -1; }
}
ps_ctx *ps_ctx_from_blobs(const char *meta, int64_t meta_len, int device, void *const ptrs[3])
{
    PS_TRY
        std::unique_ptr<ps_ctx> x(new_ctx(device));
        Index &ix = x->c.ix;
        index_meta_deserialize(std::string(meta, (size_t)meta_len), ix);
        const bwtint primary = ix.view.primary; bwtint L2[5]; std::memcpy(L2, ix.view.L2, sizeof L2);
        const size_t nb = ix.view.n_blocks, ns = ix.view.n_sa, np = (size_t)ix.ref.l_pac / 4 + 1;
        ix.blocks.adopt((OccBlock *)ptrs[0], nb); ix.sa.adopt((uint32_t *)ptrs[1], Index::sa_words(ns)); ix.pac.adopt((uint8_t *)ptrs[2], np);
        ix.ref.pac.resize(np);
        PS_HIP(hipMemcpy(ix.ref.pac.data(), ix.pac.p, np, hipMemcpyDeviceToHost));
        ix.refresh_view();
        ix.view.primary = primary; std::memcpy(ix.view.L2, L2, sizeof L2);
        index_build_jump(ix, nullptr);
        return x.release();
    PS_CATCH_PTR
}
int ps_ctx_fetch(ps_ctx *x, int which, void *dst, uint64_t bytes)
{
    PS_TRY
        void *p; uint64_t n;
        if (ps_ctx_blob(x, which, &p, &n)) return 1;
        if (bytes > n) throw Error("fetch larger than blob");
        PS_HIP(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
        return 0;
    PS_CATCH_INT
}

int ps_ctx_export_blob(ps_ctx *x, int which, void *dst, uint64_t bytes)
{
    PS_TRY
        void *p; uint64_t n;
        if (ps_ctx_blob(x, which, &p, &n)) return 1;
        if (bytes != n) throw Error("export size differs from blob size");
        PS_HIP(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToDevice));
        return 0;
    PS_CATCH_INT
}

ps_batch *ps_batch_from_fastq(ps_ctx *x, const char *fastq)
{
    PS_TRY
        require_device(x->c.device);
        ReadSet rs; load_reads(fastq, rs, x->c.host_threads);
        ps_batch *b = new ps_batch();
        b->b = batch_create(&x->c, std::move(rs));
        return b;
    PS_CATCH_PTR
}
ps_batch *ps_batch_from_codes(ps_ctx *x, int64_t n, int len, const uint8_t *codes)
{
    PS_TRY
        require_device(x->c.device);
        ReadSet rs; reads_from_codes(n, len, codes, rs);
        ps_batch *b = new ps_batch();
        b->b = batch_create(&x->c, std::move(rs));
        return b;
    PS_CATCH_PTR
}
void ps_batch_free(ps_batch *b) { delete b; }
int64_t ps_batch_n(ps_batch *b) { return b->b->rs.n; }
int ps_batch_search(ps_batch *b) { PS_TRY batch_search(*b->b); return 0; PS_CATCH_INT }
int ps_batch_select_hard(ps_batch *b, uint64_t before, uint64_t *after) { PS_TRY batch_select_hard(*b->b, before, after); return 0; PS_CATCH_INT }
int ps_batch_select_easy(ps_batch *b, int threads) { PS_TRY b->b->ctx->host_threads = threads > 0 ? threads : 1; batch_select_easy(*b->b, threads); return 0; PS_CATCH_INT }
int ps_batch_locate(ps_batch *b) { PS_TRY batch_locate(*b->b); return 0; PS_CATCH_INT }
int ps_batch_run(ps_batch *b, int threads)
{
    PS_TRY
        b->b->ctx->host_threads = threads > 0 ? threads : 1;
        batch_search(*b->b);
        batch_select_hard(*b->b, 0, nullptr);
        batch_select_easy(*b->b, threads);
        batch_locate(*b->b);
        return 0;
    PS_CATCH_INT
}
int ps_batch_write_sam(ps_batch *b, const char *path, int with_header, int threads)
{
    PS_TRY
        batch_write_sam(*b->b, path, with_header != 0, PS_PG_LINE, threads); return 0;
    PS_CATCH_INT
}
int ps_batch_n_aln(ps_batch *b, int32_t *out, int64_t cap)
{
    PS_TRY
        Batch &B = *b->b;
        for (int64_t g = 0; g < B.rs.n && g < cap; ++g) { int n; B.alns_of(g, n); out[g] = n; }
        return 0;
    PS_CATCH_INT
}
int64_t ps_batch_alns(ps_batch *b, int64_t read, ps_aln *out, int64_t cap)
{
    try {
        int n; const AlnRec *a = b->b->alns_of(read, n);
        for (int j = 0; j < n && j < cap; ++j) std::memcpy(&out[j], &a[j], sizeof(ps_aln));
        return n;
    } catch (const std::exception &e) { fail(e.what()); return -1; }
}
int ps_batch_hits(ps_batch *b, ps_hit *out, int64_t cap)
{
    PS_TRY
        Batch &B = *b->b;
        for (int64_t g = 0; g < B.rs.n && g < cap; ++g) {
            Hit h; B.hit_of(g, h); ps_hit &o = out[g];
            o.pos = h.type ? h.pos : -1; o.sa = h.sa; o.type = h.type; o.strand = h.strand; o.mapq = h.mapq; o.n_mm = h.n_mm; o.n_gapo = h.n_gapo;
            o.n_gape = h.n_gape; o.ref_shift = h.ref_shift; o.score = h.score; o.c1 = h.c1; o.c2 = h.c2; o.n_cigar = h.n_cigar; o.n_multi = h.n_multi;
            std::memset(o.cigar, 0, sizeof o.cigar); std::memcpy(o.cigar, h.cigar, sizeof h.cigar);
        }
        return 0;
    PS_CATCH_INT
}
int64_t ps_ctx_read_iters(ps_ctx *x, uint32_t *out, int64_t cap)
{
    const int64_t n = (int64_t)x->c.read_iters.size();
    for (int64_t i = 0; i < n && i < cap; ++i) out[i] = x->c.read_iters[i];
    return n;
}
int64_t ps_ctx_launch_order(ps_ctx *x, uint8_t *est, uint8_t *key, float *pred, int32_t *order, int32_t *ids, int64_t cap)
{
    const Ctx::LaunchOrder &lo = x->c.launch_order;
    const int64_t n = (int64_t)lo.order.size();
    for (int64_t i = 0; i < n && i < cap; ++i) {
        if (est) est[i] = lo.est[(size_t)i];
        if (key) key[i] = lo.key[(size_t)i];
        if (pred) pred[i] = lo.pred[(size_t)i];
        if (order) order[i] = lo.order[(size_t)i];
        if (ids) ids[i] = lo.ids[(size_t)i];
    }
    return n;
}
int ps_batch_timing(ps_batch *b, ps_timing *o)
{
    PS_TRY
        const Timing &t = b->b->tm;
        o->ms_width = t.ms_width; o->ms_backtrack = t.ms_backtrack; o->ms_compact = 0; o->ms_select = t.ms_select;
        o->ms_sa2pos = t.ms_sa2pos; o->ms_refine = t.ms_refine; o->ms_host_post = t.ms_host_post; o->ms_total = t.ms_total;
        o->ms_classify = t.ms_classify; o->ms_rows = 0; o->ms_sel_hard = t.ms_sel_hard; o->ms_sel_easy = t.ms_sel_easy;
        o->n_width_launches = t.n_width_launches; o->n_backtrack_launches = t.n_backtrack_launches;
        o->n_overflow_tier1 = b->b->n_overflow[1]; o->n_overflow_tier2 = b->b->n_overflow[2];
        o->bt_begin_ms = t.bt_begin_ms; o->bt_end_ms = t.bt_end_ms;
        return 0;
    PS_CATCH_INT
}
int ps_batch_kstats(ps_batch *b, int which, ps_kstats *o)
{
    PS_TRY
        const KStats &k = which == 0 ? b->b->st_width : (which == 1 ? b->b->st_backtrack : b->b->st_sa2pos);
        o->occ_pairs = k.occ_pairs; o->occ_same_blk = k.occ_same_blk; o->nodes = k.nodes; o->pushes = k.pushes; o->pops = k.pops;
        o->lf_steps = k.lf_steps; o->iters = k.iters; o->exact_steps = k.exact_steps; return 0;
    PS_CATCH_INT
}
int ps_ctx_set_collapse(ps_ctx *x, int mode)
{
    PS_TRY
        if (mode < -1 || mode > 1) throw Error("collapse: -1 (as PS_COLLAPSE says), 0 (off) or 1 (on)");
        x->c.collapse_mode = mode; return 0;
    PS_CATCH_INT
}
int ps_batch_collapse_info(ps_batch *b, ps_collapse_info *o)
{
    PS_TRY
        if (!b->b->collapse_known) throw Error("collapse info: the batch has not been searched");
        *o = b->b->collapse; return 0;
    PS_CATCH_INT
}
int ps_batch_duplicate_of(ps_batch *b, int64_t *out, int64_t cap)
{
    PS_TRY
        const Batch &B = *b->b;
        if (!B.collapse_known) throw Error("duplicate_of: the batch has not been searched");
        if (!B.collapse_on) throw Error("duplicate_of: the batch was searched with collapse off");
        for (int64_t g = 0; g < B.rs.n && g < cap; ++g) {
            const Bin &bin = B.bins[(size_t)B.read_bin[g]];
            out[g] = bin.h_rep_of.empty() ? g : (int64_t)bin.ids[(size_t)bin.h_rep_of[(size_t)B.read_local[g]]];
        }
        return 0;
    PS_CATCH_INT
}

// The whole `map` step behind one call: the streaming pass and the route are ps_map.hip's.
int ps_map(int threads, const char *mm, const char *error_profile, const char *indel_profile,
           const char *ref_fa, const char *fastq, const char *out_sam)
{
    PS_TRY
        map_to_sam(MapArgs{threads, mm, error_profile, indel_profile, ref_fa, fastq}, out_sam); return 0;
    PS_CATCH_INT
}
int ps_map_opts(int threads, const char *mm, const char *error_profile, const char *indel_profile,
                const char *ref_fa, const char *fastq, const char *out_sam, const ps_search_opts *opts)
{
    PS_TRY
        map_to_sam(MapArgs{threads, mm, error_profile, indel_profile, ref_fa, fastq, opts}, out_sam); return 0;
    PS_CATCH_INT
}
int ps_map_profiled(int threads, const char *mm, const char *error_profile, const char *indel_profile,
                    const char *ref_fa, const char *fastq, const char *out_sam, int min_mapq, int max_read_len, const char *profile_prefix)
{
    PS_TRY
        if (!profile_prefix || !profile_prefix[0]) throw Error("ps_map_profiled: no output prefix for the profile files");
        profile_check_max_len(max_read_len, 0);
        map_profiled(MapArgs{threads, mm, error_profile, indel_profile, ref_fa, fastq}, out_sam, min_mapq, max_read_len, profile_prefix); return 0;
    PS_CATCH_INT
}
int ps_map_to_bam(int threads, const char *mm, const char *error_profile, const char *indel_profile,
                  const char *ref_fa, const char *fastq, const char *out_bam, int min_mapq, int sort_by_coordinate, int write_index, ps_bam_stats *st)
{
    PS_TRY
        if (write_index && !sort_by_coordinate) throw Error("a .bai index needs coordinate-sorted output");
        BamStats s;
        map_to_bam(MapArgs{threads, mm, error_profile, indel_profile, ref_fa, fastq}, out_bam, min_mapq, sort_by_coordinate != 0, write_index != 0, &s);
        put(st, s);
        return 0;
    PS_CATCH_INT
}
int ps_map_route(const ps_route_opts *o, ps_route_stats *stats_out) { PS_TRY map_route(o, stats_out); return 0; PS_CATCH_INT }
int ps_map_route_opts(const ps_route_opts2 *o, ps_route_stats *stats_out) { PS_TRY map_route_opts(o, stats_out); return 0; PS_CATCH_INT }

// The resident scope: between begin and end the five mapping calls above keep their indexes and lanes of work in HBM (ps_map.hip).
int ps_resident_begin(const ps_resident_opts *o) { PS_TRY resident_begin(o); return 0; PS_CATCH_INT }
int ps_resident_end(void) { PS_TRY resident_end(); return 0; PS_CATCH_INT }
int ps_resident_info(ps_resident_stats *out)
{
    PS_TRY
        if (!out) throw Error("ps_resident_info: no place for the result");
        resident_info(*out); return 0;
    PS_CATCH_INT
}

// page-locked host buffers the library keeps between calls (ps_pipeline.h, PinBuf): given back to the system
void ps_release_host_cache(void) { try { trash_collect(); pin_cache_release(); } catch (...) {} }

int ps_parse_check(const char *reads_path, int threads, uint64_t chunk_bytes, uint64_t out[4]) { PS_TRY parse_check(reads_path, threads, (size_t)chunk_bytes, out); return 0; PS_CATCH_INT }

// The modes below publish their output files one way (ps_outfiles.h): an error leaves none of them.
// Error-profile estimation from a mapping (the stage between the two passes of a --refine run, Main.java:320-340): what
// `new ErrorProfiling(mapping, reference, maxReadLength).inferErrorProfile(false, false)` writes for the mapper.
int ps_error_profile(const char *mapping_sam_or_bam, const char *ref_fa, int max_read_len, const char *out_prefix)
{
    PS_TRY
        ProfileCounts c;
        profile_files("ps_error_profile: ", mapping_sam_or_bam, ref_fa, max_read_len, out_prefix, 0, c, nullptr);
        if (std::getenv("PS_VERBOSE"))
            std::fprintf(stderr, "[parasuite-hip] ps_error_profile: %llu records, %llu counted (%llu unmapped, %llu duplicate, %llu without position, %llu with indels, %llu skipped)\n",
                         c.n_records, c.n_processed, c.n_unmapped, c.n_duplicate, c.n_start_zero, c.n_indel_reads, c.n_skipped);
        return 0;
    PS_CATCH_INT
}

// All six files of ErrorProfiling.inferErrorProfile(infer_qualities, false) -- the toolkit's `error` mode (Main.java:560-597):
// the two above, byte for byte, and .errorprofile.vcf, .qualityPerMismatch, .indels, .qualities.
int ps_error_profile_full(const char *mapping_sam_or_bam, const char *ref_fa, int max_read_len, const char *out_prefix,
                          int infer_qualities, ps_profile_stats *stats)
{
    PS_TRY
        ProfileCounts c;
        double ms_parse = 0;
        profile_files("ps_error_profile_full: ", mapping_sam_or_bam, ref_fa, max_read_len, out_prefix, infer_qualities ? 2 : 1, c, &ms_parse);
        if (stats) {
            stats->n_records = c.n_records; stats->n_counted = c.n_processed; stats->n_unmapped = c.n_unmapped; stats->n_duplicate = c.n_duplicate;
            stats->n_start_zero = c.n_start_zero; stats->n_indel_reads = c.n_indel_reads; stats->n_skipped = c.n_skipped;
            stats->n_without_qual = c.n_without_qual; stats->n_qual_beyond_read = c.n_qual_beyond_read;
        }
        if (std::getenv("PS_VERBOSE"))
            std::fprintf(stderr, "[parasuite-hip] ps_error_profile_full: %llu records, %llu counted (%llu unmapped, %llu duplicate, %llu without position, %llu with indels, %llu skipped, "
                                 "%llu without QUAL, %llu mismatch qualities beyond the read); parse %.1f ms, count kernel %.2f ms, SD kernel %.2f ms\n",
                         c.n_records, c.n_processed, c.n_unmapped, c.n_duplicate, c.n_start_zero, c.n_indel_reads, c.n_skipped,
                         c.n_without_qual, c.n_qual_beyond_read, ms_parse, c.ms_count, c.ms_sd);
        return 0;
    PS_CATCH_INT
}

// The toolkit's `clust` mode (Main.java:601-639): PileupClusters.calculateReadPileups, its six files.
int ps_pileup_clusters(const char *mapping_sam_or_bam, const char *ref_fa, const char *out_file, const char *snp_vcf,
                       int min_read_coverage, const char *site_prefix, ps_cluster_stats *stats)
{
    PS_TRY
        const int dev = first_device();
        pileup_clusters_run(mapping_sam_or_bam, ref_fa, out_file, snp_vcf, min_read_coverage, site_prefix, dev, stats);
        return 0;
    PS_CATCH_INT
}

// Step 2 of `map -t` (Main.java:363-377): ExtractWeakMappingReads.extractReads.  Host code.
int ps_extract_weak_reads(const char *mapping_sam_or_bam, const char *out_bam, const char *out_fastq, int mapq_threshold, int threads,
                          ps_extract_stats *stats)
{
    PS_TRY
        ExtractStats s;
        extract_weak_reads(mapping_sam_or_bam, out_bam, out_fastq, mapq_threshold, threads, &s);
        if (stats) { stats->n_records = s.n_records; stats->n_weak = s.n_weak; stats->n_kept = s.n_kept; stats->bam_bytes = s.bam_bytes; }
        return 0;
    PS_CATCH_INT
}

// The `extractAligned` mode (Main.java:852-880): ExtractNotMappedReads.extractReads.  Host code.
int ps_extract_read_names(const char *mapping_sam_or_bam, const char *out_file, ps_names_stats *stats)
{
    PS_TRY
        NamesStats s;
        extract_read_names(mapping_sam_or_bam, out_file, 4, &s);
        if (stats) { stats->n_records = s.n_records; stats->out_bytes = s.out_bytes; }
        return 0;
    PS_CATCH_INT
}

// Step 5 of `map -t` and the `comb` mode (Main.java:438-488): CombineGenomeTranscript.combine.
int ps_combine_genome_transcript(const char *genome_bam, const char *transcript_bam, const char *out_bam, int sort_by_coordinate,
                                 int write_index, int threads, ps_combine_stats *stats)
{
    PS_TRY
        const int dev = first_device();
        combine_run(genome_bam, transcript_bam, out_bam, sort_by_coordinate != 0, write_index != 0, threads, dev, stats);
        return 0;
    PS_CATCH_INT
}

// The toolkit's `benchmark` mode (Main.java:489-521): ValidateBenchmarkStatisticsPARCLIP.calculateBenchmarkStatistics.
int ps_benchmark_reads(const char *mapping_sam_or_bam, const char *out_statistics, const char *reads_fq, ps_benchmark_stats *stats)
{
    PS_TRY
        const int dev = first_device();
        benchmark_run(mapping_sam_or_bam, out_statistics, reads_fq, dev, stats);
        return 0;
    PS_CATCH_INT
}

// The toolkit's `simulate` mode (Main.java:684-802): bin/createSimulatedPARCLIPDataset.pl.  The five files are renamed together.
int ps_simulate_reads(const ps_simulate_opts *opts, ps_simulate_stats *stats)
{
    PS_TRY
        if (!opts) throw Error("ps_simulate_reads: opts is NULL");
        const int dev = first_device();
        simulate_run(*opts, dev, stats);
        return 0;
    PS_CATCH_INT
}

// The toolkit's `fetch` and `fetchBed` modes (Main.java:883-945): FetchSequencesForBindingSites / FetchSequencesForBEDFile.fetchSequences.
int ps_fetch_sequences(const char *ref_fa, const char *sites, const char *out_file, int bed, ps_fetch_stats *stats)
{
    PS_TRY
        const int dev = first_device();
        fetch_run(ref_fa, sites, out_file, bed != 0, dev, stats);
        return 0;
    PS_CATCH_INT
}

int ps_bgzf_device(int device)
{
    PS_TRY
        bgzf_set_device(device < 0 ? -1 : device);
        return 0;
    PS_CATCH_INT
}
int ps_bgzf_compress(const void *src, uint64_t n, int device, void *dst, uint64_t cap, ps_bgzf_stats *stats)
{
    PS_TRY
        if (stats && stats->struct_size < sizeof(ps_bgzf_stats)) throw Error("ps_bgzf_compress: stats->struct_size is not sizeof(ps_bgzf_stats)");
        if (n && (!src || !dst)) throw Error("ps_bgzf_compress: source and destination are required");
        std::vector<BgzfSpan> spans;
        bgzf_cut((const char *)src, (size_t)n, spans);
        std::vector<std::string> comp(spans.size());
        BgzfStats s;
        if (device >= 0) bgzf_device_compress(spans.data(), spans.size(), device, comp.data(), &s);
        else {                                      // the library's host path on the same cuts: zlib at PS_BAM_LEVEL (1) on 16 threads
            int level = 1;
            if (const char *e = std::getenv("PS_BAM_LEVEL")) level = std::atoi(e);
            bgzf_host_compress(spans.data(), spans.size(), level < 0 ? 0 : (level > 9 ? 9 : level), 16, comp.data());
            for (size_t k = 0; k < comp.size(); ++k) {
                const int btype = ((unsigned char)comp[k][18] >> 1) & 3;        // of the member's first DEFLATE block
                ++s.n_blocks; s.n_stored += btype == 0; s.n_fixed += btype == 1; s.n_dynamic += btype == 2;
                s.in_bytes += spans[k].n; s.out_bytes += comp[k].size();
            }
        }
        if (s.out_bytes > cap) throw Error("ps_bgzf_compress: the members take " + std::to_string(s.out_bytes) + " bytes, the destination holds " + std::to_string(cap));
        char *o = (char *)dst;
        for (const std::string &c : comp) { std::memcpy(o, c.data(), c.size()); o += c.size(); }
        if (stats) {
            stats->n_blocks = s.n_blocks; stats->n_stored = s.n_stored; stats->n_fixed = s.n_fixed; stats->n_dynamic = s.n_dynamic; stats->pad_ = 0;
            stats->in_bytes = s.in_bytes; stats->out_bytes = s.out_bytes; stats->kernel_ms = s.kernel_ms;
        }
        return 0;
    PS_CATCH_INT
}
int ps_bam_records_device(int on) { PS_TRY bam_records_device_set(on != 0); return 0; PS_CATCH_INT }
int ps_bam_records_info(ps_bam_records_stats *out)
{
    PS_TRY
        if (!out) throw Error("ps_bam_records_info: no place for the result");
        bam_records_info(*out); return 0;
    PS_CATCH_INT
}
int64_t ps_batch_bam_records(ps_batch *b, int min_mapq, int on_device, int threads, void *dst, uint64_t cap, uint8_t *origin, ps_bam_records_stats *stats)
{
    try {
        Batch &B = *b->b;
        if (threads < 1) threads = 1;
        ps_bam_records_stats st; std::memset(&st, 0, sizeof st);
        st.n_reads = (uint64_t)B.rs.n;
        auto room = [&](uint64_t need) {
            if (dst && need > cap) throw Error("ps_batch_bam_records: the records take " + std::to_string(need) + " bytes, the destination holds " + std::to_string(cap));
        };
        if (on_device) {
            require_device(B.ctx->device);
            DevRecords r;
            batch_bam_records_device(B, min_mapq, threads, r);
            room(r.n_bytes);
            st.n_records = r.recs.size(); st.n_device = r.n_device; st.n_host = r.n_host; st.bytes = r.n_bytes;
            st.ms_upload = r.ms_upload; st.ms_kernels = r.ms_kernels; st.ms_host_records = r.ms_host_records; st.ms_download = r.ms_download;
            if (dst && r.n_bytes) std::memcpy(dst, r.bytes, r.n_bytes);
            if (dst && origin && !r.origin.empty()) std::memcpy(origin, r.origin.data(), r.origin.size());
        } else {
            std::vector<std::string> enc; std::vector<std::vector<BamRec>> recs;
            const auto t0 = std::chrono::steady_clock::now();
            batch_bam_records(B, min_mapq, threads, enc, recs);
            st.ms_host_records = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (size_t k = 0; k < enc.size(); ++k) { st.bytes += enc[k].size(); st.n_records += recs[k].size(); }
            st.n_host = st.n_records;
            room(st.bytes);
            char *o = (char *)dst;
            if (dst) for (const std::string &e : enc) { std::memcpy(o, e.data(), e.size()); o += e.size(); }
            if (dst && origin) std::memset(origin, 1, (size_t)st.n_records);
        }
        if (stats) *stats = st;
        return (int64_t)st.bytes;
    } catch (const std::exception &e) { fail(e.what()); return -1; } catch (...) { fail("unknown error"); return -1; }
}
}  // extern "C"
static const char *stats_name(const ps_bam_sort_stats *) { return "ps_bam_sort_stats"; }
static const char *stats_name(const ps_bam_name_sort_stats *) { return "ps_bam_name_sort_stats"; }
static void put(ps_bam_sort_stats *o, const BamSortStats &s)
{
    if (!o) return;
    o->on_device = s.on_device; o->n_records = s.n_records; o->bytes = s.bytes; o->n_calls_device = s.n_calls_device; o->n_calls_host = s.n_calls_host;
    o->n_resident = s.n_resident; o->ms_upload = s.ms_upload; o->ms_sort = s.ms_sort; o->ms_gather = s.ms_gather; o->ms_download = s.ms_download;
}
static void put(ps_bam_name_sort_stats *o, const BamNameSortStats &s)
{
    if (!o) return;
    o->on_device = s.on_device; o->n_records = s.n_records; o->bytes = s.bytes; o->n_calls_device = s.n_calls_device; o->n_calls_host = s.n_calls_host;
    o->n_resident = s.n_resident; o->key_words = s.key_words; o->pad_ = 0; o->n_passes = s.n_passes;
    o->ms_upload = s.ms_upload; o->ms_keys = s.ms_keys; o->ms_sort = s.ms_sort; o->ms_gather = s.ms_gather; o->ms_download = s.ms_download;
}
// The two orders' entries are one body: `who` is the entry's name in every message, Out / Stats the public struct and the library's,
// check the look at every scanned record that the order asks for (null: none; it returns what is wrong with the record), run and
// host the device route and the host route.
template <class Out, class Stats> static int sort_info(const char *who, Out *out, void (*info)(Stats &))
{
    PS_TRY
        if (!out) throw Error(std::string(who) + ": no place for the result");
        Stats s; info(s);
        out->struct_size = sizeof(Out); put(out, s); return 0;
    PS_CATCH_INT
}
template <class Out, class Stats>
static int64_t sort_records_entry(const char *who, const void *records, uint64_t n_bytes, int device, int threads, void *dst, uint64_t cap, Out *stats,
                                  const char *(*check)(const uint8_t *rec, size_t len), bool (*run)(BamSortJob &, int, Stats *), void (*host)(const char *, std::vector<BamRec> &, int, char *))
{
    try {
        const std::string name = std::string(who) + ": ";
        if (stats && stats->struct_size < sizeof(Out)) throw Error(name + "stats->struct_size is not sizeof(" + stats_name(stats) + ")");
        Stats st;
        if (n_bytes == 0) { put(stats, st); return 0; }
        if (!records || !dst) throw Error(name + "records and destination are required");
        std::vector<BamRec> recs;
        try { scan_records((const char *)records, n_bytes, recs); } catch (const Error &e) { throw Error(name + e.what()); }
        for (size_t i = 0; check && i < recs.size(); ++i)
            if (const char *why = check((const uint8_t *)records + recs[i].off, recs[i].len)) throw Error(name + "record " + std::to_string(i + 1) + " " + why);
        if (n_bytes > cap) throw Error(name + "the records take " + std::to_string(n_bytes) + " bytes, the destination holds " + std::to_string(cap));
        if (device >= 0) {
            require_device(device);
            const BgzfSpan part{(const char *)records, (size_t)n_bytes};
            std::vector<uint32_t> perm; BamBody body;
            BamSortJob job{&part, 1, recs.data(), recs.size(), &perm, &body};
            if (!run(job, device, &st)) throw Error(name + "the records need more device memory than PS_BAM_SORT_MAX_MB allows, or there are 2^32 of them or more");
            if (body.host.size() != n_bytes) throw Error(name + "the sorted stream has not the records' size");
            std::memcpy(dst, body.host.data(), body.host.size());
        } else {
            const auto t0 = std::chrono::steady_clock::now();
            host((const char *)records, recs, threads, (char *)dst);                    // nothing in it fails once the records are scanned
            st.ms_sort = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            st.n_calls_host = 1; st.n_records = recs.size(); st.bytes = n_bytes;
        }
        put(stats, st);
        return (int64_t)n_bytes;
    } catch (const std::exception &e) { fail(e.what()); return -1; } catch (...) { fail("unknown error"); return -1; }
}
static const char *name_check(const uint8_t *rec, size_t len) { return name_ends_inside(rec, len) ? nullptr : "has a name that does not end inside it"; }
extern "C" {
int ps_bam_sort_device(int device) { PS_TRY bam_sort_set_device(device < 0 ? -1 : device); return 0; PS_CATCH_INT }
int ps_bam_sort_info(ps_bam_sort_stats *out) { return sort_info("ps_bam_sort_info", out, &bam_sort_info); }
int64_t ps_bam_sort_records(const void *records, uint64_t n_bytes, int device, int threads, void *dst, uint64_t cap, ps_bam_sort_stats *stats)
{
    return sort_records_entry("ps_bam_sort_records", records, n_bytes, device, threads, dst, cap, stats, nullptr, &bam_sort_device_run, &sort_records_host);
}
int ps_bam_name_sort_device(int device) { PS_TRY bam_name_sort_set_device(device < 0 ? -1 : device); return 0; PS_CATCH_INT }
int ps_bam_name_sort_info(ps_bam_name_sort_stats *out) { return sort_info("ps_bam_name_sort_info", out, &bam_name_sort_info); }
int64_t ps_bam_name_sort_records(const void *records, uint64_t n_bytes, int device, int threads, void *dst, uint64_t cap, ps_bam_name_sort_stats *stats)
{
    return sort_records_entry("ps_bam_name_sort_records", records, n_bytes, device, threads, dst, cap, stats, &name_check, &bam_name_sort_device_run, &sort_records_host_by_name);
}
int ps_sam_to_bam(const char *sam, const char *bam, int min_mapq, int sort_by_coordinate, int write_index, int threads, ps_bam_stats *st)
{
    PS_TRY
        BamStats s;
        sam_to_bam(sam, bam, min_mapq, sort_by_coordinate != 0, write_index != 0, threads, &s);
        put(st, s);
        return 0;
    PS_CATCH_INT
}

int ps_bam_view(const char *in_bam, const char *out_bam, int min_mapq, int threads, ps_bam_stats *st)
{
    PS_TRY
        BamStats s; bam_view(in_bam, out_bam, min_mapq, threads, &s);
        put(st, s);
        return 0;
    PS_CATCH_INT
}
int ps_bam_sort(const char *in_bam, const char *out_bam, int by_name, int threads, ps_bam_stats *st)
{
    PS_TRY
        BamStats s; bam_sort(in_bam, out_bam, by_name != 0, threads, &s);
        put(st, s);
        return 0;
    PS_CATCH_INT
}
int ps_bam_index(const char *bam, int threads)
{
    PS_TRY
        bam_index(bam, threads); return 0;
    PS_CATCH_INT
}

}  // extern "C"
