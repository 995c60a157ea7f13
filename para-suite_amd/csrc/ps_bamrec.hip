// ps_bamrec.hip -- the BAM records of a located batch built on the device that mapped it (ps_bam_records_device, PS_BAM_RECORDS_GPU).
//
// After batch_locate everything a record of a device-finished read needs is in HBM: d_sel, d_fin, the packed forward strand, the
// contig and hole tables; the reads (bases, qualities, names, in input order) go up once per batch.  k_bamrec_size: one lane per
// read, ps_bamrec.h's bamrec_size (0 below the MAPQ filter) and the record's key.  The reads the device does not finish
// (PS_CLS_HOST: several best intervals, XA lists, larger tiers) keep the one resolver they have: the host builds their records with
// bam_record() while the size kernel runs, uploads bytes and lengths, and k_bamrec_splice puts the lengths in place.  An exclusive
// sum over the sizes gives every record its offset; k_bamrec_fill builds the records -- one wave per 64 consecutive reads, whose
// records are one contiguous byte range of the output: every lane fills its record into LDS, the wave copies the range out in
// aligned 16-byte stores.  The stream comes down once, in input order, into page-locked memory; the host walks the offsets for the
// BamRec array.  Every loop in the kernels is bounded by a read length, a CIGAR count, a name length, a table size or the 64
// lanes of the wave; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include "ps_bamrec.h"
#include "ps_dev.h"
#include "ps_par.h"
#include "ps_pipeline.h"

namespace ps {

// LDS staging of one wave of k_bamrec_fill: 64 records of a 50-base read take ~12 KB, of a 101-base read ~19 KB; six workgroups fit
// a CU's 160 KB.  A group of 64 whose range is longer is built in sub-groups of lanes that fit.
static const uint32_t BAMREC_STAGE = 24576;
static_assert(BAMREC_STAGE % 16 == 0 && 2 * BAMREC_STAGE <= 160 * 1024, "k_bamrec_fill: at least two workgroups per CU");

// A gapped hit after the banded alignment and the CIGAR clean-up of batch_locate.  That clean-up runs on the host and patches the host
// copy of the hit only (h_fin): a leading deletion is dropped and moves the position forward, an empty CIGAR makes the read unmapped.
// d_fin still holds the values from before, so the table carries the patched position and type next to the CIGAR.
struct BamrecCigar { int64_t pos; int32_t n, type; };

struct BamrecArgs {
    int64_t n; int32_t min_mapq;
    const uint8_t *cls; const SelRec *sel; const FinRec *fin;
    const uint8_t *seq; const int64_t *off; const int32_t *len; const char *qual; const char *names; const int64_t *name_off;
    const int32_t *cig_idx; const BamrecCigar *cig; const uint32_t *cig_words;   // per read: entry of the CIGAR table, -1 none
    const uint8_t *pac; int64_t l_pac;
    const int64_t *contig_off; const int32_t *contig_len; int32_t n_contigs;
    const int64_t *hole_off; const int32_t *hole_len; int32_t n_holes;
    int32_t max_top2;
    const int64_t *sub_g; int64_t n_sub; const uint64_t *sub_off; const uint32_t *sub_len; const int4 *sub_key; const uint8_t *sub_bytes;   // host-built records
    uint64_t *sizes; const uint64_t *offs; int4 *keys; uint8_t *out;
};

// the hit of read g as Batch::hit_of assembles it for a device-finished read
__device__ __forceinline__ void bamrec_input(const BamrecArgs &a, int64_t g, RecIn &r)
{
    const SelRec s = a.sel[g]; const FinRec f = a.fin[g];
    const int64_t n0 = a.name_off[g], o0 = a.off[g];
    r.name = a.names + n0; r.name_len = (uint32_t)(a.name_off[g + 1] - n0);
    r.seq = a.seq + o0; r.qual = a.qual ? a.qual + o0 : nullptr; r.len = a.len[g];
    int32_t type = f.type; int64_t pos = f.pos;
    r.cigar = nullptr; r.n_cigar = 0;
    const int32_t k = a.cig_idx[g];
    if (k >= 0) {                                  // a hit that went through the banded alignment: position and type as the host patched them
        const BamrecCigar c = a.cig[k];
        type = c.type; pos = c.pos;
        if (s.n_gapo && s.type) { r.cigar = a.cig_words + (size_t)k * PS_HIT_CIGAR; r.n_cigar = c.n; }
    }
    r.type = type; r.pos = type ? pos : -1; r.strand = f.strand; r.mapq = f.mapq;
    r.n_mm = s.n_mm; r.n_gapo = s.n_gapo; r.n_gape = s.n_gape; r.c1 = s.c1; r.c2 = s.c2;
    r.pac = a.pac; r.l_pac = a.l_pac;
    r.contig_off = a.contig_off; r.contig_len = a.contig_len; r.n_contigs = a.n_contigs;
    r.hole_off = a.hole_off; r.hole_len = a.hole_len; r.n_holes = a.n_holes; r.max_top2 = a.max_top2;
}

__global__ __launch_bounds__(256) void k_bamrec_size(BamrecArgs a)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.n) return;
    if (a.cls[g] & PS_CLS_HOST) { a.sizes[g] = 0; a.keys[g] = make_int4(-1, -1, 0, 4); return; }      // k_bamrec_splice puts the host's in
    RecIn r; bamrec_input(a, g, r);
    RecKey k; bamrec_key(r, k);
    a.sizes[g] = k.mapq < a.min_mapq ? 0u : bamrec_size(r);
    a.keys[g] = make_int4(k.ref, k.pos, k.end, (int)k.flag);
}

__global__ __launch_bounds__(256) void k_bamrec_splice(BamrecArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_sub) return;
    const int64_t g = a.sub_g[i];
    if (g < 0 || g >= a.n) return;
    a.sizes[g] = a.sub_len[i]; a.keys[g] = a.sub_key[i];
}

// one wave (= one workgroup) per 64 consecutive reads; offs: n + 1 entries, the exclusive sum of sizes
__global__ __launch_bounds__(64) void k_bamrec_fill(BamrecArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[BAMREC_STAGE];
    const int lane = (int)threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * 64;
    if (g0 >= a.n) return;
    const int cnt = (int)(a.n - g0 < 64 ? a.n - g0 : 64);
    const int64_t g = g0 + (lane < cnt ? lane : cnt - 1);
    const uint64_t o0 = a.offs[g], o1 = lane < cnt ? a.offs[g + 1] : o0;        // this lane's record: [o0, o1) of the output
    int s = 0;
    while (s < cnt) {                                                          // sub-groups [s, e) of lanes: every pass takes at least one lane
        const uint64_t beg = a.offs[g0 + s], beg_al = beg & ~(uint64_t)15;    // LDS byte x stands for output byte beg_al + x
        const bool fits = lane >= s && lane < cnt && o1 - beg_al <= BAMREC_STAGE;
        int e = s + __popcll(__ballot(fits));                                  // offsets rise with the lane: the lanes that fit are a run from s
        const bool direct = e == s;                                            // a single record larger than the staging: straight to global memory.  Defensive: with reads of at most PS_MAX_LEN bases and names of at most 254 no record reaches 2 KB, so no input takes this branch today
        if (direct) e = s + 1;
        if (lane >= s && lane < e && o1 > o0) {
            uint8_t *dst = direct ? a.out + o0 : stage + (o0 - beg_al);
            if (a.cls[g] & PS_CLS_HOST) {                                      // host-built: its entry by bisection over the table, its bytes copied
                int64_t lo = 0, hi = a.n_sub;
                while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (a.sub_g[mid] <= g) lo = mid; else hi = mid; }
                const uint8_t *src = a.sub_bytes + a.sub_off[lo];
                const uint32_t n = a.sub_g[lo] == g ? a.sub_len[lo] : 0u;
                for (uint32_t j = 0; j < n && j < (uint32_t)(o1 - o0); ++j) dst[j] = src[j];
            } else { RecIn r; bamrec_input(a, g, r); bamrec_fill(r, dst); }
        }
        if (!direct) {
            __syncthreads();
            const uint64_t end = a.offs[g0 + e];
            const uint32_t n_units = (uint32_t)((end - beg_al + 15) >> 4);    // <= BAMREC_STAGE / 16: end - beg_al <= BAMREC_STAGE
            for (uint32_t u = (uint32_t)lane; u < n_units; u += 64) {
                const uint64_t at = beg_al + ((uint64_t)u << 4);
                if (at >= beg && at + 16 <= end) *reinterpret_cast<uint4 *>(a.out + at) = *reinterpret_cast<const uint4 *>(stage + ((size_t)u << 4));
                else for (uint32_t j = 0; j < 16; ++j) if (at + j >= beg && at + j < end) a.out[at + j] = stage[((size_t)u << 4) + j];   // a unit shared with a neighbouring range
            }
            __syncthreads();
        }
        s = e;
    }
}

namespace {

std::atomic<bool> g_on{false};
struct Totals { std::mutex mu; ps_bam_records_stats s; };
Totals &totals() { static Totals *t = [] { Totals *x = new Totals(); std::memset(&x->s, 0, sizeof x->s); return x; }(); return *t; }
[[maybe_unused]] const bool g_env_read = [] { const char *e = std::getenv("PS_BAM_RECORDS_GPU"); if (e && std::atoi(e) > 0) g_on = true; return true; }();

const RefTables &tables_of(Ctx &c, hipStream_t s)
{
    std::lock_guard<std::mutex> l(c.work_mu);
    if (!c.rec_tables) c.rec_tables = std::make_shared<RefTables>(c.ix, s);
    return *static_cast<const RefTables *>(c.rec_tables.get());
}
// src[0, n) through page-locked staging of the lane into its (grow-only) device buffer
template <class T> T *stage_up(Work &wk, const std::string &name, const T *src, size_t n, int threads, hipStream_t s)
{
    T *h = wk.pin_get<T>("bamrec_h_" + name, std::max<size_t>(1, n)), *d = wk.ws_get<T>("bamrec_" + name, std::max<size_t>(1, n));
    par_for(n * sizeof(T), threads, [&](size_t a0, size_t a1, int) { std::memcpy((char *)h + a0, (const char *)src + a0, a1 - a0); });
    if (n) PS_HIP(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}

}  // namespace

bool bam_records_device_on() { return g_on; }
void bam_records_device_set(bool on) { Totals &t = totals(); std::lock_guard<std::mutex> l(t.mu); g_on = on; std::memset(&t.s, 0, sizeof t.s); }
void bam_records_info(ps_bam_records_stats &out) { Totals &t = totals(); std::lock_guard<std::mutex> l(t.mu); out = t.s; }
void bam_records_count(const ps_bam_records_stats &x)
{
    Totals &t = totals(); std::lock_guard<std::mutex> l(t.mu);
    t.s.n_reads += x.n_reads; t.s.n_records += x.n_records; t.s.n_device += x.n_device; t.s.n_host += x.n_host; t.s.bytes += x.bytes;
    t.s.ms_upload += x.ms_upload; t.s.ms_kernels += x.ms_kernels; t.s.ms_host_records += x.ms_host_records; t.s.ms_download += x.ms_download;
}

void batch_bam_records_device(Batch &b, int min_mapq, int threads, DevRecords &out)
{
    if (!b.located) throw Error("BAM records before locate");
    const ReadSet &rs = b.rs; const int64_t N = rs.n;
    out.bytes = nullptr; out.n_bytes = 0; out.recs.clear(); out.origin.clear();
    out.n_reads = (uint64_t)N; out.n_device = out.n_host = 0; out.ms_upload = out.ms_kernels = out.ms_host_records = out.ms_download = 0;
    if (N == 0) return;
    if (!b.wk || !b.d_sel.p || !b.d_fin.p || !b.d_class.p) throw Error("BAM records on the device: the batch has given its device records back");
    if (N >= 0x7fffffff) throw Error("BAM records on the device: too many reads in one batch");
    for (int64_t g = 0; g < N; ++g) if (rs.name_off[g + 1] - rs.name_off[g] > 254) throw Error("read name longer than 254 characters");
    if (threads < 1) threads = 1;
    Ctx &c = *b.ctx; Work &wk = *b.wk; hipStream_t s = wk.stream;
    const RefTables &rt = tables_of(c, s);
    EventPair ev_up, ev_k1, ev_k2, ev_k3, ev_down;

    // ---- the reads and the gapped hits' CIGARs go up
    ev_up.start(s);
    BamrecArgs a; std::memset(&a, 0, sizeof a);
    a.n = N; a.min_mapq = min_mapq; a.cls = b.d_class.p; a.sel = b.d_sel.p; a.fin = b.d_fin.p;
    const size_t n_bases = (size_t)rs.off[N], n_names = (size_t)rs.name_off[N];
    a.seq = stage_up(wk, "seq", rs.seq.data(), n_bases, threads, s);
    a.off = stage_up(wk, "off", rs.off.data(), (size_t)N + 1, threads, s);
    a.len = stage_up(wk, "len", rs.len.data(), (size_t)N, threads, s);
    a.qual = rs.has_qual ? stage_up(wk, "qual", rs.qual.data(), n_bases, threads, s) : nullptr;
    a.names = stage_up(wk, "names", rs.names.data(), n_names, threads, s);
    a.name_off = stage_up(wk, "name_off", rs.name_off.data(), (size_t)N + 1, threads, s);
    {
        const size_t K = b.dev_cigars.size();
        int32_t *h_idx = wk.pin_get<int32_t>("bamrec_h_cig_idx", (size_t)N); BamrecCigar *h_n = wk.pin_get<BamrecCigar>("bamrec_h_cig", std::max<size_t>(1, K));
        uint32_t *h_w = wk.pin_get<uint32_t>("bamrec_h_cig_words", std::max<size_t>(1, K * PS_HIT_CIGAR));
        par_for((size_t)N, threads, [&](size_t g0, size_t g1, int) { for (size_t g = g0; g < g1; ++g) h_idx[g] = -1; });
        for (size_t k = 0; k < K; ++k) {
            const DevCigar &dc = b.dev_cigars[k];
            if (dc.g < 0 || dc.g >= N || dc.n < 0 || dc.n > PS_HIT_CIGAR) throw Error("BAM records on the device: a CIGAR outside its table");
            h_idx[dc.g] = (int32_t)k; h_n[k] = BamrecCigar{b.h_fin[dc.g].pos, dc.n, (int32_t)b.h_fin[dc.g].type}; std::memcpy(h_w + k * PS_HIT_CIGAR, dc.c, sizeof dc.c);
        }
        int32_t *d_idx = wk.ws_get<int32_t>("bamrec_cig_idx", (size_t)N); BamrecCigar *d_n = wk.ws_get<BamrecCigar>("bamrec_cig", std::max<size_t>(1, K));
        uint32_t *d_w = wk.ws_get<uint32_t>("bamrec_cig_words", std::max<size_t>(1, K * PS_HIT_CIGAR));
        PS_HIP(hipMemcpyAsync(d_idx, h_idx, (size_t)N * 4, hipMemcpyHostToDevice, s));
        if (K) { PS_HIP(hipMemcpyAsync(d_n, h_n, K * sizeof(BamrecCigar), hipMemcpyHostToDevice, s)); PS_HIP(hipMemcpyAsync(d_w, h_w, K * PS_HIT_CIGAR * 4, hipMemcpyHostToDevice, s)); }
        a.cig_idx = d_idx; a.cig = d_n; a.cig_words = d_w;
    }
    ev_up.stop(s);
    a.pac = c.ix.pac.p; a.l_pac = c.ix.ref.l_pac;
    a.contig_off = rt.contig_off.p; a.contig_len = rt.contig_len.p; a.n_contigs = (int32_t)c.ix.ref.contigs.size();
    a.hole_off = rt.hole_off.p; a.hole_len = rt.hole_len.p; a.n_holes = rt.n_holes; a.max_top2 = c.opt.max_top2;
    uint64_t *d_sizes = wk.ws_get<uint64_t>("bamrec_sizes", (size_t)N + 1), *d_offs = wk.ws_get<uint64_t>("bamrec_offs", (size_t)N + 1);
    a.sizes = d_sizes; a.offs = d_offs; a.keys = wk.ws_get<int4>("bamrec_keys", (size_t)N);
    PS_HIP(hipMemsetAsync(d_sizes + N, 0, sizeof(uint64_t), s));

    // ---- sizes on the device; meanwhile the host builds the records of the reads it finished itself
    ev_k1.start(s);
    hipLaunchKernelGGL(k_bamrec_size, dim3(blocks_for((size_t)N)), dim3(256), 0, s, a);
    PS_HIP(hipGetLastError());
    ev_k1.stop(s);
    const HostClock::time_point t_host = HostClock::now();
    std::vector<std::string> enc; std::vector<BamRec> srecs;
    batch_bam_records_sub(b, min_mapq, threads, enc, srecs);
    out.ms_host_records = ms_since(t_host);
    const size_t M = srecs.size();
    const HostClock::time_point t_up2 = HostClock::now();
    if (M) {
        std::vector<uint64_t> base(enc.size() + 1, 0);
        for (size_t t = 0; t < enc.size(); ++t) base[t + 1] = base[t] + enc[t].size();
        int64_t *h_g = wk.pin_get<int64_t>("bamrec_h_sub_g", M); uint64_t *h_off = wk.pin_get<uint64_t>("bamrec_h_sub_off", M);
        uint32_t *h_len = wk.pin_get<uint32_t>("bamrec_h_sub_len", M); int4 *h_key = wk.pin_get<int4>("bamrec_h_sub_key", M);
        uint8_t *h_bytes = wk.pin_get<uint8_t>("bamrec_h_sub_bytes", std::max<size_t>(1, (size_t)base.back()));
        for (size_t i = 0; i < M; ++i) {
            const BamRec &r = srecs[i];
            h_g[i] = b.sub[i].g; h_off[i] = base[(size_t)r.part] + r.off; h_len[i] = (uint32_t)r.len; h_key[i] = make_int4(r.ref, r.pos, r.end, (int)r.flag);
        }
        for (size_t t = 0; t < enc.size(); ++t) if (!enc[t].empty()) std::memcpy(h_bytes + base[t], enc[t].data(), enc[t].size());
        int64_t *d_g = wk.ws_get<int64_t>("bamrec_sub_g", M); uint64_t *d_off = wk.ws_get<uint64_t>("bamrec_sub_off", M);
        uint32_t *d_len = wk.ws_get<uint32_t>("bamrec_sub_len", M); int4 *d_key = wk.ws_get<int4>("bamrec_sub_key", M);
        uint8_t *d_bytes = wk.ws_get<uint8_t>("bamrec_sub_bytes", std::max<size_t>(1, (size_t)base.back()));
        PS_HIP(hipMemcpyAsync(d_g, h_g, M * 8, hipMemcpyHostToDevice, s)); PS_HIP(hipMemcpyAsync(d_off, h_off, M * 8, hipMemcpyHostToDevice, s));
        PS_HIP(hipMemcpyAsync(d_len, h_len, M * 4, hipMemcpyHostToDevice, s)); PS_HIP(hipMemcpyAsync(d_key, h_key, M * sizeof(int4), hipMemcpyHostToDevice, s));
        if (base.back()) PS_HIP(hipMemcpyAsync(d_bytes, h_bytes, (size_t)base.back(), hipMemcpyHostToDevice, s));
        a.sub_g = d_g; a.n_sub = (int64_t)M; a.sub_off = d_off; a.sub_len = d_len; a.sub_key = d_key; a.sub_bytes = d_bytes;
    }
    ev_k2.start(s);
    if (M) { hipLaunchKernelGGL(k_bamrec_splice, dim3(blocks_for(M)), dim3(256), 0, s, a); PS_HIP(hipGetLastError()); }
    const double ms_stage2 = ms_since(t_up2);

    // ---- offsets, the total, the fill
    cub_call(s, [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, d_sizes, d_offs, (int)(N + 1), s); });
    uint64_t *h_offs = wk.pin_get<uint64_t>("bamrec_h_offs", (size_t)N + 1);
    ev_k2.stop(s);
    PS_HIP(hipMemcpyAsync(h_offs + N, d_offs + N, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    const size_t total = (size_t)h_offs[N];
    a.out = wk.ws_get<uint8_t>("bamrec_out", total + 32);
    uint8_t *h_out = (uint8_t *)out.pin.get(total + 32);
    ev_k3.start(s);
    hipLaunchKernelGGL(k_bamrec_fill, dim3((unsigned)(((size_t)N + 63) / 64)), dim3(64), 0, s, a);
    PS_HIP(hipGetLastError());
    ev_k3.stop(s);

    // ---- the stream, the offsets and the keys come down; the host walks the offsets for the kept records
    int4 *h_keys = wk.pin_get<int4>("bamrec_h_keys", (size_t)N);
    ev_down.start(s);
    if (total) PS_HIP(hipMemcpyAsync(h_out, a.out, total, hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(h_offs, d_offs, ((size_t)N + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(h_keys, a.keys, (size_t)N * sizeof(int4), hipMemcpyDeviceToHost, s));
    ev_down.stop(s);
    PS_HIP(hipStreamSynchronize(s));
    const HostClock::time_point t_walk = HostClock::now();
    size_t kept = 0;
    for (int64_t g = 0; g < N; ++g) kept += h_offs[g + 1] > h_offs[g];
    out.recs.reserve(kept); out.origin.reserve(kept);
    for (int64_t g = 0; g < N; ++g) {
        const size_t len = (size_t)(h_offs[g + 1] - h_offs[g]);
        if (!len) continue;
        const int4 k = h_keys[g];
        out.recs.push_back(BamRec{k.x, k.y, k.z, (uint32_t)k.w, (size_t)h_offs[g], len, 0});
        const bool host = (b.h_class[g] & PS_CLS_HOST) != 0;
        out.origin.push_back(host ? 1 : 0); out.n_host += host; out.n_device += !host;
    }
    const double ms_walk = ms_since(t_walk);
    out.bytes = h_out; out.n_bytes = total;
    // the stream from the first staging copy to the last upload's end (the host's staging lies inside), then the host-built records' staging
    out.ms_upload = ev_up.ms() + ms_stage2;
    out.ms_kernels = ev_k1.ms() + ev_k2.ms() + ev_k3.ms(); out.ms_download = ev_down.ms() + ms_walk;
    ps_bam_records_stats st; std::memset(&st, 0, sizeof st);
    st.n_reads = (uint64_t)N; st.n_records = kept; st.n_device = out.n_device; st.n_host = out.n_host; st.bytes = total;
    st.ms_upload = out.ms_upload; st.ms_kernels = out.ms_kernels; st.ms_host_records = out.ms_host_records; st.ms_download = out.ms_download;
    bam_records_count(st);
    static const bool verbose = std::getenv("PS_VERBOSE") != nullptr && std::atoi(std::getenv("PS_VERBOSE")) >= 2;
    if (verbose)
        std::fprintf(stderr, "[parasuite-hip]     BAM records of %lld reads on device %d: %zu records, %.1f MB (%llu built by the host on %d threads); upload %.1f ms, kernels %.1f ms (size %.1f, fill %.1f), "
                             "host-built records %.1f ms, download %.1f ms (of it %.1f walking the offsets)\n", (long long)N, c.device, kept, total / 1e6, (unsigned long long)out.n_host, threads,
                     out.ms_upload, out.ms_kernels, ev_k1.ms(), ev_k3.ms(), out.ms_host_records, out.ms_download, ms_walk);
}

}  // namespace ps
