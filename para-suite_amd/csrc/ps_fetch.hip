// ps_fetch.hip -- the reference sequence of every site of a table: the toolkit's `fetch` and `fetchBed` modes
// (include/parasuite_hip.h, ps_fetch_sequences).
//
// Replaces utils.pileupclusters.FetchSequencesForBindingSites.fetchSequences and FetchSequencesForBEDFile.fetchSequences (the
// toolkit's src/utils/pileupclusters/FetchSequencesForBindingSites.java:18-95, FetchSequencesForBEDFile.java:17-99): one thread,
// one IndexedFastaSequenceFile.getSubsequenceAt per site, which needs a .fai beside the FASTA.  Here the bases come from the
// index's packed forward strand and its hole table (.pac, .ann): both classes upper-case what they fetch (:64-68), so the case
// of a, c, g and t -- all the index drops of the FASTA's graphic characters -- never reaches the output.
//   (host)          the lines of the sites file parsed on threads into a site table: contig, start, length (0 for a site left
//                   empty), reverse flag; the rules and where the Java dies are in the header
//   (hipCUB)        an exclusive scan of the lengths: every site's 64-bit offset into ONE flat stream of output bases
//   k_fetch_gather  flat over the bytes of that stream, not one lane per site (sites run from one base to a chromosome): a lane
//                   owns 16 consecutive bytes, finds the site of its first byte by bisection over the offsets -- the workgroup
//                   narrows that to the sites of its own 4 KiB first, and stages their offsets in LDS -- walks on into the next
//                   site or sites where its bytes cross a boundary, and writes its bytes with one 16-byte store
//   (host)          the stream is gathered in pieces (PS_FETCH_PIECE bytes, cut anywhere); the text of one piece is written
//                   while the next is gathered: two buffers, one stream each
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include "../../include/parasuite_hip.h"
#include "ps_dev.h"
#include "ps_java.h"
#include "ps_pacref.h"
#include "ps_par.h"
#include "ps_pipeline.h"

namespace ps {

constexpr unsigned kFetchLane = 16, kFetchBlock = 256, kFetchBlockBytes = kFetchLane * kFetchBlock;   // bytes per lane, lanes and bytes per workgroup
constexpr int kFetchStaged = 1024;                                      // offsets of at most this many sites go to LDS
constexpr size_t kFetchPiece = (size_t)256 << 20;                        // bytes of the stream per piece (PS_FETCH_PIECE overrides)
enum : int { kFtOk = 0, kFtInverted = 1, kFtNoContig = 2, kFtPastEnd = 3, kFtBeforeStart = 4 };   // why a site is empty: the first that applies

// n sites; off has n + 1 entries, the last the length of the stream.  Sites of length 0 share their offset with the next one.
struct FetchSites { int64_t n; const int32_t *contig, *start, *len; const uint8_t *rev; const uint64_t *off; };
struct FetchRef { const uint8_t *pac, *hole_chr; const int64_t *contig_off, *hole_off; const int32_t *hole_len; int n_holes; };

// the site in [lo, hi] that holds byte g of the stream: the last one whose offset is <= g (the one before it may be empty)
template <class Off> __device__ __forceinline__ int64_t fetch_site_of(const Off *off, int64_t lo, int64_t hi, uint64_t g)
{
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (off[mid] <= g) lo = mid; else hi = mid - 1; }
    return lo;
}

// bytes [base, end) of the stream -> out[0, end - base), rounded up to whole 16-byte stores (the buffer is that long; the bytes
// behind `end` are written as 0).  base is a multiple of 16.  Every lane reaches the shuffles: no lane returns early.
__global__ void __launch_bounds__(kFetchBlock) k_fetch_gather(FetchSites t, FetchRef r, uint64_t base, uint64_t end, uint8_t *out,
                                                              unsigned long long *n_hole_bases)
{
    __shared__ uint64_t s_off[kFetchStaged];
    __shared__ int64_t s_range[2];
    const uint64_t blk0 = base + (uint64_t)blockIdx.x * kFetchBlockBytes, blk1 = min(end, blk0 + kFetchBlockBytes);   // blk0 < end by the grid's size
    if (threadIdx.x < 2) s_range[threadIdx.x] = fetch_site_of(t.off, (int64_t)0, t.n - 1, threadIdx.x ? blk1 - 1 : blk0);
    __syncthreads();
    const int64_t lo = s_range[0], hi = s_range[1];                       // this workgroup's bytes lie in sites lo..hi
    const bool staged = hi - lo < kFetchStaged;                           // the same in every lane of the workgroup
    if (staged) {
        for (int64_t i = threadIdx.x; i <= hi - lo; i += kFetchBlock) s_off[i] = t.off[lo + i];
        __syncthreads();
    }
    const uint64_t g0 = blk0 + (uint64_t)threadIdx.x * kFetchLane, g1 = min(blk1, g0 + kFetchLane);
    uint32_t w[4] = {0, 0, 0, 0}; unsigned holes = 0;
    if (g0 < blk1) {
        int64_t s = staged ? lo + fetch_site_of(s_off, (int64_t)0, hi - lo, g0) : fetch_site_of(t.off, lo, hi, g0);
        ProfRef rf{r.pac, r.hole_off, r.hole_len, r.n_holes, 0};
        rf.hole_chr = r.hole_chr;
        uint64_t site_off = 0, site_end = 0; int64_t first = 0, last = 0; bool rev = false;
        // byte g lies in site s: where its bases are, and the hole cursor at the lowest base this lane reads of it
        auto enter = [&](uint64_t g) {
            const int32_t len = t.len[s];
            site_off = staged ? s_off[s - lo] : t.off[s]; site_end = site_off + (uint64_t)len;
            first = r.contig_off[t.contig[s]] + t.start[s] - 1; last = first + len - 1; rev = t.rev[s] != 0;
            rf.seek(rev ? last - (int64_t)(min(g1, site_end) - 1 - site_off) : first + (int64_t)(g - site_off));
        };
        enter(g0);
#pragma unroll
        for (unsigned k = 0; k < kFetchLane; ++k) {
            const uint64_t g = g0 + k;
            if (g < g1) {
                if (g >= site_end) {                                      // on into the next site that has bases
                    do ++s; while (t.len[s] == 0);
                    enter(g);
                }
                const int64_t j = (int64_t)(g - site_off);
                int c = rf.letter_at(rev ? last - j : first + j, rev);
                if (c < 0) { ++holes; c = -c; }
                w[k >> 2] |= (uint32_t)c << ((k & 3u) << 3);
            }
        }
        *reinterpret_cast<uint4 *>(out + (g0 - base)) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (int d = 32; d > 0; d >>= 1) holes += __shfl_down(holes, d, 64);
    if ((threadIdx.x & 63u) == 0u && holes) atomicAdd(n_hole_bases, (unsigned long long)holes);
}

namespace {

struct FetchWiden { __host__ __device__ uint64_t operator()(int32_t v) const { return (uint64_t)v; } };

// what the writer needs of a data line, as byte ranges of the sites file: fetch writes [a0, a1) sequence [b0, b1) "\n" (the line
// up to field 11, and what is kept behind it), fetchBed ">" [a0, a1) "\n" sequence "\n" (field 3)
struct FetchText { size_t a0, a1, b0, b1; };

struct FetchOutput {                   // the buffered text of the output, written where the call's OutFiles says
    const std::string tmp; FILE *f = nullptr; std::string buf;
    explicit FetchOutput(const std::string &path) : tmp(path)
    {
        f = std::fopen(tmp.c_str(), "wb");
        if (!f) throw Error("cannot write " + tmp);
        buf.reserve((size_t)5 << 20);
    }
    ~FetchOutput() { if (f) std::fclose(f); }
    void flush()
    {
        if (!buf.empty() && std::fwrite(buf.data(), 1, buf.size(), f) != buf.size()) throw Error("cannot write " + tmp);
        buf.clear();
    }
    void put(const void *p, size_t n) { buf.append((const char *)p, n); if (buf.size() >= ((size_t)4 << 20)) flush(); }
    void put(char c) { buf.push_back(c); }
    void close()
    {
        flush();
        const int rc = std::fclose(f); f = nullptr;
        if (rc != 0) throw Error("cannot write " + tmp);
    }
};

}  // namespace

void fetch_run(const char *ref_fa, const char *sites_path, const char *out_path, bool bed, int device, ps_fetch_stats *stats)
{
    using clk = HostClock;
    const std::string who = "ps_fetch_sequences: ";
    if (!ref_fa || !ref_fa[0] || !sites_path || !sites_path[0] || !out_path || !out_path[0])
        throw Error(who + "reference, sites file and output file are required");
    const std::string ref(ref_fa);
    OutFiles files(".fetch-tmp");
    const std::string tmp_name = files.add(out_path);
    files.refuse_inputs({sites_path, ref_fa, (ref + ".ann").c_str(), (ref + ".pac").c_str()}, who, " may not be one of the inputs: ");
    require_device(device);                                                // before the files are read
    const auto t_all = clk::now();
    ps_fetch_stats st{};

    // ---- the index: contigs and holes from .ann, the packed strand onto the device
    auto t0 = clk::now();
    StreamGuard sg0, sg1; hipStream_t s = sg0.s;
    Index ix;
    try { index_load_pac(ref, ix, s); } catch (const std::exception &e) { throw Error(who + e.what()); }
    RefTables rt(ix, s); RefHoleChars hc(ix, s);
    std::unordered_map<std::string, int32_t> contig_of;
    for (size_t c = 0; c < ix.ref.contigs.size(); ++c) contig_of.emplace(ix.ref.contigs[c].name, (int32_t)c);
    st.s_index = ms_since(t0) / 1e3;

    // ---- the sites file: lines, then every data line on its own
    t0 = clk::now();
    const std::string data = read_whole_file(sites_path);
    const char *d = data.data(); const size_t nd = data.size();
    std::vector<size_t> line_b, line_e;                                    // BufferedReader.readLine: "\n", "\r" or "\r\n"
    size_t next_lf = SIZE_MAX;
    for (size_t i = 0; i < nd;) {
        if (next_lf < i || next_lf == SIZE_MAX) { const char *lf = (const char *)std::memchr(d + i, '\n', nd - i); next_lf = lf ? (size_t)(lf - d) : nd; }
        size_t e = next_lf;                                               // looked for once per "\n", not once per line: a file of "\r" ends has none
        if (const char *cr = (const char *)std::memchr(d + i, '\r', e - i)) e = (size_t)(cr - d);
        line_b.push_back(i); line_e.push_back(e);
        i = e + (e + 1 < nd && d[e] == '\r' && d[e + 1] == '\n' ? 2 : 1);
    }
    if (line_b.empty()) throw Error(who + sites_path + " is empty: no header line");
    const size_t n = line_b.size() - 1;
    if (n >= (size_t)INT_MAX) throw Error(who + "more than 2^31 - 2 sites in " + sites_path);
    st.n_lines = line_b.size(); st.n_sites = n;

    const int threads = 8, min_fields = bed ? 5 : 12;
    std::vector<int32_t> contig(n + 1, 0), start(n + 1, 1), len(n + 1, 0); std::vector<uint8_t> rev(n + 1, 0), why(n, 0);   // entry n: the scan's total
    std::vector<FetchText> text(n);
    std::vector<size_t> bad_line(threads, SIZE_MAX); std::vector<std::string> bad_what(threads);
    par_for(n, threads, [&](size_t a, size_t b, int th) {
        std::string name;
        for (size_t i = a; i < b; ++i) {
            const size_t lb = line_b[i + 1], le = line_e[i + 1];
            size_t fb[12], fe[12], beg = lb, kept_end = lb; int f = 0, kept = 0;
            for (size_t k = lb; k <= le; ++k) {
                if (k < le && d[k] != '\t') continue;
                if (f < 12) { fb[f] = beg; fe[f] = k; }
                if (k > beg) { kept = f + 1; kept_end = k; }
                ++f; beg = k + 1;
            }
            auto fail = [&](const std::string &what) { bad_line[th] = i + 2; bad_what[th] = what; };
            if (kept < min_fields) { fail("has " + std::to_string(le == lb ? 1 : kept) + " TAB-separated fields, fewer than " + std::to_string(min_fields)); return; }
            const int fc = bed ? 0 : 1;                                   // contig, start and end follow each other; the strand is field 4 in both
            int32_t st_ = 0, en = 0;
            if (!java_parse_int((const uint8_t *)d + fb[fc + 1], (uint32_t)(fe[fc + 1] - fb[fc + 1]), st_)) { fail("start '" + std::string(d + fb[fc + 1], fe[fc + 1] - fb[fc + 1]) + "' is not an int"); return; }
            if (!java_parse_int((const uint8_t *)d + fb[fc + 2], (uint32_t)(fe[fc + 2] - fb[fc + 2]), en)) { fail("end '" + std::string(d + fb[fc + 2], fe[fc + 2] - fb[fc + 2]) + "' is not an int"); return; }
            rev[i] = fe[4] - fb[4] == 1 && d[fb[4]] == '-';
            text[i] = bed ? FetchText{fb[3], fe[3], le, le} : FetchText{lb, fb[11], fe[11], kept_end};
            name.assign(bed && !(fe[0] - fb[0] >= 3 && !std::memcmp(d + fb[0], "chr", 3)) ? "chr" : "");
            name.append(d + fb[fc], fe[fc] - fb[fc]);
            const auto it = contig_of.find(name);
            int reason = kFtOk;
            if (st_ > (int32_t)((uint32_t)en + 1u)) reason = kFtInverted;     // getSubsequenceAt's checks in its order; end + 1 as a Java int
            else if (it == contig_of.end()) reason = kFtNoContig;
            else if (en > ix.ref.contigs[(size_t)it->second].len) reason = kFtPastEnd;
            else if (st_ < 1) reason = kFtBeforeStart;                    // the library's rule: htsjdk would read bytes before the contig
            why[i] = (uint8_t)reason;
            if (reason == kFtOk) { contig[i] = it->second; start[i] = st_; len[i] = en - st_ + 1; }
        }
    });
    {
        size_t first = SIZE_MAX; int t_first = -1;
        for (int th = 0; th < threads; ++th) if (bad_line[th] < first) { first = bad_line[th]; t_first = th; }
        if (t_first >= 0) throw Error(who + "line " + std::to_string(first) + " of " + sites_path + " " + bad_what[t_first]);
    }
    for (size_t i = 0; i < n; ++i) {
        st.n_reverse += rev[i];
        st.n_inverted += why[i] == kFtInverted; st.n_no_contig += why[i] == kFtNoContig; st.n_past_end += why[i] == kFtPastEnd; st.n_before_start += why[i] == kFtBeforeStart;
    }
    st.s_read = ms_since(t0) / 1e3;

    // ---- the site table onto the device; offsets by an exclusive scan of the lengths (entry n: the length of the stream)
    double ms_kernels = 0;
    DevBuf<int32_t> d_contig, d_start, d_len; DevBuf<uint8_t> d_rev; DevBuf<uint64_t> d_off; DevBuf<unsigned long long> d_holes;
    upload(d_contig, contig, s); upload(d_start, start, s); upload(d_len, len, s); upload(d_rev, rev, s);
    d_off.alloc(n + 1); d_holes.alloc(1); d_holes.zero(s);
    {
        EventPair ev(s);
        hipcub::TransformInputIterator<uint64_t, FetchWiden, const int32_t *> in(d_len.p, FetchWiden());
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, in, d_off.p, (int)(n + 1), s); });
        ev.stop(s); ms_kernels += ev.ms();
    }
    std::vector<uint64_t> off(n + 1);
    d_off.download(off.data(), n + 1, s);
    PS_HIP(hipStreamSynchronize(s));
    const uint64_t total = off[n];
    st.n_bases = total;

    size_t piece = kFetchPiece;
    if (const char *e = std::getenv("PS_FETCH_PIECE")) piece = (size_t)std::max(1ll, std::atoll(e));   // tests: force many pieces
    piece = std::min((piece + kFetchLane - 1) / kFetchLane * kFetchLane, (size_t)1 << 32);
    const uint64_t n_pieces = total ? (total + piece - 1) / piece : 1;
    st.n_pieces = n_pieces;

    // ---- gather and write: piece k + 1 is on the device while the text of piece k is written
    double ms_write = 0;
    {
        const size_t cap = (size_t)((std::min<uint64_t>(piece, total) + kFetchLane - 1) / kFetchLane * kFetchLane) + kFetchLane;
        PinBuf pin[2]; DevBuf<uint8_t> dev[2]; EventPair ev[2];
        StreamGuard *lane[2] = {&sg0, &sg1};
        struct Drain { hipStream_t a, b; ~Drain() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); } } drain{sg0.s, sg1.s};   // before the buffers are let go
        const FetchSites ts{(int64_t)n, d_contig.p, d_start.p, d_len.p, d_rev.p, d_off.p};
        const FetchRef tr{ix.pac.p, hc.chr.p, rt.contig_off.p, rt.hole_off.p, rt.hole_len.p, rt.n_holes};
        auto gather = [&](uint64_t k) {
            const int slot = (int)(k & 1); hipStream_t q = lane[slot]->s;
            const uint64_t p0 = k * piece, p1 = std::min<uint64_t>(total, p0 + piece);
            if (p1 <= p0) return;                                         // the one piece of an empty stream
            if (!dev[slot].p) { dev[slot].alloc(cap); pin[slot].get(cap); }
            ev[slot].start(q);
            hipLaunchKernelGGL(k_fetch_gather, dim3((unsigned)((p1 - p0 + kFetchBlockBytes - 1) / kFetchBlockBytes)), dim3(kFetchBlock), 0, q,
                               ts, tr, p0, p1, dev[slot].p, d_holes.p);
            PS_HIP(hipGetLastError());
            ev[slot].stop(q);
            PS_HIP(hipMemcpyAsync(pin[slot].p, dev[slot].p, (size_t)(p1 - p0), hipMemcpyDeviceToHost, q));
        };
        const auto w0 = clk::now();
        FetchOutput out(tmp_name);
        out.put(d + line_b[0], line_e[0] - line_b[0]); out.put('\n');
        ms_write += ms_since(w0);
        size_t site = 0; uint64_t done = 0; bool open = false;             // the writer: `done` bases of `site` are out, its lead too when `open`
        gather(0);
        for (uint64_t k = 0; k < n_pieces; ++k) {
            if (k + 1 < n_pieces) gather(k + 1);
            const int slot = (int)(k & 1);
            const uint64_t p0 = k * piece, p1 = std::min<uint64_t>(total, p0 + piece);
            PS_HIP(hipStreamSynchronize(lane[slot]->s));
            if (p1 > p0) ms_kernels += ev[slot].ms();
            const auto w1 = clk::now();
            const char *seq = (const char *)pin[slot].p;
            while (site < n) {
                const FetchText &x = text[site];
                if (!open) {
                    if (bed) out.put('>');
                    out.put(d + x.a0, x.a1 - x.a0);
                    if (bed) out.put('\n');
                    open = true;
                }
                const uint64_t from = off[site] + done, to = std::min<uint64_t>(off[site] + (uint64_t)len[site], p1);
                if (to > from) { out.put(seq + (from - p0), (size_t)(to - from)); done += to - from; }
                if (done < (uint64_t)len[site]) break;                    // the rest of this site is in the next piece
                out.put(d + x.b0, x.b1 - x.b0); out.put('\n');
                ++site; done = 0; open = false;
            }
            ms_write += ms_since(w1);
        }
        if (site != n) throw Error(who + "internal: the stream ended before the last site");
        const auto w2 = clk::now();
        out.close(); files.publish_all(); files.keep();
        ms_write += ms_since(w2);
    }
    unsigned long long holes = 0;
    d_holes.download(&holes, 1, s);
    PS_HIP(hipStreamSynchronize(s));
    st.n_hole_bases = holes;
    st.s_kernels = ms_kernels / 1e3; st.s_write = ms_write / 1e3; st.s_total = ms_since(t_all) / 1e3;
    if (stats) *stats = st;
    if (std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip] ps_fetch_sequences (%s): %llu sites (%llu reverse), %llu bases (%llu from holes) in %llu piece(s); "
                             "empty: %llu inverted, %llu without contig, %llu past the end, %llu before base 1; "
                             "total %.3f s: sites file %.3f, index %.3f, scan + gather kernels %.4f, text + file %.3f\n",
                     bed ? "fetchBed" : "fetch", (unsigned long long)st.n_sites, (unsigned long long)st.n_reverse, (unsigned long long)st.n_bases,
                     (unsigned long long)st.n_hole_bases, (unsigned long long)st.n_pieces, (unsigned long long)st.n_inverted,
                     (unsigned long long)st.n_no_contig, (unsigned long long)st.n_past_end, (unsigned long long)st.n_before_start,
                     st.s_total, st.s_read, st.s_index, st.s_kernels, st.s_write);
}

}  // namespace ps
