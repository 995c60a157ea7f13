// ps_combine.hip -- transcript hits lifted to genome coordinates and appended to the genomic mapping: the toolkit's `comb`
// mode and step 5 of `map -t` (include/parasuite_hip.h, ps_combine_genome_transcript).
//
// Replaces utils.postprocessing.CombineGenomeTranscript.combine (the toolkit's src/utils/postprocessing/
// CombineGenomeTranscript.java:36-666), which splits, sorts and parses the exon strings of the reference name again for
// every record and keeps the hits of a read name in a HashMap.  Here the two files are parsed on the host (ps_bam.cpp), the
// exon table of every transcript that a record refers to is parsed once, and the device does the per-record work:
//   k_cb_lift<0>    per placed transcript record: the exon walk of :211-518 -> status bits, lifted start, number of CIGAR words
//   (scan)          exclusive sum of the word counts: where each record's words go
//   k_cb_lift<1>    the same walk again, writing the words (left to right on strand 1, right to left on strand -1)
//   k_cb_heads      head flag: the name bytes differ from the previous placed record's (a group = a head and the records up to
//                   the next head; no group ids are needed, so no scan follows)
//   k_cb_groups     per group head: the run's located records -- all starts equal?, the primaryIndex record, its genome contig
//   k_cb_revcomp    per emitted record of a -1 transcript: the 4-bit packed SEQ reverse-complemented in place
// The host then builds the lifted records (bam_rec_begin / bam_rec_cigar / bam_rec_end) and hands them, after the genomic
// records, to BamSink.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <thread>
#include <unordered_map>
#include "../../include/parasuite_hip.h"
#include "ps_dev.h"
#include "ps_java.h"
#include "ps_pacref.h"

namespace ps {

enum : unsigned { kCbLocated = 1, kCbMissed = 2, kCbSpliced = 4 };
enum : int { kCbNone = 0, kCbEmpty = 1, kCbEmit = 2, kCbAmbiguous = 3, kCbNoContig = 4 };   // per record: not a group head, or its group's outcome
constexpr int kCbNoRef = -2;                                                                  // genome contig of a transcript: absent (-1: MT without chrM)

struct CbLiftArgs {
    int n; const int32_t *ctg, *pos, *l_seq; const uint32_t *flag, *cig_off, *n_cig, *cigar;
    const uint32_t *ex_off; const int32_t *ex_n, *strand, *es, *ee;
    uint32_t *status; int32_t *start; unsigned long long *nwords;       // pass 0 writes these, pass 1 reads nwords
    const unsigned long long *woff; uint32_t *words;                    // pass 1
};

// CombineGenomeTranscript.java:192-518 for one record.  Words are counted (WRITE = 0) or stored (WRITE = 1) at slot k of the
// record's `total` slots, from the right on strand -1 where the Java prepends; a store outside the slots counted in pass 0
// does not happen (the walk is the same), and is refused all the same.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_cb_lift(CbLiftArgs a)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.n) return;
    const int c = a.ctg[j], n_ex = a.ex_n[c], strand = a.strand[c];
    const int32_t *es = a.es + a.ex_off[c], *ee = a.ee + a.ex_off[c];
    const uint32_t *own = a.cigar + a.cig_off[j]; const int n_own = (int)a.n_cig[j];
    bool has_id = false, own_n = false; int ref_len = 0;
    for (int k = 0; k < n_own; ++k) {
        const int op = (int)(own[k] & 15u);
        has_id |= op == 1 || op == 2; own_n |= op == 3;
        if (cigar_on_ref(op)) ref_len += (int)(own[k] >> 4);
    }
    const int aln_start = (int32_t)((uint32_t)a.pos[j] + 1u), read_len = a.l_seq[j];   // htsjdk getAlignmentStart
    const int aln_end = (a.flag[j] & 4u) ? 0 : aln_start + ref_len - 1;       // getAlignmentEnd: 0 for an unmapped (bridging) record
    const int total = WRITE ? (int)a.nwords[j] : 0;
    uint32_t *out = WRITE ? a.words + a.woff[j] : nullptr;
    const bool rev = strand == 2;
    int k = 0, start = -1, passed = 0; bool has_n = false, missed = false;
    auto put = [&](int len, uint32_t op) {
        if (WRITE && k < total) out[rev ? total - 1 - k : k] = ((uint32_t)len << 4) | op;
        ++k; has_n |= op == 3u;
    };
    auto take_own = [&]() {                                                   // newGenomicCigar = readHit.getCigarString()
        if (WRITE) for (int w = 0; w < n_own && w < total; ++w) out[w] = own[w];
        k = n_own; has_n = own_n;
    };
    if (strand == 1) {
        for (int i = 0; i < n_ex; ++i) {
            const int before = passed;
            passed += ee[i] - es[i] + 1;
            if (aln_start <= passed && start == -1) start = es[i] + (aln_start - before) - 1;
            if (aln_end <= passed) {
                if (start >= es[i]) take_own(); else put(aln_end - before, 0u);
                break;
            } else if (start != -1) {
                if (has_id) { missed = true; break; }
                put(start >= es[i] ? ee[i] - start + 1 : ee[i] - es[i] + 1, 0u);
                if (i >= n_ex - 1) break;
                const int intron = es[i + 1] - ee[i] - 1;
                if (intron <= 0) break;
                put(intron, 3u);
            }
        }
    } else if (rev) {
        int end = -1;
        for (int i = n_ex - 1; i >= 0; --i) {
            const int before = passed;
            passed += ee[i] - es[i] + 1;
            if (aln_start <= passed && end == -1) end = ee[i] - (aln_start - before) + 1;
            if (aln_end <= passed) {
                if (end <= ee[i]) { take_own(); start = end - read_len + 1; }
                else {
                    if (has_id) { missed = true; break; }
                    put(aln_end - before, 0u);
                    start = ee[i] - (aln_end - before) + 1;
                }
                break;
            } else if (end != -1) {
                if (has_id) { missed = true; break; }
                put(end < ee[i] ? end - es[i] + 1 : ee[i] - es[i] + 1, 0u);
                if (i < 1) break;
                const int intron = es[i] - ee[i - 1] - 1;
                if (intron <= 0) break;
                put(intron, 3u);
            }
        }
    }
    if (WRITE) return;
    const bool located = start >= 1;                                          // -1: not located; below base 1: see the header's deviations
    a.status[j] = (located ? kCbLocated : 0u) | (missed ? kCbMissed : 0u) | (located && has_n ? kCbSpliced : 0u);
    a.start[j] = start;
    a.nwords[j] = located ? (unsigned long long)k : 0ull;
}

__global__ void __launch_bounds__(256) k_cb_heads(int n, const uint64_t *name_off, const uint8_t *name_len, const uint8_t *names, uint32_t *head)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= n) return;
    bool h = j == 0 || name_len[j] != name_len[j - 1];
    if (!h) {
        const uint8_t *x = names + name_off[j], *y = names + name_off[j - 1];
        for (uint32_t k = 0; k < name_len[j] && !h; ++k) h = x[k] != y[k];
    }
    head[j] = h;
}

// printReadsToBamFile (:598-666) for the group that starts at j: the located records in file order are the Java's lists; the
// one emitted is list entry primaryIndex (the list index last stored by a record without flag 0x100, 0 if none)
__global__ void __launch_bounds__(256) k_cb_groups(int n, const uint32_t *head, const uint32_t *status, const int32_t *start, const uint32_t *flag,
                            const int32_t *ctg, const int32_t *gref, uint8_t *gstat, int32_t *emit)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= n) return;
    if (!head[j]) { gstat[j] = kCbNone; return; }
    int n_loc = 0, primary = 0, first = 0; bool equal = true;
    for (int k = j; k < n && (k == j || !head[k]); ++k) {
        if (!(status[k] & kCbLocated)) continue;
        if (!(flag[k] & 0x100u)) primary = n_loc;
        if (n_loc == 0) first = start[k]; else equal &= start[k] == first;
        ++n_loc;
    }
    emit[j] = -1;
    if (n_loc == 0) { gstat[j] = kCbEmpty; return; }
    if (!equal) { gstat[j] = kCbAmbiguous; return; }
    int e = -1, at = 0;
    for (int k = j; k < n && (k == j || !head[k]); ++k) {
        if (!(status[k] & kCbLocated)) continue;
        if (at++ == primary) { e = k; break; }
    }
    if (gref[ctg[e]] == kCbNoRef) { gstat[j] = kCbNoContig; return; }
    gstat[j] = kCbEmit; emit[j] = e;
}

__device__ __forceinline__ void cb_set_nib(uint8_t *s, int i, unsigned v)
{
    const int sh = (~i & 1) << 2;
    s[i >> 1] = (uint8_t)((s[i >> 1] & ~(15u << sh)) | (v << sh));
}
// SequenceUtil.reverseComplement on BAM nibbles (=ACMGRSVTWYHKDBN): A <-> T, C <-> G, every other code keeps its value
__device__ __forceinline__ unsigned cb_comp(unsigned v) { return v == 1u ? 8u : v == 8u ? 1u : v == 2u ? 4u : v == 4u ? 2u : v; }
// one lane per group head; a record's bases are its own bytes (records start on a byte), so lanes never share a byte
__global__ void __launch_bounds__(256) k_cb_revcomp(int n, const uint8_t *gstat, const int32_t *emit, const int32_t *ctg, const int32_t *strand,
                             const uint64_t *seq_off, const int32_t *l_seq, uint8_t *seq)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= n || gstat[j] != kCbEmit) return;
    const int e = emit[j];
    if (strand[ctg[e]] != 2) return;
    uint8_t *s = seq + (seq_off[e] >> 1); const int L = l_seq[e];
    auto cb_nib = [s](int i) { return (unsigned)bam_nibble(s, (uint64_t)i); };
    for (int i = 0; i < L / 2; ++i) {
        const unsigned x = cb_nib(i), y = cb_nib(L - 1 - i);
        cb_set_nib(s, i, cb_comp(y)); cb_set_nib(s, L - 1 - i, cb_comp(x));
    }
    if (L & 1) cb_set_nib(s, L / 2, cb_comp(cb_nib(L / 2)));
}

// ---- host side

// an exon position of a transcript name: Integer.parseInt, except that more than ten digits are refused whatever they spell
// (leading zeros, which parseInt takes): kept as it has been
static bool cb_exon_int(const std::string &s, int32_t &v)
{
    const size_t sign = !s.empty() && (s[0] == '-' || s[0] == '+');
    return s.size() - sign <= 10 && java_parse_int((const uint8_t *)s.data(), (uint32_t)s.size(), v);
}

struct CbTimes { double parse = 0, tables = 0, h2d = 0, kernels = 0, d2h = 0, assemble = 0, write = 0; };

void combine_run(const char *genome_path, const char *transcript_path, const char *out_bam, bool sort_by_coordinate, bool write_index,
                 int threads, int device, ps_combine_stats *stats)
{
    if (!genome_path || !transcript_path || !out_bam || !out_bam[0]) throw Error("ps_combine_genome_transcript: genomic mapping, transcript mapping and output file are required");
    OutFiles files(".combine-tmp"); const std::string t = add_bam(files, out_bam, write_index);
    files.refuse_inputs({genome_path, transcript_path}, "ps_combine_genome_transcript: ");
    if (write_index && !sort_by_coordinate) throw Error("a .bai index needs coordinate-sorted output");
    require_device(device);                                                // before the files are read
    const auto t0 = HostClock::now();
    BamFile G, T;
    {
        std::string err;
        std::thread other([&]() { try { load_records(transcript_path, std::max(1, threads / 2), T); } catch (const std::exception &e) { err = e.what(); if (err.empty()) err = "error"; } });
        try { load_records(genome_path, std::max(1, threads - threads / 2), G); } catch (...) { other.join(); throw; }
        other.join();
        if (!err.empty()) throw Error(err);
    }
    combine_records(G, T, transcript_path, t.c_str(), sort_by_coordinate, write_index, threads, device, stats, ms_since(t0));
    files.publish_all(); files.keep();
}

// the same on records in memory (both are consumed): the files' loader above, or ps_map_route's passes, which hand over what they
// have just written.  transcript_path: what the error messages call the transcript mapping.  The caller has checked the
// arguments (combine_run above; ps_map_route always asks for the sorted, indexed form on a device it has used) and owns out_bam (§4m).
void combine_records(BamFile &G, BamFile &T, const char *transcript_path, const char *out_bam, bool sort_by_coordinate, bool write_index,
                     int threads, int device, ps_combine_stats *stats, double parse_ms)
{
    threads = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
    PS_HIP(hipSetDevice(device));
    CbTimes tm; ps_combine_stats st{};
    auto t0 = HostClock::now();
    if (T.sort_order != "queryname")                                       // :85-94 (the Java logs this and exits with status 0)
        throw Error(std::string("ps_combine_genome_transcript: ") + transcript_path + " is not sorted by read name: its header says SO:" +
                    (T.sort_order.empty() ? "(none)" : T.sort_order) + ", SO:queryname is required");
    if (T.n() > (size_t)INT_MAX) throw Error("ps_combine_genome_transcript: more than 2^31 transcript records");
    st.n_genome = G.n(); st.n_transcript = T.n();
    tm.parse = parse_ms;

    // placed records (RNAME not '*', :105-107) as flat arrays; exon tables of the transcripts they name, parsed once each
    t0 = HostClock::now();
    std::vector<int32_t> pidx; pidx.reserve(T.n());
    for (size_t i = 0; i < T.n(); ++i) { if (T.recs[i].ref < 0) ++st.n_unplaced; else pidx.push_back((int32_t)i); }
    const int n = (int)pidx.size();
    const size_t n_ctg = std::max<size_t>(1, T.refs.size());
    std::vector<uint8_t> used(n_ctg, 0);
    for (int j = 0; j < n; ++j) {
        const int32_t r = T.recs[(size_t)pidx[(size_t)j]].ref;
        if ((size_t)r >= T.refs.size()) throw Error("ps_combine_genome_transcript: a transcript record refers to a reference that is not in its header");
        used[(size_t)r] = 1;
    }
    std::unordered_map<std::string, int> g_id;
    for (size_t r = 0; r < G.refs.size(); ++r) g_id.emplace(G.refs[r].first, (int)r);
    auto g_find = [&](const std::string &nm) { auto it = g_id.find(nm); return it == g_id.end() ? -1 : it->second; };
    std::vector<uint32_t> ex_off(n_ctg, 0); std::vector<int32_t> ex_n(n_ctg, 0), strand(n_ctg, 0), gref(n_ctg, kCbNoRef), es, ee;
    for (size_t c = 0; c < T.refs.size(); ++c) {
        if (!used[c]) continue;
        const std::string &nm = T.refs[c].first;
        const std::vector<std::string> f = java_split(nm, '|');
        if (f.size() < 6) throw Error("ps_combine_genome_transcript: transcript name " + nm + " has fewer than six '|' fields (Gene|Transcript|Chr|starts|ends|strand)");
        std::vector<std::string> s = java_split(f[3], ';'), e = java_split(f[4], ';');
        if (s.size() != e.size()) throw Error("ps_combine_genome_transcript: transcript name " + nm + " lists " + std::to_string(s.size()) + " exon starts and " + std::to_string(e.size()) + " exon ends");
        std::sort(s.begin(), s.end()); std::sort(e.begin(), e.end());      // Arrays.sort(String[]): byte order, "100000" before "99990"
        ex_off[c] = (uint32_t)es.size(); ex_n[c] = (int32_t)s.size();
        for (size_t k = 0; k < s.size(); ++k) {
            int32_t a = 0, b = 0;
            if (!cb_exon_int(s[k], a) || !cb_exon_int(e[k], b)) throw Error("ps_combine_genome_transcript: transcript name " + nm + " has an exon position that is not a number");
            es.push_back(a); ee.push_back(b);
        }
        strand[c] = f[5] == "1" ? 1 : (f[5] == "-1" ? 2 : 0);
        const int first = g_find("chr" + f[2]);                            // :621-631: "chrMT" is looked up before MT becomes M
        if (first < 0) gref[c] = kCbNoRef;
        else if (f[2] == "MT") gref[c] = g_find("chrM");
        else gref[c] = first;
    }
    if (es.size() > (size_t)UINT_MAX) throw Error("ps_combine_genome_transcript: more than 2^32 exons");
    RecTable R;
    try { flatten_records(T, kRecCigar | kRecSeq | kRecNames, &pidx, threads, R); } catch (const std::exception &e) { throw Error(std::string("ps_combine_genome_transcript: ") + e.what()); }
    const std::vector<int32_t> &ctg = R.ref, &l_seq = R.l_seq; const std::vector<uint32_t> &flag = R.flag, &n_cig = R.n_cig;
    std::vector<uint8_t> &seq = R.seq;
    tm.tables = ms_since(t0);

    // device
    t0 = HostClock::now();
    StreamGuard sg; hipStream_t s = sg.s;
    DevRecTable d; DevBuf<int32_t> d_exn, d_strand, d_es, d_ee, d_gref; DevBuf<uint32_t> d_exoff;
    d.upload(R, s);
    upload(d_exoff, ex_off, s); upload(d_exn, ex_n, s); upload(d_strand, strand, s); upload(d_es, es, s); upload(d_ee, ee, s); upload(d_gref, gref, s);
    const size_t nn = (size_t)std::max(1, n);
    DevBuf<uint32_t> d_status, d_head, d_words; DevBuf<int32_t> d_start, d_emit; DevBuf<unsigned long long> d_nw, d_woff; DevBuf<uint8_t> d_gstat;
    d_status.alloc(nn); d_head.alloc(nn); d_start.alloc(nn); d_emit.alloc(nn); d_nw.alloc(nn); d_woff.alloc(nn); d_gstat.alloc(nn);
    PS_HIP(hipStreamSynchronize(s));
    tm.h2d = ms_since(t0);

    t0 = HostClock::now();
    unsigned long long total_words = 0;
    if (n) {
        CbLiftArgs a;
        a.n = n; a.ctg = d.ref.p; a.pos = d.pos.p; a.l_seq = d.l_seq.p; a.flag = d.flag.p; a.cig_off = d.cig_off.p; a.n_cig = d.n_cig.p; a.cigar = d.cigar.p;
        a.ex_off = d_exoff.p; a.ex_n = d_exn.p; a.strand = d_strand.p; a.es = d_es.p; a.ee = d_ee.p;
        a.status = d_status.p; a.start = d_start.p; a.nwords = d_nw.p; a.woff = d_woff.p; a.words = nullptr;
        hipLaunchKernelGGL(k_cb_lift<false>, dim3(blocks_for((size_t)n)), dim3(256), 0, s, a);
        PS_HIP(hipGetLastError());
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, d_nw.p, d_woff.p, n, s); });
        unsigned long long lw = 0, lo = 0;
        PS_HIP(hipMemcpyAsync(&lw, d_nw.p + (n - 1), sizeof lw, hipMemcpyDeviceToHost, s));
        PS_HIP(hipMemcpyAsync(&lo, d_woff.p + (n - 1), sizeof lo, hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        total_words = lo + lw;
        d_words.alloc((size_t)std::max<unsigned long long>(1, total_words));
        a.words = d_words.p;
        hipLaunchKernelGGL(k_cb_lift<true>, dim3(blocks_for((size_t)n)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_cb_heads, dim3(blocks_for((size_t)n)), dim3(256), 0, s, n, d.name_off.p, d.name_len.p, d.names.p, d_head.p);
        hipLaunchKernelGGL(k_cb_groups, dim3(blocks_for((size_t)n)), dim3(256), 0, s, n, d_head.p, d_status.p, d_start.p, d.flag.p, d.ref.p, d_gref.p, d_gstat.p, d_emit.p);
        hipLaunchKernelGGL(k_cb_revcomp, dim3(blocks_for((size_t)n)), dim3(256), 0, s, n, d_gstat.p, d_emit.p, d.ref.p, d_strand.p, d.seq_off.p, d.l_seq.p, d.seq.p);
        PS_HIP(hipGetLastError());
        PS_HIP(hipStreamSynchronize(s));
    }
    tm.kernels = ms_since(t0);

    t0 = HostClock::now();
    std::vector<uint32_t> status((size_t)n), words((size_t)total_words); std::vector<int32_t> start((size_t)n), emit((size_t)n);
    std::vector<unsigned long long> nw((size_t)n), woff((size_t)n); std::vector<uint8_t> gstat((size_t)n);
    if (n) {
        d_status.download(status.data(), (size_t)n, s); d_start.download(start.data(), (size_t)n, s); d_emit.download(emit.data(), (size_t)n, s);
        d_nw.download(nw.data(), (size_t)n, s); d_woff.download(woff.data(), (size_t)n, s); d_gstat.download(gstat.data(), (size_t)n, s);
        if (total_words) d_words.download(words.data(), (size_t)total_words, s);
        if (!seq.empty()) d.seq.download(seq.data(), seq.size(), s);
        PS_HIP(hipStreamSynchronize(s));
    }
    tm.d2h = ms_since(t0);

    // the records
    t0 = HostClock::now();
    std::vector<int32_t> out_rec;                                          // emitted records, in transcript-file order of their groups
    for (int j = 0; j < n; ++j) {
        if (!(status[(size_t)j] & kCbLocated)) ++st.n_unlocated;
        if (status[(size_t)j] & kCbMissed) ++st.n_missed_indel_splice;
        if (status[(size_t)j] & kCbSpliced) ++st.n_spliced;
        const int g = gstat[(size_t)j];
        if (g != kCbNone) ++st.n_groups;
        if (g == kCbAmbiguous) ++st.n_groups_ambiguous;
        if (g == kCbNoContig) ++st.n_no_contig;
        if (g == kCbEmit) {
            const int e = emit[(size_t)j];
            if (e < 0 || e >= n) throw Error("ps_combine_genome_transcript: internal error (emitted record out of range)");
            out_rec.push_back(e);
            if (gref[(size_t)ctg[(size_t)e]] < 0) ++st.n_mt_unplaced;
            if (strand[(size_t)ctg[(size_t)e]] == 2) ++st.n_strand_flipped;
        }
    }
    st.n_lifted = out_rec.size();
    const int W = std::max(1, std::min<int>(threads, (int)(out_rec.size() / 4096) + 1));
    std::vector<std::string> bufs((size_t)W); std::vector<std::vector<BamRec>> brecs((size_t)W); std::vector<std::string> errs((size_t)W);
    auto le32 = [](const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
    auto build = [&](int w) {
        try {
            std::string &o = bufs[(size_t)w];
            const size_t a0 = out_rec.size() * (size_t)w / (size_t)W, a1 = out_rec.size() * (size_t)(w + 1) / (size_t)W;
            for (size_t x = a0; x < a1; ++x) {
                const int e = out_rec[x]; const uint8_t *p = T.rec((size_t)pidx[(size_t)e]);
                const size_t bs = le32(p), l_name = p[12], nc0 = n_cig[(size_t)e], ls = (size_t)l_seq[(size_t)e];
                const uint32_t *cw = words.data() + woff[(size_t)e]; const size_t nc = (size_t)nw[(size_t)e];
                if (nc > 65535) throw Error("ps_combine_genome_transcript: a lifted CIGAR has more than 65535 operations");
                const int64_t ref_len = cigar_ref_span(cw, (uint32_t)nc);
                const int c = ctg[(size_t)e]; const int32_t pos = start[(size_t)e] - 1;
                BamCore core{gref[(size_t)c], pos, pos + (ref_len > 0 ? ref_len : 1), 10, (int)(flag[(size_t)e] ^ (strand[(size_t)c] == 2 ? 16u : 0u)),
                             (uint32_t)nc, (uint32_t)ls, (int32_t)le32(p + 24), (int32_t)le32(p + 28), (int32_t)le32(p + 32)};
                BamRec r; r.part = w;
                bam_rec_begin(o, core, (const char *)p + 36, l_name - 1, r);
                bam_rec_cigar(o, cw, nc);
                const uint8_t *q = p + 36 + l_name + 4 * nc0 + (ls + 1) / 2;  // QUAL as it is (the Java does not reverse it), then the tags
                o.append((const char *)seq.data() + R.seq_off[(size_t)e] / 2, (ls + 1) / 2);
                o.append((const char *)q, (size_t)(p + 4 + bs - q));
                bam_rec_end(o, r);
                brecs[(size_t)w].push_back(r);
            }
        } catch (const std::exception &ex) { errs[(size_t)w] = ex.what(); if (errs[(size_t)w].empty()) errs[(size_t)w] = "error"; }
    };
    { std::vector<std::thread> th; for (int w = 1; w < W; ++w) th.emplace_back(build, w); build(0); for (auto &x : th) x.join(); }
    for (const std::string &e : errs) if (!e.empty()) throw Error(e);
    tm.assemble = ms_since(t0);

    // genomic records in file order, then the lifted ones
    t0 = HostClock::now();
    BamStats bst;
    BamSink sink(G.text, G.refs, out_bam, sort_by_coordinate, write_index, threads, 6);
    std::vector<std::vector<BamRec>> grecs(G.enc.size());
    for (const BamRec &r : G.recs) grecs[(size_t)r.part].push_back(r);
    const uint64_t n_g = G.n();
    G.recs.clear(); G.recs.shrink_to_fit();
    sink.add(G.enc, grecs, n_g);
    sink.add(bufs, brecs, st.n_lifted);
    sink.finish(&bst);
    tm.write = ms_since(t0);
    st.bam_bytes = bst.bam_bytes;
    if (stats) *stats = st;
    if (std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip] ps_combine_genome_transcript: %llu genomic + %llu transcript records (%llu unplaced, %llu unlocated), %llu groups, "
                             "%llu lifted (%llu spliced records, %llu strand-flipped); parse %.1f ms, tables %.1f ms, H2D %.1f ms, kernels + scan %.1f ms, "
                             "D2H %.1f ms, record assembly %.1f ms, sort + BGZF + write %.1f ms\n",
                     (unsigned long long)st.n_genome, (unsigned long long)st.n_transcript, (unsigned long long)st.n_unplaced, (unsigned long long)st.n_unlocated,
                     (unsigned long long)st.n_groups, (unsigned long long)st.n_lifted, (unsigned long long)st.n_spliced, (unsigned long long)st.n_strand_flipped,
                     tm.parse, tm.tables, tm.h2d, tm.kernels, tm.d2h, tm.assemble, tm.write);
}

}  // namespace ps
