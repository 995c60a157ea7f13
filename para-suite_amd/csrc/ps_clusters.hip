// ps_clusters.hip -- RBP-bound clusters with T->C statistics: the toolkit's `clust` mode (include/parasuite_hip.h,
// ps_pileup_clusters).
//
// Replaces utils.pileupclusters.PileupClusters.calculateReadPileups (the toolkit's src/utils/pileupclusters/
// PileupClusters.java:62-673), which walks the sorted BAM one record at a time with a getSubsequenceAt call and HashMap
// updates per read.  Here the records are parsed on the host (ps_bam.cpp), and the device does the counting:
//   k_cl_classify   per record: skip reasons, alignment start / end, errors
//   (select)        the kept records, in file order
//   k_cl_seg..      cluster boundaries (rule 2 of DESIGN §4c): one segmented max-scan of the alignment ends gives the Java's
//                   clusterEnd wherever it is "in sync"; a record with a short span that opens a cluster below the running
//                   maximum starts a stretch that one lane walks record by record up to the next record the scan opens
//   k_cl_count      per aligned base: coverage and T->C counts of the site, the first insertion (record << 16 | read index)
//                   for the HashMap order, read-index flags per cluster
//   k_cl_reduce     per cluster (one wave): SNP test, HashMap-order best site; then segmented radix sorts (fractions descending,
//                   buckets ascending) and k_cl_sum: the fractions' sum in that order, buckets of more than 8 sites
//   k_cl_sitefreq   one lane per rank k walks the crosslinked clusters in file order (the Java's sequential double sums)
// The host builds the cluster and CCR sequences from the FASTA bytes and writes the text.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <zlib.h>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <thread>
#include <unordered_map>
#include "../../include/parasuite_hip.h"
#include "ps_dev.h"
#include "ps_inflate.h"
#include "ps_java.h"
#include "ps_pacref.h"

namespace ps {

enum : unsigned { kClErrContig = 1, kClErrPastEnd = 2, kClErrSeq = 4, kClErrLong = 8 };

// per record; keep: 1 = a record the Java clusters (not flag 4, CIGAR not (I or D) and N, :146-157); cnt: unmapped, skipped
__global__ void k_cl_classify(int n, const uint32_t *flag, const int32_t *ref, const int32_t *pos, const int32_t *l_seq,
                              const uint32_t *cig_off, const uint32_t *n_cig, const uint32_t *cigar, const int32_t *ref_to_contig,
                              int n_refs, const int32_t *contig_len, uint8_t *keep, int32_t *start, int32_t *end,
                              unsigned long long *cnt, unsigned *err)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n) return;
    keep[r] = 0;
    if (flag[r] & 4u) { atomicAdd(&cnt[0], 1ull); return; }
    const uint32_t *cg = cigar + cig_off[r];
    bool has_i = false, has_d = false, has_n = false, over = false;
    int span = 0, rp = 0, bases = 0;
    for (int c = 0; c < (int)n_cig[r]; ++c) {
        const int op = (int)(cg[c] & 15u), len = (int)(cg[c] >> 4);
        has_i |= op == 1; has_d |= op == 2; has_n |= op == 3;
        if (cigar_on_ref(op)) span += len;
        if (op == 0 || op == 7 || op == 8) { bases += len; over |= rp + len > l_seq[r]; }
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) rp += len;
    }
    if ((has_i || has_d) && has_n) { atomicAdd(&cnt[1], 1ull); return; }
    const int rid = ref[r], ctg = rid >= 0 && rid < n_refs ? ref_to_contig[rid] : -1;
    if (ctg < 0) { atomicOr(err, kClErrContig); return; }
    const int s = pos[r] + 1, e = s + span - 1;                          // htsjdk getAlignmentStart / getAlignmentEnd
    if (e > contig_len[ctg]) atomicOr(err, kClErrPastEnd);
    if (l_seq[r] == 0 || over) atomicOr(err, kClErrSeq);
    if (bases >= 65536) atomicOr(err, kClErrLong);
    keep[r] = 1; start[r] = s; end[r] = e;
}

// kept index j -> its record's start, end, strand, reference id; head: the reference name differs from the previous record's
__global__ void k_cl_gather(int K, const int32_t *kidx, const int32_t *start, const int32_t *end, const uint32_t *flag, const int32_t *ref,
                            int32_t *sk, int32_t *ek, uint8_t *rv, int32_t *rk, uint32_t *head)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= K) return;
    const int r = kidx[j];
    sk[j] = start[r]; ek[j] = end[r]; rv[j] = (flag[r] & 16u) ? 1 : 0; rk[j] = ref[r];
    head[j] = j == 0 || ref[kidx[j - 1]] != ref[r];
}
__global__ void k_cl_key(int K, const uint32_t *seg, const int32_t *ek, unsigned long long *key)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < K) key[j] = ((unsigned long long)seg[j] << 32) | (uint32_t)ek[j];
}
// Rule 2 (:175-176): j opens iff clusterEnd - start_j < 5 or the reference changes.  mx[j - 1] (low word) is the running
// maximum M of the ends of the same reference; the Java's clusterEnd c <= M always, and c == M until a record opens with
// end < M (a span below 5).  So "M - start < 5" opens exactly where c == M; such a record is a true opener in any case
// (c <= M), and it resets the state (stop).  desync: an opener with end < M, after which c < M until the next stop.
__global__ void k_cl_open(int K, const uint32_t *seg, const unsigned long long *mx, const int32_t *sk, const int32_t *ek,
                          uint32_t *open, uint8_t *stop, uint8_t *desync)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= K) return;
    if (j == 0 || seg[j] != seg[j - 1]) { open[j] = 1; stop[j] = 1; desync[j] = 0; return; }
    const int M = (int)(uint32_t)mx[j - 1];
    const bool naive = M - sk[j] < 5;
    open[j] = naive; stop[j] = naive; desync[j] = naive && ek[j] < M;
}
// one lane per desynchronised stretch: the Java's recurrence, record by record, up to the next record that opens for the scan
__global__ void k_cl_fix(int K, const uint8_t *desync, const uint8_t *stop, const int32_t *sk, const int32_t *ek, uint32_t *open)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= K || !desync[j]) return;
    int c = ek[j];
    for (int k = j + 1; k < K && !stop[k]; ++k) {
        const bool o = c - sk[k] < 5;
        open[k] = o;
        c = o ? ek[k] : max(c, ek[k]);
    }
}
__global__ void k_cl_init(int C, int32_t *lo, int32_t *hi)
{
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c < C) { lo[c] = INT_MAX; hi[c] = INT_MIN; }
}
// per kept record: its cluster (cid - 1); the cluster's opener, read count, reverse members after the opener, window [lo, hi]
__global__ void k_cl_members(int K, const uint32_t *open, const uint32_t *cid, const int32_t *sk, const int32_t *ek, const uint8_t *rv,
                             int32_t *opener, uint32_t *nreads, uint32_t *nrev, int32_t *lo, int32_t *hi)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= K) return;
    const int c = (int)cid[j] - 1;
    if (open[j]) opener[c] = j;
    else if (rv[j]) atomicAdd(&nrev[c], 1u);
    atomicAdd(&nreads[c], 1u);
    atomicMin(&lo[c], sk[j]); atomicMax(&hi[c], ek[j]);
}
__global__ void k_cl_width(int C, const int32_t *lo, const int32_t *hi, unsigned long long *w)
{
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c < C) w[c] = hi[c] >= lo[c] ? (unsigned long long)((int64_t)hi[c] - lo[c] + 1) : 0ull;
}

struct ClCountArgs {
    int K; const int32_t *kidx; const uint32_t *cid; const int32_t *sk, *ek; const uint8_t *rv;
    const int32_t *ref, *ref_to_contig; const int64_t *contig_off;
    const uint32_t *cig_off, *n_cig, *cigar; const uint64_t *seq_off; const uint8_t *seq;
    const uint8_t *pac; const int64_t *hole_off; const int32_t *hole_len; int n_holes;
    const int32_t *lo, *hi; const unsigned long long *off;
    uint32_t *cov, *t2c; unsigned long long *first, *cflags, *ct2c, *beyond;
};
// calculateClusterInformation, :585-673, one record per lane.  The read and reference bases of the alignment blocks (M, =, X)
// are concatenated (length B) and reverse-complemented on the reverse strand, so concatenation index u is read index
// i = B-1-u there, and a T->C there is reference A with read G.  Index i is booked at start + i, or end - i on the reverse
// strand (the Java's shifted positions after D / N included).
__global__ void __launch_bounds__(256) k_cl_count(ClCountArgs a)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j >= a.K) return;
    const int r = a.kidx[j], c = (int)a.cid[j] - 1, s = a.sk[j], e = a.ek[j];
    const bool rev = a.rv[j] != 0;
    const int64_t g1 = a.contig_off[a.ref_to_contig[a.ref[r]]] - 1;       // + 1-based position = offset on the packed strand
    const uint32_t *cg = a.cigar + a.cig_off[r]; const int nc = (int)a.n_cig[r];
    int B = 0;
    for (int k = 0; k < nc; ++k) { const int op = (int)(cg[k] & 15u); if (op == 0 || op == 7 || op == 8) B += (int)(cg[k] >> 4); }
    const int lo = a.lo[c], hi = a.hi[c];
    const unsigned long long base = a.off[c];
    ProfRef rf{a.pac, a.hole_off, a.hole_len, a.n_holes, 0};
    rf.seek(g1 + s);
    const uint64_t sb = a.seq_off[r];
    unsigned long long flags = 0, n_t2c = 0, n_beyond = 0;
    int rp = 0, gp = s, u = 0;
    for (int k = 0; k < nc; ++k) {
        const int op = (int)(cg[k] & 15u), len = (int)(cg[k] >> 4);
        if (op == 0 || op == 7 || op == 8) {
            for (int z = 0; z < len; ++z, ++u) {
                const int pr = rf.at(g1 + gp + z);
                const uint64_t b = sb + (uint64_t)(rp + z);
                const int nib = bam_nibble(a.seq, b);
                const int i = rev ? B - 1 - u : u, p = rev ? e - i : s + i;
                if (p < lo || p > hi) continue;                              // never: [start, end] lies in the window
                const unsigned long long at = base + (unsigned long long)(p - lo);
                atomicAdd(&a.cov[at], 1u);
                if (rev ? (pr == 0 && nib == 4) : (pr == 3 && nib == 2)) {   // reference T, read C after the reverse complement
                    atomicAdd(&a.t2c[at], 1u);
                    atomicMin(&a.first[at], ((unsigned long long)j << 16) | (unsigned)i);
                    ++n_t2c;
                    if (i < 51) flags |= 1ull << i; else ++n_beyond;
                }
            }
            rp += len; gp += len;
        } else if (op == 1 || op == 4) rp += len;
        else if (op == 2 || op == 3) gp += len;
    }
    if (flags) atomicOr(&a.cflags[c], flags);
    if (n_t2c) atomicAdd(&a.ct2c[c], n_t2c);
    if (n_beyond) atomicAdd(a.beyond, n_beyond);
}
// sites (positions with a T->C) per cluster: one wave per cluster
__global__ void __launch_bounds__(64) k_cl_nsites(const unsigned long long *off, const unsigned long long *w, const uint32_t *t2c, uint32_t *nsites)
{
    const int c = (int)blockIdx.x;
    unsigned n = 0;
    for (unsigned long long p = threadIdx.x; p < w[c]; p += 64) n += t2c[off[c] + p] != 0;
    if (n) atomicAdd(&nsites[c], n);
}

struct ClOut { int32_t best_pos; uint32_t best_cnt; double best_val, sum; uint32_t n_kept, snp_hits, snv, unmodelled; };
__device__ __forceinline__ unsigned cl_bucket(int p, unsigned cap) { const unsigned h = (unsigned)p; return (h ^ (h >> 16)) & (cap - 1); }

struct ClReduceArgs {
    int n_eval, min_cov; const uint32_t *nreads, *maxsites; const int32_t *opener, *rk, *lo; const unsigned long long *off, *w;
    const uint32_t *cov, *t2c; const unsigned long long *first; const unsigned long long *snp; int n_snp;
    uint32_t *sbk; double *sfrac; unsigned long long *kend, *bend; ClOut *out;
};
__device__ __forceinline__ bool cl_better(double v, unsigned bk, unsigned long long f, double v2, unsigned bk2, unsigned long long f2)
{
    return v > v2 || (v == v2 && (bk > bk2 || (bk == bk2 && f > f2)));
}
// :180-222 for one closing cluster per wave, over its window in 64-position steps.  HashMap order (rule 6): bucket
// (p ^ p >>> 16) & (cap - 1), then first insertion; cap = the smallest power of two >= 16 holding the largest site count so
// far at load factor 0.75.  `>=` keeps the last maximum in that order, i.e. the largest (fraction, bucket, first insertion):
// a total order (a first insertion names one site), so the lanes' maxima combine in any order.  The sites' buckets and the
// kept fractions are written compacted, in position order, at the cluster's offset (segments [off, bend) and [off, kend)) for
// the two segmented sorts that follow.
__global__ void __launch_bounds__(64) k_cl_reduce(ClReduceArgs a)
{
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    const unsigned long long o = a.off[c];
    if ((int64_t)a.nreads[c] < (int64_t)a.min_cov) { if (lane == 0) { a.kend[c] = o; a.bend[c] = o; } return; }
    unsigned cap = 16;
    while ((unsigned long long)a.maxsites[c] * 4 > 3ull * cap) cap <<= 1;
    const unsigned long long W = a.w[c], lt = (1ull << lane) - 1;
    const int lo = a.lo[c];
    const unsigned long long rkey = (unsigned long long)(uint32_t)a.rk[a.opener[c]] << 32;
    double bv = -1.0; unsigned bb = 0, bx = 0; unsigned long long bf = 0; int bp = -1;
    unsigned n0 = 0, m = 0, snp_hits = 0, snv = 0;
    for (unsigned long long p0 = 0; p0 < W; p0 += 64) {
        const unsigned long long p = p0 + (unsigned long long)lane;
        const uint32_t x = p < W ? a.t2c[o + p] : 0u;
        const int pos = lo + (int)p;
        bool snp = false;
        if (x) {
            const unsigned long long key = rkey | (uint32_t)pos;
            int l = 0, h = a.n_snp;
            while (l < h) { const int mid = (l + h) >> 1; if (a.snp[mid] < key) l = mid + 1; else h = mid; }
            snp = l < a.n_snp && a.snp[l] == key;
        }
        const unsigned long long ms = __ballot(x != 0), mk = __ballot(x != 0 && !snp);
        if (x) {
            const unsigned bk = cl_bucket(pos, cap);
            a.sbk[o + n0 + (unsigned)__popcll(ms & lt)] = bk;
            snp_hits += snp; snv += x == 1;
            if (!snp) {
                const double v = (double)x / (double)a.cov[o + p];
                a.sfrac[o + m + (unsigned)__popcll(mk & lt)] = v;
                const unsigned long long f = a.first[o + p];
                if (bp < 0 || cl_better(v, bk, f, bv, bb, bf)) { bv = v; bb = bk; bf = f; bp = pos; bx = x; }
            }
        }
        n0 += (unsigned)__popcll(ms); m += (unsigned)__popcll(mk);
    }
    for (int d = 32; d > 0; d >>= 1) {
        const double v = __shfl_xor(bv, d); const unsigned bk = __shfl_xor(bb, d), x = __shfl_xor(bx, d);
        const unsigned long long f = __shfl_xor(bf, d); const int pp = __shfl_xor(bp, d);
        if (pp >= 0 && (bp < 0 || cl_better(v, bk, f, bv, bb, bf))) { bv = v; bb = bk; bf = f; bp = pp; bx = x; }
        snp_hits += __shfl_xor(snp_hits, d); snv += __shfl_xor(snv, d);
    }
    if (lane == 0) {
        a.out[c] = ClOut{bp, bx, bp < 0 ? 0.0 : bv, 0.0, m, snp_hits, snv, 0};
        a.kend[c] = o + m; a.bend[c] = o + n0;
    }
}
// after the sorts: the descending fractions summed in that order, one rounded add at a time (:223-260), and whether a bucket
// holds more than 8 sites (the sorted buckets of a cluster: a run of 9 equal values)
__global__ void __launch_bounds__(64) k_cl_sum(int n_eval, int min_cov, const uint32_t *nreads, const unsigned long long *off, const unsigned long long *bend,
                                              const uint32_t *sbk, const double *sfrac, ClOut *out)
{
#pragma clang fp contract(off)
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (c >= n_eval || (int64_t)nreads[c] < (int64_t)min_cov) return;
    const unsigned long long o = off[c], n0 = bend[c] - o;
    bool over = false;
    for (unsigned long long k = (unsigned long long)lane; k + 8 < n0; k += 64) over |= sbk[o + k] == sbk[o + k + 8];
    over = __ballot(over) != 0;
    if (lane == 0) {
        const unsigned m = out[c].n_kept;
        double sum = 0.0;
        for (unsigned i = 0; i < m; ++i) sum += sfrac[o + i];
        out[c].sum = sum; out[c].unmodelled = over;
    }
}

// .sitefrequency (:232-248, :531-538): alleleFrequencyInformation[k] is the file-order sum of the k-th largest fraction over the
// crosslinked clusters, the first one's value doubled for k >= 1 (addAll, then set(k, get(k) + sorted[k])).  One lane per k,
// one block per 64 ranks; wave 0 adds, waves 1..7 stage the next chunk's values in LDS (each cluster's ranks are adjacent,
// so a loader wave's loads coalesce), as k_qual_sd does.
constexpr int kSfLoaders = 7, kSfPer = 8, kSfChunk = kSfLoaders * kSfPer;
__global__ void __launch_bounds__(64 * (kSfLoaders + 1)) k_cl_sitefreq(const int32_t *__restrict__ xl, int n_xl, const unsigned long long *__restrict__ off,
                                                                       const ClOut *__restrict__ res, const double *__restrict__ sfrac, int kmax, double *__restrict__ acc)
{
#pragma clang fp contract(off)
    __shared__ double buf[2][kSfChunk][64];                  // 56 KiB; -1: the cluster has no k-th fraction
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), k = (int)blockIdx.x * 64 + lane;
    const int n_chunks = (n_xl + kSfChunk - 1) / kSfChunk;
    double s = 0.0;
    for (int ch = 0; ch <= n_chunks; ++ch) {
        if (wave > 0 && ch < n_chunks) {
            const int u0 = ch * kSfChunk + (wave - 1) * kSfPer;
#pragma unroll
            for (int q = 0; q < kSfPer; ++q) {
                const int u = u0 + q;
                double v = -1.0;
                if (u < n_xl) { const int c = xl[u]; if (k < (int)res[c].n_kept) v = sfrac[off[c] + (unsigned long long)k]; }
                buf[ch & 1][(wave - 1) * kSfPer + q][lane] = v;
            }
        }
        if (wave == 0 && ch > 0) {
            const int u0 = (ch - 1) * kSfChunk, n = min(kSfChunk, n_xl - u0);
            for (int q = 0; q < n; ++q) {
                const double v = buf[(ch - 1) & 1][q][lane];
                if (v >= 0.0) s = s + (u0 + q == 0 && k >= 1 ? v + v : v);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && k < kmax) acc[k] = s;
}

// ---- host side

// the whole FASTA as stored (soft-masked lower case kept): first word of the header -> bases
static std::unordered_map<std::string, std::string> cl_read_fasta(const char *path)
{
    std::string b;                                             // plain, gzip or BGZF, as ps_index reads the same path (ps_inflate.h)
    {
        ByteSource src(path, "cannot open ");
        read_all(src, b, 8);
    }
    std::unordered_map<std::string, std::string> out;
    std::string *cur = nullptr;
    size_t i = 0;
    while (i < b.size()) {
        size_t e = b.find('\n', i); if (e == std::string::npos) e = b.size();
        size_t l = e; if (l > i && b[l - 1] == '\r') --l;
        if (b[i] == '>') {
            size_t q = i + 1; while (q < l && b[q] != ' ' && b[q] != '\t') ++q;
            cur = &out[b.substr(i + 1, q - i - 1)];
        } else if (cur) cur->append(b, i, l - i);
        i = e + 1;
    }
    return out;
}
// SNPCalling.querySNP (SNPCalling.java:49-69) as a table: (BAM reference id << 32 | POS) of every VCF record whose CHROM is
// a reference name with a leading "chr" stripped, whose REF holds T and whose first ALT allele holds C (upper-cased)
static std::vector<unsigned long long> cl_read_vcf(const char *path, const std::vector<std::pair<std::string, uint32_t>> &refs)
{
    std::vector<unsigned long long> keys;
    if (!path || !path[0]) return keys;
    gzFile g = gzopen(path, "rb");                             // plain text, gzip and BGZF (concatenated members) alike
    if (!g) throw Error(std::string("cannot open ") + path);
    std::string text; char buf[1 << 16]; int n;
    while ((n = gzread(g, buf, sizeof buf)) > 0) text.append(buf, (size_t)n);
    const bool bad = n < 0;
    gzclose(g);
    if (bad) throw Error(std::string("cannot read ") + path);
    std::unordered_map<std::string, std::vector<int>> by_chrom;
    for (size_t r = 0; r < refs.size(); ++r) {
        const std::string &nm = refs[r].first;
        by_chrom[nm.compare(0, 3, "chr") == 0 ? nm.substr(3) : nm].push_back((int)r);
    }
    size_t i = 0;
    while (i < text.size()) {
        size_t e = text.find('\n', i); if (e == std::string::npos) e = text.size();
        if (e > i && text[i] != '#') {
            std::string line = text.substr(i, e - i);
            if (!line.empty() && line.back() == '\r') line.pop_back();
            std::string f[5]; size_t p = 0; int k = 0;
            for (; k < 5 && p <= line.size(); ++k) { size_t q = line.find('\t', p); if (q == std::string::npos) q = line.size(); f[k] = line.substr(p, q - p); p = q + 1; }
            auto it = by_chrom.find(f[0]);
            if (k == 5 && it != by_chrom.end()) {
                std::string ref = f[3], alt = f[4].substr(0, f[4].find(','));
                for (char &ch : ref) ch = (char)std::toupper((unsigned char)ch);
                for (char &ch : alt) ch = (char)std::toupper((unsigned char)ch);
                const bool symbolic = alt.empty() || alt[0] == '<' || alt == "*" || alt.find('[') != std::string::npos || alt.find(']') != std::string::npos;
                const long pos = std::strtol(f[1].c_str(), nullptr, 10);
                if (!symbolic && ref.find('T') != std::string::npos && alt.find('C') != std::string::npos && pos > 0 && pos <= INT_MAX)
                    for (int r : it->second) keys.push_back(((unsigned long long)(uint32_t)r << 32) | (uint32_t)pos);
            }
        }
        i = e + 1;
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    return keys;
}
static void cl_revcomp(std::string &s)                         // htsjdk SequenceUtil.reverseComplement: case kept, other bytes as they are
{
    std::reverse(s.begin(), s.end());
    for (char &c : s)
        switch (c) { case 'A': c = 'T'; break; case 'T': c = 'A'; break; case 'C': c = 'G'; break; case 'G': c = 'C'; break;
                     case 'a': c = 't'; break; case 't': c = 'a'; break; case 'c': c = 'g'; break; case 'g': c = 'c'; break; default: break; }
}

struct ClResult {
    std::string out, fasta, tsv, report, sitefreq, sitepos;
    ps_cluster_stats st{};
    double ms_parse = 0, ms_vcf = 0, ms_kernels = 0, ms_text = 0;
};

static void pileup_clusters(const char *mapping, const char *ref_fa, const char *vcf, int min_cov, int device, int threads, ClResult &res)
{
    require_device(device);
    auto t0 = HostClock::now();
    RecTable t;
    try { load_rec_table(mapping, kRecCigar | kRecSeq, threads, t); } catch (const std::exception &e) { throw Error(e.what()); }
    if (t.sort_order != "coordinate")                                  // :85-92
        throw Error(std::string("ps_pileup_clusters: ") + mapping + " is not sorted by coordinate: its header says SO:" +
                    (t.sort_order.empty() ? "(none)" : t.sort_order) + ", SO:coordinate is required");
    if (t.n() > (size_t)INT_MAX) throw Error("ps_pileup_clusters: more than 2^31 records");
    res.ms_parse = ms_since(t0);
    t0 = HostClock::now();
    const std::vector<unsigned long long> snp = cl_read_vcf(vcf, t.refs);
    res.ms_vcf = ms_since(t0);

    t0 = HostClock::now();
    StreamGuard sg; hipStream_t s = sg.s;
    Index ix;
    index_load_pac(ref_fa, ix, s);
    const RefTables rt(ix, s);
    const std::vector<int32_t> ref_to_contig = RefTables::ref_to_contig(ix, t.refs);
    const int n = (int)t.n();
    DevRecTable d; DevBuf<int32_t> d_r2c; DevBuf<unsigned long long> d_snp;
    d.upload(t, s); upload(d_r2c, ref_to_contig, s); upload(d_snp, snp, s);
    DevBuf<uint8_t> d_keep; DevBuf<int32_t> d_start, d_end; DevBuf<unsigned long long> d_cnt; DevBuf<unsigned> d_err;
    d_keep.alloc(std::max(1, n)); d_start.alloc(std::max(1, n)); d_end.alloc(std::max(1, n)); d_cnt.alloc(3); d_cnt.zero(s); d_err.alloc(1); d_err.zero(s);
    if (n) hipLaunchKernelGGL(k_cl_classify, dim3(blocks_for(n)), dim3(256), 0, s, n, d.flag.p, d.ref.p, d.pos.p, d.l_seq.p, d.cig_off.p, d.n_cig.p, d.cigar.p,
                              d_r2c.p, (int)t.refs.size(), rt.contig_len.p, d_keep.p, d_start.p, d_end.p, d_cnt.p, d_err.p);
    PS_HIP(hipGetLastError());
    DevBuf<int32_t> d_kidx; DevBuf<int> d_nsel; d_kidx.alloc(std::max(1, n)); d_nsel.alloc(1); d_nsel.zero(s);
    if (n) cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceSelect::Flagged(tmp, b, hipcub::CountingInputIterator<int32_t>(0), d_keep.p, d_kidx.p, d_nsel.p, n, s); });
    unsigned long long cnt[3]; unsigned err = 0; int K = 0;
    d_cnt.download(cnt, 3, s); d_err.download(&err, 1, s); d_nsel.download(&K, 1, s);
    PS_HIP(hipStreamSynchronize(s));
    if (err & kClErrContig) throw Error("ps_pileup_clusters: a record names a sequence the reference does not have");
    if (err & kClErrPastEnd) throw Error("ps_pileup_clusters: a record reaches past the end of its reference sequence");
    if (err & kClErrSeq) throw Error("ps_pileup_clusters: a mapped record has no SEQ ('*') or a CIGAR longer than its SEQ");
    if (err & kClErrLong) throw Error("ps_pileup_clusters: a record aligns 65536 bases or more");
    ps_cluster_stats &st = res.st;
    st.n_records = (uint64_t)n; st.n_unmapped = cnt[0]; st.n_skipped_indel = cnt[1]; st.n_kept = (uint64_t)K;

    // boundaries (rule 2)
    DevBuf<int32_t> d_sk, d_ek, d_rk; DevBuf<uint8_t> d_rv, d_stop, d_desync; DevBuf<uint32_t> d_head, d_seg, d_open, d_cid; DevBuf<unsigned long long> d_key, d_mx;
    const size_t Kn = std::max(1, K);
    d_sk.alloc(Kn); d_ek.alloc(Kn); d_rk.alloc(Kn); d_rv.alloc(Kn); d_stop.alloc(Kn); d_desync.alloc(Kn); d_head.alloc(Kn); d_seg.alloc(Kn);
    d_open.alloc(Kn); d_cid.alloc(Kn); d_key.alloc(Kn); d_mx.alloc(Kn);
    int C = 0;
    if (K) {
        hipLaunchKernelGGL(k_cl_gather, dim3(blocks_for(K)), dim3(256), 0, s, K, d_kidx.p, d_start.p, d_end.p, d.flag.p, d.ref.p, d_sk.p, d_ek.p, d_rv.p, d_rk.p, d_head.p);
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::InclusiveSum(tmp, b, d_head.p, d_seg.p, K, s); });
        hipLaunchKernelGGL(k_cl_key, dim3(blocks_for(K)), dim3(256), 0, s, K, d_seg.p, d_ek.p, d_key.p);
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::InclusiveScan(tmp, b, d_key.p, d_mx.p, hipcub::Max(), K, s); });
        hipLaunchKernelGGL(k_cl_open, dim3(blocks_for(K)), dim3(256), 0, s, K, d_seg.p, d_mx.p, d_sk.p, d_ek.p, d_open.p, d_stop.p, d_desync.p);
        hipLaunchKernelGGL(k_cl_fix, dim3(blocks_for(K)), dim3(256), 0, s, K, d_desync.p, d_stop.p, d_sk.p, d_ek.p, d_open.p);
        PS_HIP(hipGetLastError());
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::InclusiveSum(tmp, b, d_open.p, d_cid.p, K, s); });
        uint32_t c_last = 0;
        PS_HIP(hipMemcpyAsync(&c_last, d_cid.p + (K - 1), sizeof c_last, hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        C = (int)c_last;
    }
    st.n_clusters = (uint64_t)C;
    const size_t Cn = std::max(1, C);
    DevBuf<int32_t> d_opener, d_lo, d_hi; DevBuf<uint32_t> d_nreads, d_nrev, d_nsites, d_maxs; DevBuf<unsigned long long> d_w, d_off, d_cflags, d_ct2c, d_beyond;
    d_opener.alloc(Cn); d_lo.alloc(Cn); d_hi.alloc(Cn); d_nreads.alloc(Cn); d_nrev.alloc(Cn); d_nsites.alloc(Cn); d_maxs.alloc(Cn);
    d_w.alloc(Cn); d_off.alloc(Cn); d_cflags.alloc(Cn); d_ct2c.alloc(Cn); d_beyond.alloc(1);
    d_nreads.zero(s); d_nrev.zero(s); d_nsites.zero(s); d_cflags.zero(s); d_ct2c.zero(s); d_beyond.zero(s);
    unsigned long long total = 0;
    DevBuf<uint32_t> d_cov, d_t2c, d_sbk, d_sbk_sorted; DevBuf<unsigned long long> d_first; DevBuf<double> d_sfrac, d_sorted; DevBuf<ClOut> d_res;
    d_res.alloc(Cn);
    const int n_eval = std::max(0, C - 1);                               // the last cluster is never closed (:528-529)
    if (C) {
        hipLaunchKernelGGL(k_cl_init, dim3(blocks_for(C)), dim3(256), 0, s, C, d_lo.p, d_hi.p);
        hipLaunchKernelGGL(k_cl_members, dim3(blocks_for(K)), dim3(256), 0, s, K, d_open.p, d_cid.p, d_sk.p, d_ek.p, d_rv.p, d_opener.p, d_nreads.p, d_nrev.p, d_lo.p, d_hi.p);
        hipLaunchKernelGGL(k_cl_width, dim3(blocks_for(C)), dim3(256), 0, s, C, d_lo.p, d_hi.p, d_w.p);
        PS_HIP(hipGetLastError());
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(tmp, b, d_w.p, d_off.p, C, s); });
        unsigned long long lw = 0, lo = 0;
        PS_HIP(hipMemcpyAsync(&lw, d_w.p + (C - 1), sizeof lw, hipMemcpyDeviceToHost, s));
        PS_HIP(hipMemcpyAsync(&lo, d_off.p + (C - 1), sizeof lo, hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        total = lo + lw;
        const size_t Tn = std::max<unsigned long long>(1, total);
        d_cov.alloc(Tn); d_t2c.alloc(Tn); d_first.alloc(Tn); d_sbk.alloc(Tn); d_sbk_sorted.alloc(Tn); d_sfrac.alloc(Tn); d_sorted.alloc(Tn);
        d_cov.zero(s); d_t2c.zero(s);
        PS_HIP(hipMemsetAsync(d_first.p, 0xff, Tn * sizeof(unsigned long long), s));
        ClCountArgs a;
        a.K = K; a.kidx = d_kidx.p; a.cid = d_cid.p; a.sk = d_sk.p; a.ek = d_ek.p; a.rv = d_rv.p; a.ref = d.ref.p; a.ref_to_contig = d_r2c.p; a.contig_off = rt.contig_off.p;
        a.cig_off = d.cig_off.p; a.n_cig = d.n_cig.p; a.cigar = d.cigar.p; a.seq_off = d.seq_off.p; a.seq = d.seq.p;
        a.pac = ix.pac.p; a.hole_off = rt.hole_off.p; a.hole_len = rt.hole_len.p; a.n_holes = rt.n_holes;
        a.lo = d_lo.p; a.hi = d_hi.p; a.off = d_off.p; a.cov = d_cov.p; a.t2c = d_t2c.p; a.first = d_first.p; a.cflags = d_cflags.p; a.ct2c = d_ct2c.p; a.beyond = d_beyond.p;
        hipLaunchKernelGGL(k_cl_count, dim3(blocks_for(K)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_cl_nsites, dim3(C), dim3(64), 0, s, d_off.p, d_w.p, d_t2c.p, d_nsites.p);
        PS_HIP(hipGetLastError());
        cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceScan::InclusiveScan(tmp, b, d_nsites.p, d_maxs.p, hipcub::Max(), C, s); });
        if (n_eval) {
            if (total > (unsigned long long)INT_MAX) throw Error("ps_pileup_clusters: the cluster windows hold more than 2^31 positions");
            DevBuf<unsigned long long> d_kend, d_bend; d_kend.alloc((size_t)n_eval); d_bend.alloc((size_t)n_eval);
            ClReduceArgs r;
            r.n_eval = n_eval; r.min_cov = min_cov; r.nreads = d_nreads.p; r.maxsites = d_maxs.p; r.opener = d_opener.p; r.rk = d_rk.p;
            r.lo = d_lo.p; r.off = d_off.p; r.w = d_w.p; r.cov = d_cov.p; r.t2c = d_t2c.p; r.first = d_first.p; r.snp = d_snp.p; r.n_snp = (int)snp.size();
            r.sbk = d_sbk.p; r.sfrac = d_sfrac.p; r.kend = d_kend.p; r.bend = d_bend.p; r.out = d_res.p;
            hipLaunchKernelGGL(k_cl_reduce, dim3(n_eval), dim3(64), 0, s, r);
            PS_HIP(hipGetLastError());
            // per cluster: the kept fractions in descending order, the sites' buckets in ascending order
            const int ni = (int)total;
            cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceSegmentedRadixSort::SortKeysDescending(tmp, b, d_sfrac.p, d_sorted.p, ni, n_eval, d_off.p, d_kend.p, 0, 64, s); });
            cub_call(s, [&](void *tmp, size_t &b) { return hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, b, d_sbk.p, d_sbk_sorted.p, ni, n_eval, d_off.p, d_bend.p, 0, 32, s); });
            hipLaunchKernelGGL(k_cl_sum, dim3(n_eval), dim3(64), 0, s, n_eval, min_cov, d_nreads.p, d_off.p, d_bend.p, d_sbk_sorted.p, d_sorted.p, d_res.p);
            PS_HIP(hipGetLastError());
        }
    }
    // everything the text needs, per cluster
    std::vector<int32_t> kidx((size_t)K), opener((size_t)C), hi((size_t)C);
    std::vector<uint32_t> nreads((size_t)C), nrev((size_t)C), nsites((size_t)C);
    std::vector<unsigned long long> cflags((size_t)C), ct2c((size_t)C); std::vector<ClOut> cres((size_t)n_eval);
    unsigned long long beyond = 0;
    if (K) d_kidx.download(kidx.data(), (size_t)K, s);
    if (C) {
        d_opener.download(opener.data(), (size_t)C, s); d_hi.download(hi.data(), (size_t)C, s); d_nreads.download(nreads.data(), (size_t)C, s);
        d_nrev.download(nrev.data(), (size_t)C, s); d_nsites.download(nsites.data(), (size_t)C, s); d_cflags.download(cflags.data(), (size_t)C, s);
        d_ct2c.download(ct2c.data(), (size_t)C, s);
        if (n_eval) d_res.download(cres.data(), (size_t)n_eval, s);
    }
    d_beyond.download(&beyond, 1, s);
    PS_HIP(hipStreamSynchronize(s));
    st.n_t2c_beyond_51 = beyond;
    // crosslinked clusters in file order (:232), their read-index flags (:249-255) and the ranks' sums on the device
    std::vector<int32_t> xl; uint64_t allele_pos[51] = {0}, n_allele_pos = 0; int kmax = 0;
    for (int c = 0; c < n_eval; ++c) {
        const ClOut &r = cres[(size_t)c];
        if ((int64_t)nreads[c] < (int64_t)min_cov || r.n_kept == 0 || !(r.sum >= 0.2)) continue;
        xl.push_back(c); kmax = std::max(kmax, (int)r.n_kept);
        for (int j = 0; j < 51; ++j) if (cflags[c] >> j & 1) { ++allele_pos[j]; ++n_allele_pos; }
    }
    std::vector<double> afreq((size_t)kmax, 0.0);
    if (kmax) {
        DevBuf<int32_t> d_xl; DevBuf<double> d_acc;
        upload(d_xl, xl, s); d_acc.alloc((size_t)kmax);
        hipLaunchKernelGGL(k_cl_sitefreq, dim3(blocks_for(kmax, 64)), dim3(64 * (kSfLoaders + 1)), 0, s, d_xl.p, (int)xl.size(), d_off.p, d_res.p, d_sorted.p, kmax, d_acc.p);
        PS_HIP(hipGetLastError());
        d_acc.download(afreq.data(), (size_t)kmax, s);
        PS_HIP(hipStreamSynchronize(s));
    }
    res.ms_kernels = ms_since(t0);

    // text: the cluster and CCR sequences from the FASTA bytes (:262-343, :367-487)
    t0 = HostClock::now();
    const auto fasta = cl_read_fasta(ref_fa);
    std::vector<const std::string *> ref_seq(t.refs.size(), nullptr);
    for (size_t r = 0; r < t.refs.size(); ++r) { auto it = fasta.find(t.refs[r].first); if (it != fasta.end()) ref_seq[r] = &it->second; }
    auto seq_of = [&](int r) -> const std::string & { if (!ref_seq[(size_t)t.ref[(size_t)r]]) throw Error("ps_pileup_clusters: " + t.refs[(size_t)t.ref[(size_t)r]].first + " is not in the FASTA"); return *ref_seq[(size_t)t.ref[(size_t)r]]; };
    auto fetch = [&](int r, int64_t a, int64_t b) -> std::string {      // getSubsequenceAt(name, a, b), 1-based inclusive
        const std::string &q = seq_of(r);
        if (b > (int64_t)q.size()) throw Error("ps_pileup_clusters: the cluster sequence of a record reaches past the end of " + t.refs[(size_t)t.ref[(size_t)r]].first);
        return b < a ? std::string() : q.substr((size_t)(a - 1), (size_t)(b - a + 1));
    };
    struct Part { std::string out, fasta, tsv; uint64_t written = 0, ccr = 0, clipped = 0, past = 0, snp = 0, snv = 0, unmod = 0; std::string err; };
    const int T = std::max(1, std::min(threads, n_eval / 64 + 1));
    std::vector<Part> parts((size_t)T);
    auto work = [&](int w) {
        Part &P = parts[(size_t)w];
        try {
            const int c0 = (int)((int64_t)n_eval * w / T), c1 = (int)((int64_t)n_eval * (w + 1) / T);
            for (int c = c0; c < c1; ++c) {
                if ((int64_t)nreads[c] < (int64_t)min_cov) continue;
                const ClOut &r = cres[(size_t)c];
                const int j0 = opener[c], j1 = c + 1 < C ? opener[c + 1] : K;
                const int r0 = kidx[(size_t)j0];
                const std::string &chr = t.refs[(size_t)t.ref[(size_t)r0]].first;
                const std::string id = "cl_" + std::to_string(c + 2) + "_" + chr;
                const bool t_rev = (t.flag[(size_t)r0] & 16u) != 0;
                const char *comb = t_rev ? "-" : (nrev[c] ? "+/-" : "+");
                // the sequence: the opener's M and D elements (:367-414), then the overhang of members that end further (:421-487)
                std::string seq;
                int64_t cend = 0;
                for (int j = j0; j < j1; ++j) {
                    const int rr = kidx[(size_t)j];
                    const int64_t st_j = (int64_t)t.pos[(size_t)rr] + 1;
                    const uint32_t *cg = t.cigar.data() + t.cig_off[(size_t)rr];
                    const int64_t en_j = st_j + cigar_ref_span(cg, t.n_cig[(size_t)rr]) - 1;
                    int64_t cbs = st_j;
                    if (j == j0) {
                        for (uint32_t k = 0; k < t.n_cig[(size_t)rr]; ++k) {
                            const int op = (int)(cg[k] & 15u); const int64_t len = cg[k] >> 4;
                            if (op == 0 || op == 2) seq += fetch(rr, cbs, cbs + len - 1);
                            if (op != 1) cbs += len;
                        }
                        cend = en_j;
                    } else if (en_j > cend) {
                        for (uint32_t k = 0; k < t.n_cig[(size_t)rr]; ++k) {
                            const int op = (int)(cg[k] & 15u); const int64_t len = cg[k] >> 4;
                            if (cbs + len - 1 < cend) { if (op != 1) cbs += len; continue; }
                            if (op == 0 || op == 2) {
                                const std::string add = fetch(rr, cbs, cbs + len - 1);
                                const int64_t ov = cend - cbs + 1;
                                if (ov > 0) seq.append(add, (size_t)std::min<int64_t>(ov, len), std::string::npos);
                                else seq = add + seq;
                            }
                            cend = en_j;
                            if (op != 1) cbs += len;
                        }
                    }
                }
                if (t_rev) cl_revcomp(seq);
                P.snp += r.snp_hits; P.snv += r.snv; P.unmod += r.unmodelled;
                if (nsites[c] > 0 && r.best_pos > 0) {                  // :262-315
                    const std::string &q = seq_of(r0);
                    std::string ccr;
                    if (r.best_pos - 20 < 1) ++P.clipped;
                    else if ((int64_t)r.best_pos + 20 > (int64_t)q.size()) ++P.past;
                    else { ccr = q.substr((size_t)(r.best_pos - 21), 41); if (!std::strcmp(comb, "-")) cl_revcomp(ccr); }
                    for (char &ch : ccr) ch = (char)std::toupper((unsigned char)ch);
                    const std::string a = std::to_string(r.best_pos - 20), b = std::to_string(r.best_pos + 20);
                    P.fasta += ">" + id + " 20-anchor-20 " + chr + ":" + comb + ":" + a + "-" + b + "\n" + ccr + "\n";
                    P.tsv += "Gene\t" + id + "\t" + comb + "\t" + chr + "\t" + std::to_string(t.pos[(size_t)r0] + 1) + "\t" + std::to_string(hi[c]) + "\t" + a + "\t" + b + "\t" + ccr +
                             "\t" + std::to_string(r.best_pos) + "\t" + std::to_string(nreads[c]) + "\t" + std::to_string(nsites[c]) + "\t" + std::to_string(r.best_cnt) +
                             "\t" + java_double_to_string(r.best_val) + "\t" + std::to_string(ct2c[c]) + "\t" + java_double_to_string(r.sum) + "\n";
                    ++P.ccr;
                }
                P.out += id + "\t" + chr + "\t" + std::to_string(t.pos[(size_t)r0] + 1) + "\t" + std::to_string(hi[c]) + "\t" + (t_rev ? "-" : "+") + "\t" +
                         std::to_string(nreads[c]) + "\t" + std::to_string(ct2c[c]) + "\t" + std::to_string(nsites[c]) + "\t" +
                         java_double_to_string(r.sum) + "\t" + seq + "\t" + comb + "\t" + std::to_string(seq.size()) + "\n";
                ++P.written;
            }
        } catch (const std::exception &e) { P.err = e.what(); if (P.err.empty()) P.err = "error"; }
    };
    { std::vector<std::thread> th; for (int w = 1; w < T; ++w) th.emplace_back(work, w); work(0); for (auto &x : th) x.join(); }
    for (const Part &P : parts) if (!P.err.empty()) throw Error(P.err);
    res.out = "ClusterID\tChr\tStart\tEnd\tStrand\t#reads\t#T2C\t#T2C sites\tT2C Fraction\tSeqenece\tCombStrand\tSeqLength\n";
    res.tsv = "Protein_Group\tCluster ID\tStrand\tChromosome\tCluster_Begin\tCluster_End\tAnchor_FlankSeq_Begin\tAnchor_FlankSeq_End"
              "\tAnchor_FlankSeq\tAnchor_Position\tCluster_Clone_Count\tNumber_of_T2C_Positions\tT2C_Freq_at_Anchor_Position"
              "\tT2C_Fract_at_Anchor_Position\tT2C_Freq_Whole_Cluster\tT2C_Fract_Whole_Cluster\n";
    if (K && min_cov <= 0) { res.out += "\t\t0\t0\t+\t0\t0\t0\t0.0\t\t+\t0\n"; ++st.n_clusters_written; }   // the empty pseudo-cluster the first record closes (:180)
    for (const Part &P : parts) {
        res.out += P.out; res.fasta += P.fasta; res.tsv += P.tsv;
        st.n_clusters_written += P.written; st.n_ccr += P.ccr; st.n_ccr_clipped += P.clipped; st.n_ccr_past_end += P.past;
        st.n_snp_hits += P.snp; st.n_snv_sites += P.snv; st.n_order_unmodelled += P.unmod;
    }
    // doubleStranded (:494-498): a forward-first cluster adds one per reverse member, a reverse-first cluster nothing
    for (int c = 0; c < C; ++c) if (!(t.flag[(size_t)kidx[(size_t)opener[c]]] & 16u)) st.n_double_stranded += nrev[c];
    st.n_crosslinked = xl.size();
    res.report = "Double stranded clusters found: " + std::to_string(st.n_double_stranded) + "\nLoci found that are SNPs: 0\n" +
                 std::to_string(st.n_skipped_indel) + " insertion or deletion skipped\nT-C mutations identified as SNPs: " + std::to_string(st.n_snp_hits) +
                 "\nT-C mutations identified as SNVs (100% T-C in 1 site): " + std::to_string(st.n_snv_sites) + "\n";
    for (int k = 0; k < kmax; ++k) res.sitefreq += java_double_to_string(afreq[(size_t)k] / (double)xl.size()) + "\n";
    for (int j = 0; j < 51; ++j) res.sitepos += java_double_to_string((double)allele_pos[j] / (double)n_allele_pos) + "\n";
    res.ms_text = ms_since(t0);
}

void pileup_clusters_run(const char *mapping, const char *ref_fa, const char *out_file, const char *snp_vcf, int min_cov,
                         const char *site_prefix, int device, ps_cluster_stats *stats)
{
    if (!mapping || !ref_fa || !out_file || !out_file[0]) throw Error("ps_pileup_clusters: mapping, reference and output file are required");
    ClResult r;
    const std::string out = out_file, sp = site_prefix && site_prefix[0] ? site_prefix : mapping, ref = ref_fa;
    const std::pair<std::string, const std::string *> texts[6] = {{out, &r.out}, {out + ".ccr.fasta", &r.fasta}, {out + ".ccr.tsv", &r.tsv}, {out + ".report", &r.report},
                                                                  {sp + ".sitefrequency.tsv", &r.sitefreq}, {sp + ".sitepositions.tsv", &r.sitepos}};
    OutFiles files(".clusters-tmp");
    for (const auto &x : texts) files.add(x.first);
    files.refuse_inputs({mapping, ref_fa, (ref + ".ann").c_str(), (ref + ".pac").c_str(), snp_vcf}, "ps_pileup_clusters: ");
    pileup_clusters(mapping, ref_fa, snp_vcf, min_cov, device, 8, r);
    const auto t0 = HostClock::now();
    for (const auto &x : texts) write_text_file(files.tmp(x.first), *x.second);
    files.publish_all(); files.keep();
    r.ms_text += ms_since(t0);
    if (stats) *stats = r.st;
    if (std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip] ps_pileup_clusters: %llu records, %llu kept, %llu clusters, %llu written, %llu crosslinked; "
                             "parse %.1f ms, VCF %.1f ms, kernels %.1f ms, text %.1f ms\n",
                     (unsigned long long)r.st.n_records, (unsigned long long)r.st.n_kept, (unsigned long long)r.st.n_clusters,
                     (unsigned long long)r.st.n_clusters_written, (unsigned long long)r.st.n_crosslinked, r.ms_parse, r.ms_vcf, r.ms_kernels, r.ms_text);
}

}  // namespace ps
