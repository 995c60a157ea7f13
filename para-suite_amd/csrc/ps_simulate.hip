// ps_simulate.hip -- PAR-CLIP reads drawn from transcripts: the toolkit's `simulate` mode (include/parasuite_hip.h,
// ps_simulate_reads).
//
// Replaces bin/createSimulatedPARCLIPDataset.pl, one Perl process that walks the transcripts, their clusters, every base of the
// transcript once per cluster (the SNP pre-selection, :369-394) and every base of every read.  The rules are the Perl's; the
// random stream is this library's own and counter-based (the header states it), so every unit of work draws from its own key
// and the units can be cut any way.  The host reads the files, holds the exon maps and writes the text; the device draws:
//   k_sim_plan      one lane per transcript: selection, 1..3 clusters, their reads, position, starts, ends, bound flag and
//                   T->C sites (:265-364).  Three exclusive scans (hipCUB) number the clusters, the read slots and the
//                   positions of the SNP pass
//   k_sim_snp       the SNP pre-selection over every (cluster, transcript position) of the clusters that are not skipped, laid
//                   out flat so that a long transcript spreads over many blocks: 16 consecutive positions per lane, 4096 per
//                   block.  Run twice: once to count per block, and after a scan of the counts once more to write the records
//                   in order -- the index of a record is its snp<id>.  Only a position that is a SNP touches the transcript text
//   k_sim_reads     one lane per read slot: start and end, the per-base loop (:428-591) into 64 bytes of sequence and 64 of
//                   quality, the read's counters; the counters of the .log are summed per wave, one atomic each.  A SNP at a
//                   position is the same pure function of (cluster, position) that k_sim_snp evaluates: no table is looked up
// No libm call and no fused multiply-add below: the text must equal tests/perl_simulator.py byte for byte.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/parasuite_hip.h"
#include "ps_dev.h"

namespace ps {

// ---- the random stream (__host__ too: it can be run without a device)

__host__ __device__ inline uint64_t sim_mix(uint64_t x)                  // the finalizer of splitmix64
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; return x ^ (x >> 31);
}
__host__ __device__ inline uint64_t sim_run_key(uint64_t seed) { return sim_mix(seed + 0x9E3779B97F4A7C15ull); }
// cluster 0, read 0: the transcript's own draws; cluster 1..3, read 0: the cluster's; read i + 1: read i of that cluster
__host__ __device__ inline uint64_t sim_unit(uint64_t run, uint64_t transcript, uint32_t cluster, uint32_t read)
{
    return sim_mix(sim_mix(run ^ transcript) ^ ((uint64_t)cluster << 32 | read));
}
__host__ __device__ inline uint32_t sim_draw(uint64_t unit, uint64_t slot) { return (uint32_t)(sim_mix(unit ^ slot) >> 32); }
__host__ __device__ inline double sim_rand(uint64_t unit, uint64_t slot) { return (double)sim_draw(unit, slot) * (1.0 / 4294967296.0); }
__host__ __device__ inline int sim_floor_rand(uint64_t unit, uint64_t slot, uint32_t k) { return (int)(((uint64_t)sim_draw(unit, slot) * k) >> 32); }
__host__ __device__ inline int sim_ceil_rand(uint64_t unit, uint64_t slot, int k) { return k > 0 ? 1 + sim_floor_rand(unit, slot, (uint32_t)k) : 0; }
__host__ __device__ inline double sim_normal(uint64_t unit, uint64_t slot, double mean, double sd)
{
    uint64_t sum = 0;
    for (int i = 0; i < 12; ++i) sum += sim_draw(unit, slot + (uint64_t)i);
    const double z = (double)((int64_t)sum - (int64_t)(6ull << 32)) * (1.0 / 4294967296.0);
    const double scaled = sd * z;                                         // rounded on its own: contraction is off for this file
    return mean + scaled;
}

// slots (the same numbers as tests/perl_simulator.py)
enum : uint64_t { kTSelect = 0, kTClusters = 1 };
enum : uint64_t { kCReads = 0, kCPos = 12, kCNT2C = 13, kCNStart = 14, kCNEnd = 15, kCStarts = 16, kCEnds = 52, kCBound = 88, kCSite = 89, kCSnp = 128 };
enum : uint64_t { kRStart = 0, kREnd = 1, kRLoop = 16, kLTest = 0, kLAnyBase = 1, kLSnp = 2, kLIndel = 3, kLInsBase = 4, kLQual = 8, kLQualSnp = 20, kLQualIns = 32 };
constexpr int kSimMaxLen = 30, kSimMinLen = 7, kSimStride = 64, kSimSnpPerLane = 16, kSimSnpPerBlock = 256 * kSimSnpPerLane;

struct SimParams {
    uint64_t run;
    double select_read, snp_rate, snp_report, bound_prob;
    int allow_indels, pad_;
    double thr[4][3], freq[4], sitepos[40], qmean[31], qsd[31], ins[31], del[31];
};
enum : uint8_t { kSimAbsent = 0, kSimSkipped = 1, kSimActive = 2 };
struct SimCluster {                    // slot = transcript * 3 + cluster
    int32_t n_reads, pos, start[3], end[3], site[4];                      // site[k] has rate freq[k]
    uint8_t n_start, n_end, bound, n_sites, state, pad_[3];
};
struct SimSnp { uint32_t slot, z; uint8_t ref, alt /* 0: none, the base is no ACGT */, homozygous, reported; };
struct SimRead { int32_t start, end; uint8_t seq_len, qual_len, emitted; int8_t ins_j /* position whose iteration ran twice, -1: none */; };
enum : int { kSimReads = 0, kSimBases = 1, kSimSumLen = 2, kSimT2C = 3, kSimMut = 4, kSimIndels = 5, kSimSnps = 6, kSimLeftOut = 7, kSimNonAcgt = 8,
             kSimMostT2C = 9, kSimMostErr = 10, kSimCounters = 11 };

__host__ __device__ inline int sim_base_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
__host__ __device__ inline uint8_t sim_quality(uint64_t unit, uint64_t slot, double mean, double sd)
{
    const double v = sim_normal(unit, slot, mean, sd);
    const int q = v >= 65.0 ? 64 : (v < 3.0 ? 3 : (int)v);                // int(v) > 64 -> 64, int(v) <= 2 -> 3
    return (uint8_t)(33 + q);
}
// is position z of the cluster with key cu a SNP; mutate_base for its alternative (0 for a base that is no ACGT), its zygosity
__host__ __device__ inline bool sim_is_snp(uint64_t cu, uint32_t z, double rate) { return sim_rand(cu, kCSnp + 4ull * z) <= rate; }
__host__ __device__ inline uint8_t sim_snp_alt(uint64_t cu, uint32_t z, uint8_t ref)
{
    const int b = sim_base_code(ref);
    if (b < 0) return 0;
    const int k = sim_floor_rand(cu, kCSnp + 4ull * z + 1, 3);            // the k-th of the three other bases, in ACGT order
    return (uint8_t)"ACGT"[k + (k >= b)];
}
__host__ __device__ inline bool sim_snp_homozygous(uint64_t cu, uint32_t z) { return sim_rand(cu, kCSnp + 4ull * z + 2) <= 0.5; }

// the last index i with off[i] <= g; off ascending with n + 1 entries, off[0] <= g < off[n]
__device__ inline uint32_t sim_slot_of(const unsigned long long *off, uint32_t n, unsigned long long g)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

// ---- kernels

// n transcripts; cl, read_count and flat_len have 3 n entries (+ 1 for the scans, zeroed by the host), cl_count n (+ 1)
__global__ void __launch_bounds__(256) k_sim_plan(const SimParams *pp, uint32_t n, const uint8_t *text, const unsigned long long *seq_off,
                                                 SimCluster *cl, unsigned long long *cl_count, unsigned long long *read_count, unsigned long long *flat_len)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const SimParams &p = *pp;
    const int L = (int)(seq_off[t + 1] - seq_off[t]);
    const uint8_t *seq = text + seq_off[t];
    const uint64_t tu = sim_unit(p.run, t, 0, 0);
    const int ncl = sim_rand(tu, kTSelect) < p.select_read ? sim_ceil_rand(tu, kTClusters, 3) : 0;
    cl_count[t] = (unsigned long long)ncl;
    for (int k = 0; k < 3; ++k) {
        SimCluster c; memset(&c, 0, sizeof c);
        if (k < ncl) {
            const uint64_t cu = sim_unit(p.run, t, (uint32_t)k + 1, 0);
            c.n_reads = (int)sim_normal(cu, kCReads, 16.0, 10.0);
            c.pos = sim_ceil_rand(cu, kCPos, L - kSimMaxLen);
            c.state = c.pos < 10 || L - c.pos < kSimMaxLen ? kSimSkipped : kSimActive;
            if (c.state == kSimActive) {
                const int n_t2c = sim_ceil_rand(cu, kCNT2C, 4);
                c.n_start = (uint8_t)sim_ceil_rand(cu, kCNStart, 3);
                c.n_end = (uint8_t)sim_ceil_rand(cu, kCNEnd, 3);
                int max_start = INT_MIN, min_end = INT_MAX;
                for (int i = 0; i < c.n_start; ++i) { c.start[i] = (int)sim_normal(cu, kCStarts + 12ull * i, (double)c.pos, 1.0); max_start = max(max_start, c.start[i]); }
                for (int i = 0; i < c.n_end; ++i) { c.end[i] = (int)sim_normal(cu, kCEnds + 12ull * i, (double)(c.pos + (kSimMaxLen - kSimMinLen)), 1.0); min_end = min(min_end, c.end[i]); }
                if (sim_rand(cu, kCBound) < p.bound_prob) {
                    c.bound = 1;
                    // twelve uniforms keep a start within pos +- 6 and an end within pos + 23 +- 6: at most 35 candidates, all inside the text
                    int tpos[40], nt = 0;
                    for (int q = max_start; q < min_end && nt < 40; ++q) if (seq[q] == 'T') tpos[nt++] = q;
                    for (int s = 0; s < n_t2c && nt; ++s) {
                        int pick = 0;
                        if (nt > 1) {                                     // get_t2c_position
                            double total = 0.0;
                            for (int i = 0; i < nt; ++i) total += p.sitepos[tpos[i] - max_start];
                            const double r = sim_rand(cu, kCSite + (uint64_t)s) * total;
                            double done = 0.0; pick = nt - 1;             // the Perl's -1: the last one
                            for (int i = 0; i < nt; ++i) { done += p.sitepos[tpos[i] - max_start]; if (r <= done) { pick = i; break; } }
                        }
                        c.site[c.n_sites++] = tpos[pick];
                        for (int i = pick; i + 1 < nt; ++i) tpos[i] = tpos[i + 1];
                        --nt;
                    }
                }
            }
        }
        const size_t slot = (size_t)t * 3 + k;
        cl[slot] = c;
        read_count[slot] = c.state == kSimActive && c.n_reads > 0 ? (unsigned long long)c.n_reads : 0ull;
        flat_len[slot] = c.state == kSimActive ? (unsigned long long)L : 0ull;
    }
}

// flat position g of the SNP pass = flat_off[slot] + z.  EMIT false: block_count[block] = SNPs of the block's 4096 positions;
// EMIT true: block_count holds the exclusive scan of those, and the records go to out in the order of g
template <bool EMIT>
__global__ void __launch_bounds__(256) k_sim_snp(const SimParams *pp, uint32_t n_slots, const unsigned long long *flat_off, unsigned long long total,
                                                const uint8_t *text, const unsigned long long *seq_off, unsigned long long *block_count, SimSnp *out)
{
    using Scan = hipcub::BlockScan<unsigned, 256>;
    __shared__ typename Scan::TempStorage tmp;
    const SimParams &p = *pp;
    const unsigned long long g0 = (unsigned long long)blockIdx.x * kSimSnpPerBlock + (unsigned long long)threadIdx.x * kSimSnpPerLane;
    unsigned mask = 0;                                                    // bit i: position g0 + i is a SNP
    if (g0 < total) {
        uint32_t slot = sim_slot_of(flat_off, n_slots, g0);
        uint64_t cu = sim_unit(p.run, slot / 3, slot % 3 + 1, 0);
        for (int i = 0; i < kSimSnpPerLane && g0 + i < total; ++i) {
            const unsigned long long g = g0 + i;
            if (g >= flat_off[slot + 1]) {                                // g < total = flat_off[n_slots]: the walk ends inside the table
                do ++slot; while (g >= flat_off[slot + 1]);
                cu = sim_unit(p.run, slot / 3, slot % 3 + 1, 0);
            }
            if (sim_is_snp(cu, (uint32_t)(g - flat_off[slot]), p.snp_rate)) mask |= 1u << i;
        }
    }
    unsigned before = 0, all = 0;
    Scan(tmp).ExclusiveSum((unsigned)__popc(mask), before, all);
    if (!EMIT) { if (threadIdx.x == 0) block_count[blockIdx.x] = all; return; }
    if (!mask) return;
    unsigned long long w = block_count[blockIdx.x] + before;
    uint32_t slot = sim_slot_of(flat_off, n_slots, g0);
    for (int i = 0; i < kSimSnpPerLane; ++i) {
        if (!(mask >> i & 1u)) continue;
        const unsigned long long g = g0 + i;
        while (g >= flat_off[slot + 1]) ++slot;
        const uint32_t t = slot / 3, z = (uint32_t)(g - flat_off[slot]);
        const uint64_t cu = sim_unit(p.run, t, slot % 3 + 1, 0);
        SimSnp r;
        r.slot = slot; r.z = z; r.ref = text[seq_off[t] + z]; r.alt = sim_snp_alt(cu, z, r.ref);
        r.homozygous = sim_snp_homozygous(cu, z); r.reported = sim_rand(cu, kCSnp + 4ull * z + 3) <= p.snp_report;
        out[w++] = r;
    }
}

__device__ __forceinline__ void sim_wave_add(unsigned v, unsigned long long *dst)
{
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(dst, (unsigned long long)v);
}
__device__ __forceinline__ void sim_wave_max(unsigned v, unsigned long long *dst)
{
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_down(v, o, 64));
    if ((threadIdx.x & 63u) == 0u && v) atomicMax(dst, (unsigned long long)v);
}

// n_reads read slots; read slot r belongs to the cluster slot with read_off[slot] <= r < read_off[slot + 1] and is its read
// r - read_off[slot].  seq and qual: kSimStride bytes per read slot.  Every lane of a wave reaches the sums.
__global__ void __launch_bounds__(256) k_sim_reads(const SimParams *pp, uint32_t n_slots, const unsigned long long *read_off, unsigned long long n_reads,
                                                  const SimCluster *cl, const uint8_t *text, const unsigned long long *seq_off,
                                                  SimRead *reads, uint8_t *seq_out, uint8_t *qual_out, unsigned long long *cnt)
{
    const SimParams &p = *pp;
    const unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned c_reads = 0, c_bases = 0, c_len = 0, c_t2c = 0, c_mut = 0, c_indels = 0, c_snps = 0, c_left = 0, c_other = 0, read_t2c = 0, read_err = 0;
    if (r < n_reads) {
        const uint32_t slot = sim_slot_of(read_off, n_slots, r);
        const uint32_t t = slot / 3, i = (uint32_t)(r - read_off[slot]);
        const SimCluster c = cl[slot];
        const uint64_t cu = sim_unit(p.run, t, slot % 3 + 1, 0), ru = sim_unit(p.run, t, slot % 3 + 1, i + 1);
        SimRead out; memset(&out, 0, sizeof out);
        out.ins_j = -1;
        const int start = c.start[sim_floor_rand(ru, kRStart, c.n_start)], end = c.end[sim_floor_rand(ru, kREnd, c.n_end)];
        out.start = start; out.end = end;
        if (end - start > kSimMaxLen || start >= end) c_left = 1;
        else {
            const uint8_t *wt = text + seq_off[t] + start;               // start >= pos - 6 >= 4, end <= pos + 29 < the transcript's length
            uint8_t *sq = seq_out + r * kSimStride, *ql = qual_out + r * kSimStride;
            const int len = end - start;
            int ns = 0, nq = 0; bool indel_set = false;
            auto put_seq = [&](uint8_t ch) { if (ns < kSimStride) sq[ns++] = ch; };
            auto put_qual = [&](uint8_t ch) { if (nq < kSimStride) ql[nq++] = ch; };
            c_len = (unsigned)len;
            for (int j = 0, it = 0; j < len; ++it) {
                const uint64_t base = kRLoop + 64ull * it;
                const uint8_t cur = wt[j];
                const double test = sim_rand(ru, base + kLTest), qm = p.qmean[j], qs = p.qsd[j];
                int site = -1;
                for (int s = 0; s < c.n_sites; ++s) if (c.site[s] == start + j) site = s;
                if (site >= 0) {                                          // a T->C site of a bound cluster
                    if (p.freq[site] > test) { put_seq('C'); ++c_t2c; ++read_t2c; } else put_seq(cur);
                    put_qual(sim_quality(ru, base + kLQual, qm, qs));
                    ++j; continue;
                }
                int row = sim_base_code(cur), here = row;
                if (row < 0) { ++c_other; row = sim_floor_rand(ru, base + kLAnyBase, 4); here = 0; }
                if (sim_is_snp(cu, (uint32_t)(start + j), p.snp_rate)) {
                    const double pass = sim_snp_homozygous(cu, (uint32_t)(start + j)) ? 1.0 : 0.5;
                    if (sim_rand(ru, base + kLSnp) <= pass) {             // an extra quality, and the alternative where there is one
                        put_qual(sim_quality(ru, base + kLQualSnp, qm, qs));
                        const uint8_t alt = sim_snp_alt(cu, (uint32_t)(start + j), cur);
                        if (alt) put_seq(alt);
                        ++c_snps;
                    }
                }
                put_qual(sim_quality(ru, base + kLQual, qm, qs));
                if (!(test < p.thr[row][0])) {
                    const int k = test < p.thr[row][1] ? 1 : (test < p.thr[row][2] ? 2 : 3);
                    put_seq((uint8_t)"ACGT"[(here + k) & 3]);
                    ++c_mut; ++read_err; read_t2c += k == 2;              // the Perl's count, :538
                    ++j; continue;
                }
                put_seq(cur);
                if (p.allow_indels) {
                    const double test_indel = sim_rand(ru, base + kLIndel);
                    if (!indel_set && test_indel <= p.ins[j]) {
                        put_qual(sim_quality(ru, base + kLQualIns, qm, qs));
                        put_seq((uint8_t)"ACGT"[sim_floor_rand(ru, base + kLInsBase, 4)]);
                        ++c_indels; indel_set = true; out.ins_j = (int8_t)j;
                        continue;                                         // position j again
                    }
                    if (!indel_set && test_indel <= p.del[j]) { ++c_indels; indel_set = true; ++j; continue; }
                }
                ++c_bases; ++j;
            }
            out.seq_len = (uint8_t)ns; out.qual_len = (uint8_t)nq; out.emitted = 1; c_reads = 1;
        }
        reads[r] = out;
    }
    sim_wave_add(c_reads, cnt + kSimReads); sim_wave_add(c_bases, cnt + kSimBases); sim_wave_add(c_len, cnt + kSimSumLen);
    sim_wave_add(c_t2c, cnt + kSimT2C); sim_wave_add(c_mut, cnt + kSimMut); sim_wave_add(c_indels, cnt + kSimIndels);
    sim_wave_add(c_snps, cnt + kSimSnps); sim_wave_add(c_left, cnt + kSimLeftOut); sim_wave_add(c_other, cnt + kSimNonAcgt);
    sim_wave_max(read_t2c, cnt + kSimMostT2C); sim_wave_max(read_err, cnt + kSimMostErr);
}

// ---- host side

namespace {

using Text = std::string;

Text sim_read_file(const std::string &who, const char *path) { try { return read_whole_file(path); } catch (const std::exception &e) { throw Error(who + e.what()); } }
// <FH> and chomp: lines end at "\n" only, a last line without one counts
std::vector<Text> sim_lines(const Text &data)
{
    std::vector<Text> out;
    for (size_t b = 0; b < data.size();) {
        size_t e = data.find('\n', b);
        if (e == Text::npos) e = data.size();
        out.emplace_back(data, b, e - b);
        b = e + 1;
    }
    return out;
}
inline bool sim_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }
inline bool sim_digit(char c) { return c >= '0' && c <= '9'; }
// a string in numeric context: the decimal number it starts with, 0 without one (a "\r" behind it is not looked at)
double sim_num(const Text &s)
{
    size_t i = 0;
    while (i < s.size() && sim_ws(s[i])) ++i;
    const size_t b = i;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
    size_t d = i;
    while (d < s.size() && sim_digit(s[d])) ++d;
    if (d > i) { i = d; if (i < s.size() && s[i] == '.') { ++i; while (i < s.size() && sim_digit(s[i])) ++i; } }
    else if (i + 1 < s.size() && s[i] == '.' && sim_digit(s[i + 1])) { ++i; while (i < s.size() && sim_digit(s[i])) ++i; }
    else return 0.0;
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        size_t e = i + 1;
        if (e < s.size() && (s[e] == '+' || s[e] == '-')) ++e;
        if (e < s.size() && sim_digit(s[e])) { while (e < s.size() && sim_digit(s[e])) ++e; i = e; }
    }
    return std::strtod(s.substr(b, i - b).c_str(), nullptr);
}
// split('\s+', line): a leading empty field stays, trailing ones are dropped
std::vector<Text> sim_split_ws(const Text &line)
{
    std::vector<Text> f; size_t i = 0, b = 0;
    for (;;) {
        while (i < line.size() && !sim_ws(line[i])) ++i;
        f.emplace_back(line, b, i - b);
        if (i >= line.size()) break;
        while (i < line.size() && sim_ws(line[i])) ++i;
        b = i;
    }
    while (!f.empty() && f.back().empty()) f.pop_back();
    return f;
}
std::vector<Text> sim_split(const Text &s, char sep)                      // trailing empty fields dropped, as Perl's split does
{
    std::vector<Text> f; size_t b = 0;
    for (size_t i = 0; i <= s.size(); ++i) if (i == s.size() || s[i] == sep) { f.emplace_back(s, b, i - b); b = i + 1; }
    while (!f.empty() && f.back().empty()) f.pop_back();
    return f;
}
inline double sim_field(const std::vector<Text> &f, size_t k) { return k < f.size() ? sim_num(f[k]) : 0.0; }

struct SimTranscript { Text f0, f1, chrom; std::vector<int64_t> starts, lens; int64_t total = 0; double strand = 0; };
// $genomic_positions[idx]
int64_t sim_gp(const SimTranscript &t, int64_t idx)
{
    if (t.strand == -1) idx = t.total - 1 - idx;
    for (size_t e = 0; e < t.starts.size(); ++e) { if (idx < t.lens[e]) return t.starts[e] + idx; idx -= t.lens[e]; }
    throw Error("ps_simulate_reads: a position outside the exons");
}
bool sim_int(const Text &s, int64_t &v)
{
    size_t i = s.size() && (s[0] == '+' || s[0] == '-') ? 1 : 0;
    if (s.size() == i || s.size() - i > 18) return false;
    for (size_t k = i; k < s.size(); ++k) if (!sim_digit(s[k])) return false;
    v = std::strtoll(s.c_str(), nullptr, 10);
    return true;
}
void sim_parse_header(const std::string &who, const Text &header, uint64_t seq_len, SimTranscript &t)
{
    const std::vector<Text> f = sim_split(header, '|');
    const Text name = header.substr(1);
    if (f.size() < 6) throw Error(who + "transcript " + name + ": the header has " + std::to_string(f.size()) + " '|' fields, 6 are needed");
    auto bounds = [&](const Text &text) {
        std::vector<int64_t> v;
        for (const Text &piece : sim_split(text, ';')) {
            int64_t x;
            if (!sim_int(piece, x)) throw Error(who + "transcript " + name + ": exon bound '" + piece + "' is not an integer");
            v.push_back(x);
        }
        std::sort(v.begin(), v.end());
        return v;
    };
    const std::vector<int64_t> starts = bounds(f[3]), ends = bounds(f[4]);
    if (starts.size() != ends.size() || starts.empty())
        throw Error(who + "transcript " + name + ": " + std::to_string(starts.size()) + " exon starts and " + std::to_string(ends.size()) + " exon ends");
    t.f0 = f[0]; t.f1 = f[1]; t.chrom = f[2]; t.starts = starts; t.lens.resize(starts.size()); t.total = 0; t.strand = sim_num(f.back());
    for (size_t e = 0; e < starts.size(); ++e) { t.lens[e] = std::max<int64_t>(0, ends[e] - starts[e] + 1); t.total += t.lens[e]; }
    if (t.total < (int64_t)seq_len)
        throw Error(who + "transcript " + name + ": the exons hold " + std::to_string(t.total) + " positions, the sequence has " + std::to_string(seq_len));
}

void sim_load_profiles(const std::string &who, const ps_simulate_opts &o, SimParams &p)
{
    auto need = [&](const char *path, size_t have, size_t want) {
        if (have < want) throw Error(who + path + " has " + std::to_string(have) + " lines, " + std::to_string(want) + " are needed");
    };
    const std::vector<Text> rows = sim_lines(sim_read_file(who, o.error_profile));
    need(o.error_profile, rows.size(), 4);
    for (int run = 0; run < 4; ++run) {
        const std::vector<Text> f = sim_split_ws(rows[run]);
        double v[4];
        for (int k = 0; k < 4; ++k) v[k] = sim_field(f, k);
        double no_error = v[(run + 1) % 4] + v[(run + 2) % 4];
        no_error = no_error + v[(run + 3) % 4];
        v[run] = 1 - no_error;
        p.thr[run][0] = v[run];
        p.thr[run][1] = p.thr[run][0] + v[(run + 1) % 4];
        p.thr[run][2] = p.thr[run][1] + v[(run + 2) % 4];
    }
    const std::vector<Text> freq = sim_lines(sim_read_file(who, o.t2c_profile));
    need(o.t2c_profile, freq.size(), 4);
    for (int k = 0; k < 4; ++k) p.freq[k] = sim_num(freq[k]);
    const std::vector<Text> pos = sim_lines(sim_read_file(who, o.t2c_positions));
    need(o.t2c_positions, pos.size(), 40);
    for (int k = 0; k < 40; ++k) p.sitepos[k] = sim_num(pos[k]);
    const std::vector<Text> qual = sim_lines(sim_read_file(who, o.quality_dist));
    need(o.quality_dist, qual.size(), 31);
    for (int k = 0; k < 31; ++k) { const std::vector<Text> f = sim_split(qual[k], '\t'); p.qmean[k] = sim_field(f, 0); p.qsd[k] = sim_field(f, 1); }
    for (int k = 0; k < 31; ++k) p.ins[k] = p.del[k] = 0.0;
    if (p.allow_indels) {
        const std::vector<Text> ind = sim_lines(sim_read_file(who, o.indel_profile));
        need(o.indel_profile, ind.size(), 31);
        for (int k = 0; k < 31; ++k) { const std::vector<Text> f = sim_split_ws(ind[k]); p.ins[k] = sim_field(f, 0); p.del[k] = sim_field(f, 1); }
    }
}

Text sim_perl_num(double v) { char b[40]; std::snprintf(b, sizeof b, "%.15g", v); return b; }

void sim_scan(hipStream_t s, const DevBuf<unsigned long long> &in, DevBuf<unsigned long long> &out)
{
    out.alloc(in.n);
    cub_call(s, [&](void *tmp, size_t &bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in.p, out.p, (int)in.n, s); });
}

}  // namespace

void simulate_run(const ps_simulate_opts &o, int device, ps_simulate_stats *stats)
{
    using clk = HostClock;
    const std::string who = "ps_simulate_reads: ";
    for (const char *a : {o.transcripts_fa, o.out_prefix, o.error_profile, o.t2c_profile, o.t2c_positions, o.quality_dist, o.indel_profile})
        if (!a || !a[0]) throw Error(who + "the transcript file, the output prefix and the five profile files are required");
    require_device(device);                                                // before the files are read
    const auto t_all = clk::now();
    ps_simulate_stats st{};
    SimParams P; std::memset(&P, 0, sizeof P);
    P.run = sim_run_key(o.seed);
    P.select_read = o.select_read <= 0 ? 0.216 : o.select_read;
    P.snp_rate = o.snp_rate < 0 ? 0.01 : o.snp_rate;
    P.snp_report = o.snp_report < 0 ? 0.8 : o.snp_report;
    P.bound_prob = o.bound_prob;
    P.allow_indels = o.allow_indels < 0 ? 1 : (o.allow_indels != 0);

    // ---- the inputs: profiles, then the transcripts as one text with offsets; every transcript but the last is checked
    auto t0 = clk::now();
    sim_load_profiles(who, o, P);
    std::vector<Text> headers; std::vector<uint8_t> text; std::vector<unsigned long long> seq_off;
    {
        const Text fa = sim_read_file(who, o.transcripts_fa);
        text.reserve(fa.size());
        for (size_t b = 0; b < fa.size();) {
            size_t e = fa.find('\n', b);
            if (e == Text::npos) e = fa.size();
            if (fa[b] == '>' && e > b) { headers.emplace_back(fa, b, e - b); seq_off.push_back(text.size()); }
            else if (!headers.empty()) text.insert(text.end(), fa.begin() + b, fa.begin() + e);
            b = e + 1;
        }
        seq_off.push_back(text.size());
    }
    st.n_transcripts = headers.size();
    const size_t n = headers.empty() ? 0 : headers.size() - 1;             // createReads runs when the NEXT header arrives (:203-218)
    if (n > (size_t)(INT_MAX / 4)) throw Error(who + "more than 2^29 transcripts in " + o.transcripts_fa);
    std::vector<SimTranscript> tr(n);
    for (size_t t = 0; t < n; ++t) {
        const unsigned long long len = seq_off[t + 1] - seq_off[t];
        if (len > (unsigned long long)(INT_MAX / 8)) throw Error(who + "transcript " + headers[t].substr(1) + " is longer than 2^28 bases");
        sim_parse_header(who, headers[t], len, tr[t]);
    }
    if (!n) throw Error(who + "no read was drawn from " + o.transcripts_fa + ": the last transcript of a file is never simulated");
    st.s_read = ms_since(t0) / 1e3;

    StreamGuard sg; hipStream_t s = sg.s;
    const uint32_t n_slots = (uint32_t)(3 * n);
    DevBuf<SimParams> d_par; d_par.alloc(1); d_par.upload(&P, 1, s);
    DevBuf<uint8_t> d_text; upload(d_text, text, s);
    DevBuf<unsigned long long> d_seq_off; upload(d_seq_off, seq_off, s);
    DevBuf<SimCluster> d_cl; d_cl.alloc(n_slots);
    DevBuf<unsigned long long> d_cl_count, d_read_count, d_flat_len, d_cl_base, d_read_off, d_flat_off;
    d_cl_count.alloc(n + 1); d_read_count.alloc(n_slots + 1); d_flat_len.alloc(n_slots + 1);
    d_cl_count.zero(s); d_read_count.zero(s); d_flat_len.zero(s);          // entry n of each stays 0: the scans put the totals there

    // ---- plan
    double ms = timed(s, [&] {
        hipLaunchKernelGGL(k_sim_plan, dim3(blocks_for(n)), dim3(256), 0, s, d_par.p, (uint32_t)n, d_text.p, d_seq_off.p, d_cl.p, d_cl_count.p, d_read_count.p, d_flat_len.p);
        PS_HIP(hipGetLastError());
    });
    t0 = clk::now();
    sim_scan(s, d_cl_count, d_cl_base); sim_scan(s, d_read_count, d_read_off); sim_scan(s, d_flat_len, d_flat_off);
    std::vector<SimCluster> cl(n_slots); std::vector<unsigned long long> cl_base(n + 1), read_off(n_slots + 1);
    unsigned long long flat_total = 0;
    d_cl.download(cl.data(), n_slots, s); d_cl_base.download(cl_base.data(), n + 1, s); d_read_off.download(read_off.data(), n_slots + 1, s);
    PS_HIP(hipMemcpyAsync(&flat_total, d_flat_off.p + n_slots, sizeof flat_total, hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    st.s_plan = (ms + ms_since(t0)) / 1e3;
    const unsigned long long n_read_slots = read_off[n_slots];
    st.n_clusters = cl_base[n]; st.n_snp_positions = flat_total;
    if (flat_total / kSimSnpPerBlock >= (unsigned long long)INT_MAX || n_read_slots / 256 >= (unsigned long long)INT_MAX)
        throw Error(who + "too much work for one call: " + std::to_string(flat_total) + " SNP positions, " + std::to_string(n_read_slots) + " reads");

    // ---- SNP pre-selection: count per block, scan, write in order
    const unsigned snp_blocks = (unsigned)((flat_total + kSimSnpPerBlock - 1) / kSimSnpPerBlock);
    DevBuf<unsigned long long> d_blk, d_blk_off; DevBuf<SimSnp> d_snp; std::vector<SimSnp> snps;
    if (snp_blocks) {
        d_blk.alloc((size_t)snp_blocks + 1); d_blk.zero(s);
        double ms_kernels = 0;
        ms = ms_kernels = timed(s, [&] {
            hipLaunchKernelGGL(k_sim_snp<false>, dim3(snp_blocks), dim3(256), 0, s, d_par.p, n_slots, d_flat_off.p, flat_total, d_text.p, d_seq_off.p, d_blk.p, (SimSnp *)nullptr);
            PS_HIP(hipGetLastError());
        });
        t0 = clk::now();
        sim_scan(s, d_blk, d_blk_off);
        unsigned long long n_snp = 0;
        PS_HIP(hipMemcpyAsync(&n_snp, d_blk_off.p + snp_blocks, sizeof n_snp, hipMemcpyDeviceToHost, s));
        PS_HIP(hipStreamSynchronize(s));
        ms += ms_since(t0);
        if (n_snp > (unsigned long long)UINT_MAX) throw Error(who + "more than 2^32 SNPs");
        snps.resize((size_t)n_snp);
        if (n_snp) {
            d_snp.alloc((size_t)n_snp);
            const double ms_emit = timed(s, [&] {
                hipLaunchKernelGGL(k_sim_snp<true>, dim3(snp_blocks), dim3(256), 0, s, d_par.p, n_slots, d_flat_off.p, flat_total, d_text.p, d_seq_off.p, d_blk_off.p, d_snp.p);
                PS_HIP(hipGetLastError());
            });
            ms += ms_emit; ms_kernels += ms_emit;
            t0 = clk::now();
            d_snp.download(snps.data(), snps.size(), s); PS_HIP(hipStreamSynchronize(s));
            ms += ms_since(t0);
        }
        st.s_snp = ms / 1e3; st.s_snp_kernels = ms_kernels / 1e3;
    }
    st.n_snps_preselected = snps.size();

    // ---- reads
    std::vector<SimRead> reads((size_t)n_read_slots); std::vector<uint8_t> seq_out((size_t)n_read_slots * kSimStride), qual_out((size_t)n_read_slots * kSimStride);
    unsigned long long cnt[kSimCounters] = {};
    if (n_read_slots) {
        DevBuf<SimRead> d_reads; DevBuf<uint8_t> d_sq, d_ql; DevBuf<unsigned long long> d_cnt;
        d_reads.alloc(reads.size()); d_sq.alloc(seq_out.size()); d_ql.alloc(qual_out.size()); d_cnt.alloc(kSimCounters); d_cnt.zero(s);
        ms = timed(s, [&] {
            hipLaunchKernelGGL(k_sim_reads, dim3(blocks_for((size_t)n_read_slots)), dim3(256), 0, s, d_par.p, n_slots, d_read_off.p, n_read_slots, d_cl.p, d_text.p, d_seq_off.p,
                               d_reads.p, d_sq.p, d_ql.p, d_cnt.p);
            PS_HIP(hipGetLastError());
        });
        t0 = clk::now();
        d_reads.download(reads.data(), reads.size(), s); d_sq.download(seq_out.data(), seq_out.size(), s); d_ql.download(qual_out.data(), qual_out.size(), s);
        d_cnt.download(cnt, kSimCounters, s);
        PS_HIP(hipStreamSynchronize(s));
        st.s_reads = (ms + ms_since(t0)) / 1e3;
    }
    st.n_reads = cnt[kSimReads]; st.n_bases_simulated = cnt[kSimBases]; st.sum_read_length = cnt[kSimSumLen]; st.n_t2c = cnt[kSimT2C];
    st.n_errors = cnt[kSimMut]; st.n_indels = cnt[kSimIndels]; st.n_snps = cnt[kSimSnps]; st.n_reads_skipped = cnt[kSimLeftOut];
    st.n_non_acgt = cnt[kSimNonAcgt]; st.most_t2c = cnt[kSimMostT2C]; st.most_errors = cnt[kSimMostErr];
    if (!st.n_reads) throw Error(who + "no read was drawn from " + o.transcripts_fa + " (the Perl divides by zero here)");

    // ---- the text, in transcript, cluster, read order
    t0 = clk::now();
    Text fastq, clusters, vsf = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", err;
    fastq.reserve(reads.size() * 160);
    size_t snp_at = 0; unsigned long long err_entries = 0;
    for (size_t t = 0; t < n; ++t) {
        const SimTranscript &T = tr[t];
        int cluster_index = 1;
        for (int k = 0; k < 3; ++k) {
            const size_t slot = t * 3 + k; const SimCluster &c = cl[slot];
            if (c.state == kSimAbsent) break;
            st.n_selected += k == 0;
            if (c.state == kSimSkipped) { ++st.n_clusters_skipped; continue; }
            int64_t cs = sim_gp(T, *std::min_element(c.start, c.start + c.n_start)), ce = sim_gp(T, *std::max_element(c.end, c.end + c.n_end));
            if (T.strand == -1) std::swap(cs, ce);
            clusters += "cl_" + std::to_string(cl_base[t] + k + 1) + "\tchr" + T.chrom + "\t" + std::to_string(cs) + "\t" + std::to_string(ce) + "\t" + (c.bound ? "1" : "0") + "\n";
            for (; snp_at < snps.size() && snps[snp_at].slot == slot; ++snp_at) {
                const SimSnp &v = snps[snp_at];
                if (!v.reported) continue;
                ++st.n_snps_reported;
                vsf += T.chrom + "\t" + std::to_string(sim_gp(T, v.z)) + "\tsnp" + std::to_string(snp_at + 1) + "\t" + (char)v.ref + "\t";
                if (v.alt) vsf += (char)v.alt;
                vsf += "\t.\t.\t.\n";
            }
            const Text name_head = "@SEQ_ID:" + T.f0 + "|" + T.f1 + "|" + T.chrom + "|", name_tail = std::string("|") + (c.bound ? "1" : "0") + "-" + std::to_string(cluster_index) + ":";
            for (int i = 0; i < c.n_reads; ++i) {
                const size_t r = (size_t)read_off[slot] + i; const SimRead &R = reads[r];
                if (!R.emitted) continue;
                const uint8_t *wt = text.data() + seq_off[t] + R.start;
                for (int j = 0; j < R.end - R.start; ++j) {
                    if (sim_base_code(wt[j]) >= 0) continue;
                    for (int rep = 0; rep < (R.ins_j == j ? 2 : 1); ++rep) {
                        err += "unrecognized base in ACGT_hash="; err += (char)wt[j]; err += "\nSequence_header=" + headers[t] + "\nSequence=";
                        err.append((const char *)text.data() + seq_off[t], (size_t)(seq_off[t + 1] - seq_off[t])); err += "\n";
                        ++err_entries;
                    }
                }
                int64_t a, b;
                if (T.strand == 1) { a = sim_gp(T, R.start); b = sim_gp(T, R.end); } else { a = sim_gp(T, R.end) + 1; b = sim_gp(T, R.start) + 1; }
                fastq += name_head + std::to_string(a) + "|" + std::to_string(b) + name_tail + std::to_string(i) + "\n";
                fastq.append((const char *)seq_out.data() + r * kSimStride, R.seq_len); fastq += "\n+\n";
                fastq.append((const char *)qual_out.data() + r * kSimStride, R.qual_len); fastq += "\n";
            }
            ++cluster_index;
        }
    }
    if (snp_at != snps.size() || err_entries != st.n_non_acgt) throw Error(who + "internal: the device's records do not add up");
    st.avg_read_length = (double)st.sum_read_length / (double)st.n_reads;
    st.avg_reads_per_cluster = (double)st.n_reads / (double)st.n_clusters;
    const Text log = "number reads generated: " + std::to_string(st.n_reads) + "\nnumber bases simulated: " + std::to_string(st.n_bases_simulated) +
                     "\naverage read-length: " + sim_perl_num(st.avg_read_length) + "\nnumber clusters generated: " + std::to_string(st.n_clusters) +
                     "\naverage reads per cluster: " + sim_perl_num(st.avg_reads_per_cluster) + "\nT2C mutations occured: " + std::to_string(st.n_t2c) +
                     "\nsequencing errors occured: " + std::to_string(st.n_errors) + "\nread with most T2C: " + std::to_string(st.most_t2c) +
                     "\nread with most errors: " + std::to_string(st.most_errors) + "\nnumber indels generated: " + std::to_string(st.n_indels) +
                     "\nnumer snps generated: " + std::to_string(st.n_snps) + "\n\nSome parameters:\nselect_prob=" + sim_perl_num(P.select_read) +
                     "\nread bound by RBP probability: " + sim_perl_num(P.bound_prob) + "\n";
    {
        OutFiles files(".sim-tmp"); const std::string prefix = o.out_prefix;      // the five outputs: renamed together, or all removed
        const std::pair<const char *, const Text *> texts[5] = {{".fastq", &fastq}, {".clusters", &clusters}, {"_snps.vsf", &vsf}, {".log", &log}, {".err", &err}};
        try { for (const auto &x : texts) write_text_file(files.add(prefix + x.first), *x.second); files.publish_all(); files.keep(); }
        catch (const std::exception &e) { throw Error(who + e.what()); }
    }
    st.s_write = ms_since(t0) / 1e3; st.s_total = ms_since(t_all) / 1e3;
    if (stats) *stats = st;
    if (std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip] ps_simulate_reads: %llu transcripts, %llu selected, %llu clusters (%llu skipped), %llu reads (%llu left out), "
                             "%llu SNPs over %llu positions (%llu reported); read %.3f s, plan %.3f s, SNP pass %.3f s (kernels %.2f ms), reads %.3f s, text %.3f s, total %.3f s\n",
                     (unsigned long long)st.n_transcripts, (unsigned long long)st.n_selected, (unsigned long long)st.n_clusters, (unsigned long long)st.n_clusters_skipped,
                     (unsigned long long)st.n_reads, (unsigned long long)st.n_reads_skipped, (unsigned long long)st.n_snps_preselected, (unsigned long long)st.n_snp_positions,
                     (unsigned long long)st.n_snps_reported, st.s_read, st.s_plan, st.s_snp, st.s_snp_kernels * 1e3, st.s_reads, st.s_write, st.s_total);
}

}  // namespace ps
