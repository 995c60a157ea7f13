// ps_profile.hip -- error-profile estimation from the first mapping pass.
//
// Replaces utils.errorprofile.ErrorProfiling.inferErrorProfile (/root/reference/src/src/utils/errorprofile/
// ErrorProfiling.java:100-631; counting loop :145-409, output :504-531 and :545-591), the single-threaded stage between
// the two mapping passes of a `--refine` run (Main.java:320-340).  Same counts, same two files (ps_error_profile_full adds
// the other four of the Java's `error` mode: k_profile<Q>, k_qual_sd, error_profile_write_extra):
//   <mapping>.errorprofile  four lines, row = reference base A C G T, column = read base, P(read | ref) pooled over the
//                           positions, in READ orientation, every value Double.toString + TAB (NaN for a base never seen)
//   <mapping>.indelprofile  "<ins>\t<del>", no newline: the mean over the alignment columns with a non-zero rate of
//                           (gaps starting at the column) / (bases counted at that read position)
// The records are parsed on the host (SAM text or BAM: ps_bam.cpp), the counting is one kernel over the records (one
// record per lane, block-level histograms in LDS, 64-bit totals in HBM), the reference comes from the index's packed
// forward strand + its hole table (a hole = any non-ACGT letter of the FASTA: never counted, as in the Java where
// calculateArrayPos returns -1 for it, :634-664).  Quirks of the Java that are kept because they shape the numbers:
// positions are columns of the alignment as rebuilt from the CIGAR only when read and reference span differ in length
// (:196-290; equal-length spans are compared base by base whatever the CIGAR says), an insertion's own bases and a
// deletion's reference bases are never counted, gap counts are booked at column (columns so far + q), q = 1..length,
// in forward-strand coordinates while the base counts they are divided by are in read orientation (:247-272, :553-570).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include "ps_dev.h"
#include "ps_java.h"
#include "ps_pacref.h"

namespace ps {

struct ProfArgs {
    const int32_t *ref_off_lo; const int32_t *ref_off_hi;   // per record: global start on the packed forward strand (64-bit as two words), < 0 hi: skip
    const int32_t *l_seq; const uint32_t *flag; const uint32_t *cig_off; const uint32_t *n_cig; const uint32_t *cigar;
    const uint64_t *seq_off; const uint8_t *seq;
    const uint8_t *pac; const int64_t *hole_off; const int32_t *hole_len; int n_holes;
    int n_records, max_len;
    unsigned long long *conv, *ins, *del, *stat;              // stat: processed, indel reads, skipped, too long; Q >= 1: without QUAL, QUAL index beyond the read
    const uint8_t *qual;                                      // Q >= 1: Phred byte of base j at seq_off + j
    unsigned long long *qpm;                                  // Q >= 1: 16 QUAL sums, then 16 pair counts ([ref base * 4 + read base])
    unsigned long long *qpos; int32_t *n_q;                   // Q == 2: max_len QUAL sums, then max_len counts; per record: positions booked
};

constexpr int kQpmReps = 8;           // copies of the 16 .qualityPerMismatch sums / counts in LDS: every pair of a block lands on 16 words

__host__ __device__ constexpr size_t prof_lds_bytes(int Q, int max_len)
{
    return Q == 0 ? (size_t)max_len * 18 * 4 : (size_t)(((size_t)max_len * (Q == 2 ? 20 : 18) + 1) & ~(size_t)1) * 4 + (size_t)kQpmReps * 16 * 12;
}
int profile_max_len(int quals)
{
    int m = 1;
    while (m < 4096 && prof_lds_bytes(quals, m + 1) <= 160 * 1024) ++m;
    return m;
}

// one record per lane.  col = column of the rebuilt alignment (forward strand); a counted pair goes to position
// strand ? width-1-col : col with both bases complemented on the reverse strand (ErrorProfiling.java:301-306).
// Q (compile time, so the launches of the mapper's two files carry none of it): 1 also books .qualityPerMismatch -- QUAL[p]
// of every pair at read position p of a record whose CIGAR has no I and no D (:379-390), QUAL taken in SAM order, never
// reversed (:301 reads it before the reverse-complement at :313); p >= L (reverse-strand N records) is left out and counted --
// 2 also books QUAL[i] at every position i < L of every counted record with QUAL (:402-406 book i < width and fail at i = L)
template <int Q>
__global__ void __launch_bounds__(256) k_profile(ProfArgs a)
{
    extern __shared__ unsigned int sm[];
    unsigned int *s_conv = sm, *s_ins = sm + a.max_len * 16, *s_del = s_ins + a.max_len;
    unsigned int *s_qsum = s_del + a.max_len, *s_qcnt = s_qsum + a.max_len;                        // Q == 2
    const int n_words = a.max_len * (Q == 2 ? 20 : 18);
    unsigned long long *s_qpm = reinterpret_cast<unsigned long long *>(sm + ((n_words + 1) & ~1));  // Q >= 1: kQpmReps x 16 sums
    unsigned int *s_qpc = reinterpret_cast<unsigned int *>(s_qpm + kQpmReps * 16);                 // kQpmReps x 16 counts
    for (int i = threadIdx.x; i < n_words; i += blockDim.x) sm[i] = 0;
    if (Q) for (int i = threadIdx.x; i < kQpmReps * 16; i += blockDim.x) { s_qpm[i] = 0; s_qpc[i] = 0; }
    __syncthreads();
    unsigned long long n_proc = 0, n_indel = 0, n_skip = 0, n_long = 0, n_noq = 0, n_beyond = 0;
    const int rep = (int)(threadIdx.x & (kQpmReps - 1)) * 16;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.n_records; r += gridDim.x * blockDim.x) {
        if (Q == 2) a.n_q[r] = 0;
        if (a.ref_off_hi[r] < 0) continue;                                  // unmapped / duplicate / start 0: counted by the host
        const int64_t g0 = ((int64_t)a.ref_off_hi[r] << 32) | (uint32_t)a.ref_off_lo[r];
        const int L = a.l_seq[r];
        const uint32_t *cg = a.cigar + a.cig_off[r]; const int nc = (int)a.n_cig[r];
        int R = 0; bool gapped = false;
        for (int c = 0; c < nc; ++c) {
            const int op = (int)(cg[c] & 15u), len = (int)(cg[c] >> 4);
            if (cigar_on_ref(op)) R += len;
            if (Q && (op == 1 || op == 2)) gapped = true;                    // the CIGAR string contains I or D (:379-382)
        }
        if (R < 1) R = 1;                                                    // htsjdk: alignment end = start for an empty span
        ++n_proc;
        const int width = L > R ? L : R;
        if (width > a.max_len) { ++n_long; continue; }                      // the Java would fail here (array bound): reported as an error by the host
        const bool strand = (a.flag[r] & 16u) != 0;
        const uint64_t sb = a.seq_off[r];
        const bool has_q = Q && L > 0 && a.qual[sb] != 0xffu;               // QUAL '*' (BAM 0xFF): htsjdk gives an empty array
        const bool in_qpm = Q && has_q && !gapped;
        auto book = [&](int p, int jk) {
            atomicAdd(&s_conv[p * 16 + jk], 1u);
            if (Q && in_qpm) {
                if (p < L) { atomicAdd(&s_qpm[rep + jk], (unsigned long long)a.qual[sb + (uint64_t)p]); atomicAdd(&s_qpc[rep + jk], 1u); }
                else ++n_beyond;
            }
        };
        auto book_quals = [&]() {                                           // a record that reaches the comparison loop (:363)
            if (!Q) return;
            if (!has_q) { ++n_noq; return; }
            if (Q == 2) {
                int i = (int)(threadIdx.x & 63) % L;                         // lanes start at different positions: fewer same-word atomics
                for (int t = 0; t < L; ++t) {
                    atomicAdd(&s_qsum[i], (unsigned int)a.qual[sb + (uint64_t)i]); atomicAdd(&s_qcnt[i], 1u);
                    if (++i == L) i = 0;
                }
                a.n_q[r] = L;
            }
        };
        ProfRef rf{a.pac, a.hole_off, a.hole_len, a.n_holes, 0};
        rf.seek(g0);
        if (L == R) {                                                       // spans of equal length: base by base, the CIGAR is not looked at
            book_quals();
            for (int c = 0; c < L; ++c) {
                const int pr = rf.at(g0 + c), pd = prof_read_code(a.seq, sb + (uint64_t)c);
                if (pr >= 0 && pd >= 0) book(strand ? L - 1 - c : c, strand ? (3 - pr) * 4 + (3 - pd) : pr * 4 + pd);
            }
            continue;
        }
        ++n_indel;
        // pass 1: gap columns are booked whatever follows; a match block that leaves the arrays marks the read as skipped
        bool skip = false;
        { int pm = 0, pref = 0, prd = 0;
          for (int c = 0; c < nc; ++c) {
              const int op = (int)(cg[c] & 15u), len = (int)(cg[c] >> 4);
              if (op == 0 || op == 7 || op == 8) { if (pm + len > width || pref + len > R || prd + len > L) skip = true; pm += len; pref += len; prd += len; }
              else if (op == 3) { pref += len; prd += len; }
              else if (op == 1) { pm += len; prd += len; for (int q = 1; q <= len; ++q) if (pm + q < a.max_len) atomicAdd(&s_ins[pm + q], 1u); }
              else if (op == 2) { pm += len; pref += len; for (int q = 1; q <= len; ++q) if (pm + q < a.max_len) atomicAdd(&s_del[pm + q], 1u); }
          } }
        if (skip) { ++n_skip; continue; }
        book_quals();
        // pass 2: the match columns
        { int pm = 0, pref = 0, prd = 0;
          for (int c = 0; c < nc; ++c) {
              const int op = (int)(cg[c] & 15u), len = (int)(cg[c] >> 4);
              if (op == 0 || op == 7 || op == 8) {
                  for (int z = 0; z < len; ++z) {
                      const int pr = rf.at(g0 + pref + z), pd = prof_read_code(a.seq, sb + (uint64_t)(prd + z)), col = pm + z;
                      if (pr >= 0 && pd >= 0) book(strand ? width - 1 - col : col, strand ? (3 - pr) * 4 + (3 - pd) : pr * 4 + pd);
                  }
                  pm += len; pref += len; prd += len;
              } else if (op == 3) { pref += len; prd += len; }
              else if (op == 1) { pm += len; prd += len; }
              else if (op == 2) { pm += len; pref += len; }
          } }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.max_len * 16; i += blockDim.x) if (s_conv[i]) atomicAdd(&a.conv[i], (unsigned long long)s_conv[i]);
    for (int i = threadIdx.x; i < a.max_len; i += blockDim.x) { if (s_ins[i]) atomicAdd(&a.ins[i], (unsigned long long)s_ins[i]); if (s_del[i]) atomicAdd(&a.del[i], (unsigned long long)s_del[i]); }
    if (n_proc) atomicAdd(&a.stat[0], n_proc);
    if (n_indel) atomicAdd(&a.stat[1], n_indel);
    if (n_skip) atomicAdd(&a.stat[2], n_skip);
    if (n_long) atomicAdd(&a.stat[3], n_long);
    if (Q) {
        if (threadIdx.x < 16) {
            unsigned long long sq = 0, sc = 0;
            for (int k = 0; k < kQpmReps; ++k) { sq += s_qpm[k * 16 + threadIdx.x]; sc += s_qpc[k * 16 + threadIdx.x]; }
            if (sc) { atomicAdd(&a.qpm[threadIdx.x], sq); atomicAdd(&a.qpm[16 + threadIdx.x], sc); }
        }
        if (n_noq) atomicAdd(&a.stat[4], n_noq);
        if (n_beyond) atomicAdd(&a.stat[5], n_beyond);
    }
    if (Q == 2)
        for (int i = threadIdx.x; i < a.max_len; i += blockDim.x) if (s_qcnt[i]) { atomicAdd(&a.qpos[i], (unsigned long long)s_qsum[i]); atomicAdd(&a.qpos[a.max_len + i], (unsigned long long)s_qcnt[i]); }
}

// .qualities standard deviation, :421-436: per position i, tempSdValue += Math.pow(q - mean, 2) over the list of position i,
// i.e. over the records in FILE order, one rounded add at a time.  That recurrence is not associative, so no histogram or
// tree reduction gives its bits: one lane per read position walks all records in order.  One block per 64 positions; wave 0
// adds, waves 1..7 stage the QUAL bytes of the next chunk of records in LDS meanwhile (each record's bytes for the 64
// positions are adjacent, so a loader wave's loads coalesce), one barrier per chunk.  Math.pow(x, 2.0) == x * x exactly
// (HotSpot's intrinsic since JDK 9 special-cases the exponent 2); the product and the sum are rounded one at a time: no FMA.
constexpr int kSdLoaders = 7, kSdPer = 32, kSdChunk = kSdLoaders * kSdPer;
__global__ void __launch_bounds__(64 * (kSdLoaders + 1)) k_qual_sd(const uint8_t *__restrict__ qual, const uint64_t *__restrict__ seq_off,
                                                                   const int32_t *__restrict__ n_q, int n_records, int max_len,
                                                                   const unsigned long long *__restrict__ qpos, double *__restrict__ ssd)
{
#pragma clang fp contract(off)
    __shared__ uint16_t buf[2][kSdChunk][64];                 // 56 KiB; 0xFFFF: the record books nothing at this position
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), i = (int)blockIdx.x * 64 + lane;
    const int n_chunks = (n_records + kSdChunk - 1) / kSdChunk;
    double s = 0, mean = 0;
    if (wave == 0 && i < max_len) {
        const unsigned long long c = qpos[max_len + i];
        mean = c ? (double)qpos[i] / (double)c : 0.0;
        s = ssd[i];                                           // earlier batches of the same totals
    }
    for (int k = 0; k <= n_chunks; ++k) {
        if (wave > 0 && k < n_chunks) {
            // every load is unconditional (clamped record, a safe byte where nothing is booked) and the choice a select, so
            // the 32 records' loads are in flight together instead of one branch and one wait each
            const int r0 = k * kSdChunk + (wave - 1) * kSdPer;
            int nq[kSdPer]; uint64_t so[kSdPer]; uint16_t v[kSdPer];
#pragma unroll
            for (int u = 0; u < kSdPer; ++u) {
                const int r = min(r0 + u, n_records - 1);
                const int c = n_q[r];
                nq[u] = r0 + u < n_records ? c : 0;
                so[u] = seq_off[r];
            }
#pragma unroll
            for (int u = 0; u < kSdPer; ++u) {
                const bool ok = i < nq[u];                                            // n_q <= the record's length
                const uint8_t q = qual[ok ? so[u] + (uint64_t)i : 0];
                v[u] = ok ? (uint16_t)q : (uint16_t)0xffff;
            }
#pragma unroll
            for (int u = 0; u < kSdPer; ++u) buf[k & 1][(wave - 1) * kSdPer + u][lane] = v[u];
        }
        if (wave == 0 && k > 0) {
            const int m = min(kSdChunk, n_records - (k - 1) * kSdChunk);
            const uint16_t (*b)[64] = buf[(k - 1) & 1];
#pragma unroll 8
            for (int u = 0; u < m; ++u) {
                const unsigned q = b[u][lane];
                const double d = (double)(int)q - mean;
                const double t = s + d * d;
                s = q != 0xffffu ? t : s;
            }
        }
        __syncthreads();
    }
    if (wave == 0 && i < max_len) ssd[i] = s;
}

struct ProfileAccum::Impl {
    int device, max_len, quals = 0; StreamGuard sg; const uint8_t *pac;
    std::unique_ptr<RefTables> ref;
    DevBuf<unsigned long long> d_acc; size_t n_acc = 0;
    struct Kept { DevBuf<uint8_t> qual; DevBuf<uint64_t> soff; DevBuf<int32_t> nq; int n = 0; };
    std::vector<Kept> kept;                   // quals == 2: the batches in order, for the standard-deviation walk
    DevBuf<double> d_ssd;
    double ms_count = 0;
};
// the accumulator: conv (max_len*16), ins, del (max_len each), stat (4; quals >= 1: 6), quals >= 1: qpm (32), quals == 2: qpos (2*max_len)
static size_t prof_acc_words(int max_len, int quals)
{
    return (size_t)max_len * 18 + 4 + (quals >= 1 ? 2 + 32 : 0) + (quals == 2 ? (size_t)max_len * 2 : 0);
}
// the one range check of every entry: 1..profile_max_len(quals), so a length that passes it never fails later on LDS bytes
void profile_check_max_len(int max_len, int quals)
{
    if (quals < 0 || quals > 2) throw Error("error profile: quality mode out of range");
    if (max_len < 1 || max_len > profile_max_len(quals))
        throw Error(std::string("error profile: maximum read length out of range") + (quals ? " for the quality files" : "") + " (1.." + std::to_string(profile_max_len(quals)) + ")");
}
ProfileAccum::ProfileAccum(int device, const Index &ix, int max_len, int quals)
{
    profile_check_max_len(max_len, quals);
    require_device(device);
    std::unique_ptr<Impl> q(new Impl());
    q->device = device; q->max_len = max_len; q->quals = quals; q->pac = ix.pac.p;
    q->ref.reset(new RefTables(ix, q->sg.s));
    q->n_acc = prof_acc_words(max_len, quals);
    q->d_acc.alloc(q->n_acc); q->d_acc.zero(q->sg.s);
    if (quals == 2) { q->d_ssd.alloc((size_t)max_len); q->d_ssd.zero(q->sg.s); }
    PS_HIP(hipStreamSynchronize(q->sg.s));
    p = q.release();
}
ProfileAccum::~ProfileAccum() { delete p; }
void ProfileAccum::add(const ProfRecords &t)
{
    const size_t n = t.n();
    if (!n) return;
    if (n > 0x7fffffffull) throw Error("error profile: more than 2^31 records in one call");
    const int Q = p->quals;
    if (Q && t.qual.size() != t.seq.size() * 2) throw Error("error profile: the records carry no base qualities");
    require_device(p->device);
    hipStream_t s = p->sg.s;
    std::vector<int32_t> lo(n), hi(n);
    for (size_t i = 0; i < n; ++i) { const int64_t g = t.gpos[i]; lo[i] = g < 0 ? 0 : (int32_t)(uint32_t)(g & 0xffffffffll); hi[i] = g < 0 ? -1 : (int32_t)(g >> 32); }
    DevBuf<int32_t> d_lo, d_hi, d_nq; DevRecTable d;
    upload(d_lo, lo, s); upload(d_hi, hi, s); d.upload(t, s);
    if (Q == 2) d_nq.alloc(n);
    const int max_len = p->max_len;
    ProfArgs a;
    a.ref_off_lo = d_lo.p; a.ref_off_hi = d_hi.p; a.l_seq = d.l_seq.p; a.flag = d.flag.p; a.cig_off = d.cig_off.p; a.n_cig = d.n_cig.p; a.cigar = d.cigar.p;
    a.seq_off = d.seq_off.p; a.seq = d.seq.p; a.pac = p->pac; a.hole_off = p->ref->hole_off.p; a.hole_len = p->ref->hole_len.p; a.n_holes = p->ref->n_holes;
    a.n_records = (int)n; a.max_len = max_len;
    a.conv = p->d_acc.p; a.ins = p->d_acc.p + (size_t)max_len * 16; a.del = a.ins + max_len; a.stat = a.del + max_len;
    a.qual = d.qual.p; a.qpm = Q ? a.stat + 6 : nullptr; a.qpos = Q == 2 ? a.stat + 6 + 32 : nullptr; a.n_q = d_nq.p;
    int blocks = (int)std::min<size_t>(2048, (n + 255) / 256); if (blocks < 1) blocks = 1;
    if (Q == 0) {
        const size_t lds = prof_lds_bytes(0, max_len);
        set_dynamic_lds(reinterpret_cast<const void *>(k_profile<0>), "k_profile<0>", lds);
        hipLaunchKernelGGL(k_profile<0>, dim3(blocks), dim3(256), lds, s, a);
        PS_HIP(hipGetLastError());
        PS_HIP(hipStreamSynchronize(s));      // the record arrays above are released on return
        return;
    }
    const size_t lds = prof_lds_bytes(Q, max_len);         // <= 160 KiB: profile_max_len
    void (*kern)(ProfArgs) = Q == 1 ? k_profile<1> : k_profile<2>;
    set_dynamic_lds(reinterpret_cast<const void *>(kern), Q == 1 ? "k_profile<1>" : "k_profile<2>", lds);
    p->ms_count += timed(s, [&]() { hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, s, a); PS_HIP(hipGetLastError()); });
    if (Q == 2) { Impl::Kept k; k.qual = std::move(d.qual); k.soff = std::move(d.seq_off); k.nq = std::move(d_nq); k.n = (int)n; p->kept.push_back(std::move(k)); }
}
void ProfileAccum::finish(ProfileCounts &out)
{
    require_device(p->device);
    const int max_len = p->max_len, Q = p->quals;
    const size_t st = (size_t)max_len * 18;
    std::vector<unsigned long long> acc(p->n_acc);
    p->d_acc.download(acc.data(), p->n_acc, p->sg.s);
    PS_HIP(hipStreamSynchronize(p->sg.s));
    out.max_len = max_len;
    out.conv.assign(acc.begin(), acc.begin() + (size_t)max_len * 16);
    out.ins.assign(acc.begin() + (size_t)max_len * 16, acc.begin() + (size_t)max_len * 17);
    out.del.assign(acc.begin() + (size_t)max_len * 17, acc.begin() + (size_t)max_len * 18);
    out.n_processed = acc[st]; out.n_indel_reads = acc[st + 1]; out.n_skipped = acc[st + 2];
    if (acc[st + 3]) throw Error("error profile: a read (or its reference span) is longer than the maximum read length given (the reference's arrays would overflow)");
    out.quals = Q;
    if (!Q) return;
    out.n_without_qual = acc[st + 4]; out.n_qual_beyond_read = acc[st + 5];
    out.qpm_sum.assign(acc.begin() + st + 6, acc.begin() + st + 22);
    out.qpm_cnt.assign(acc.begin() + st + 22, acc.begin() + st + 38);
    out.ms_count = p->ms_count;
    if (Q != 2) return;
    out.qsum.assign(acc.begin() + st + 38, acc.begin() + st + 38 + max_len);
    out.qcnt.assign(acc.begin() + st + 38 + max_len, acc.begin() + st + 38 + 2 * (size_t)max_len);
    const unsigned long long *qpos = p->d_acc.p + st + 38;
    const int grid = (max_len + 63) / 64;
    out.ms_sd = 0;
    for (Impl::Kept &k : p->kept)
        out.ms_sd += timed(p->sg.s, [&]() { hipLaunchKernelGGL(k_qual_sd, dim3(grid), dim3(64 * (kSdLoaders + 1)), 0, p->sg.s, k.qual.p, k.soff.p, k.nq.p, k.n, max_len, qpos, p->d_ssd.p); PS_HIP(hipGetLastError()); });
    p->kept.clear();
    out.qssd.assign((size_t)max_len, 0.0);
    p->d_ssd.download(out.qssd.data(), (size_t)max_len, p->sg.s);
    PS_HIP(hipStreamSynchronize(p->sg.s));
}

void error_profile_count(const char *mapping, const char *ref_prefix, int max_len, int device, int threads, ProfileCounts &out, int quals, double *ms_parse)
{
    profile_check_max_len(max_len, quals);
    require_device(device);
    ProfRecords r;
    const auto t0 = HostClock::now();
    try { load_rec_table(mapping, kRecCigar | kRecSeq | (quals > 0 ? kRecQual : 0u), threads, r); } catch (const std::exception &e) { throw Error(e.what()); }
    if (ms_parse) *ms_parse = ms_since(t0);
    StreamGuard sg;
    Index ix;
    index_load_pac(ref_prefix, ix, sg.s);
    const std::vector<int32_t> ref_to_contig = RefTables::ref_to_contig(ix, r.refs);
    const size_t n = r.n();
    out = ProfileCounts(); out.max_len = max_len;
    unsigned long long n_unmapped = 0, n_duplicate = 0, n_start_zero = 0;
    r.gpos.assign(n, -1);
    for (size_t i = 0; i < n; ++i) {
        if (r.flag[i] & 4u) { ++n_unmapped; continue; }                       // ErrorProfiling.java:155-158
        if (r.flag[i] & 1024u) { ++n_duplicate; continue; }                   // :159-162
        if (r.pos[i] < 0) { ++n_start_zero; continue; }                       // :163-166 (alignment start 0 = no position)
        if (r.ref[i] < 0 || ref_to_contig[r.ref[i]] < 0) throw Error("error profile: a record names a sequence the reference does not have");
        r.gpos[i] = ix.ref.contigs[ref_to_contig[r.ref[i]]].offset + (int64_t)r.pos[i];
    }
    r.ref = {}; r.pos = {};                                                   // gpos stands for them: nothing to upload
    ProfileAccum acc(device, ix, max_len, quals);
    acc.add(r);
    acc.finish(out);
    out.n_records = n; out.n_unmapped = n_unmapped; out.n_duplicate = n_duplicate; out.n_start_zero = n_start_zero;
}

// what the Java derives from the counts before it writes (ErrorProfiling.java:448-458, :553-570): totals per (reference,
// read) base pair and per reference base, and per read position the insertion and deletion rates (0.0 where no base was
// counted at that position)
struct ProfTotals { double tot[4][4], base[4]; std::vector<double> ins_rate, del_rate; };
static ProfTotals profile_totals(const ProfileCounts &c)
{
    const int ML = c.max_len;
    ProfTotals t{};
    std::vector<double> per_pos((size_t)ML, 0.0);
    for (int i = 0; i < ML; ++i)
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 4; ++k) { const double x = (double)c.conv[(size_t)i * 16 + j * 4 + k]; t.tot[j][k] += x; t.base[j] += x; per_pos[i] += x; }
    t.ins_rate.assign((size_t)ML, 0.0); t.del_rate.assign((size_t)ML, 0.0);
    for (int i = 0; i < ML; ++i)
        if (per_pos[i] != 0.0) { t.ins_rate[i] = (double)c.ins[i] / per_pos[i]; t.del_rate[i] = (double)c.del[i] / per_pos[i]; }
    return t;
}

// the two files of ErrorProfiling.java:504-531 and :545-591
void error_profile_write(const ProfileCounts &c, const std::string &out_prefix)
{
    const int ML = c.max_len;
    const ProfTotals t = profile_totals(c);
    std::string text;
    for (int j = 0; j < 4; ++j) {
        for (int k = 0; k < 4; ++k) text += java_double_to_string(t.tot[j][k] / t.base[j]) + "\t";
        text += "\n";
    }
    write_text_file(out_prefix + ".errorprofile", text);
    // a position without counted bases has rate 0 and is left out of the mean, as one whose gaps are 0 (:554-558)
    double ins_all = 0, del_all = 0; int ins_zero = 0, del_zero = 0;
    for (int i = 0; i < ML; ++i) {
        const double x = t.ins_rate[i], y = t.del_rate[i];
        if (x > 0) ins_all += x; else ++ins_zero;
        if (y > 0) del_all += y; else ++del_zero;
    }
    if (ML == ins_zero && ML == del_zero) ins_all = del_all = 0.0;
    else { ins_all = ins_all / (ML - ins_zero); del_all = del_all / (ML - del_zero); }
    write_text_file(out_prefix + ".indelprofile", java_double_to_string(ins_all) + "\t" + java_double_to_string(del_all));
}

// the other four files the Java always writes: .errorprofile.vcf (:504-531, the raw totals as doubles, a blank line after each
// reference base), .qualityPerMismatch (:438-447, :516: QUAL sum / pairs, NaN for none), .indels (:553-579: the rates per
// read position) and .qualities (:421-436: mean and population standard deviation per position; created empty without -q)
void error_profile_write_extra(const ProfileCounts &c, const std::string &out_prefix)
{
    if (c.quals < 1) throw Error("error profile: the quality counts were not taken");
    const int ML = c.max_len;
    const ProfTotals t = profile_totals(c);
    static const char B[4] = {'A', 'C', 'G', 'T'};
    std::string vcf, qpm, ind, qua;
    for (int j = 0; j < 4; ++j) {
        for (int k = 0; k < 4; ++k) {
            vcf += std::string(1, B[j]) + "\t" + B[k] + "\t" + java_double_to_string(t.tot[j][k]) + "\n";
            qpm += java_double_to_string((double)c.qpm_sum[j * 4 + k] / (double)c.qpm_cnt[j * 4 + k]) + "\t";
        }
        vcf += "\n"; qpm += "\n";
    }
    for (int i = 0; i < ML; ++i) ind += java_double_to_string(t.ins_rate[i]) + "\t" + java_double_to_string(t.del_rate[i]) + "\n";
    if (c.quals == 2)
        for (int i = 0; i < ML; ++i) {
            const double n = (double)c.qcnt[i], mean = (double)c.qsum[i] / n, sd = std::sqrt(c.qssd[i] / n);     // n = 0: NaN, NaN
            qua += java_double_to_string(mean) + "\t" + java_double_to_string(sd) + "\n";
        }
    const std::pair<const char *, const std::string *> files[4] = {{".errorprofile.vcf", &vcf}, {".qualityPerMismatch", &qpm}, {".indels", &ind}, {".qualities", &qua}};
    for (const auto &fl : files) write_text_file(out_prefix + fl.first, *fl.second);
}

}  // namespace ps
