// ps_benchmark.hip -- a mapping of simulated PAR-CLIP reads scored against the truth in the read names: the toolkit's
// `benchmark` mode (include/parasuite_hip.h, ps_benchmark_reads).
//
// Replaces utils.benchmarking.ValidateBenchmarkStatisticsPARCLIP.calculateBenchmarkStatistics (the toolkit's
// src/utils/benchmarking/ValidateBenchmarkStatisticsPARCLIP.java:43-242), one thread that reads the FASTQ line by line and
// then splits, parses and compares the name of every record.  Both passes are independent per line / per record except for
// three pieces of sequential state, each of which is a minimum over indexes (DESIGN.md §4f has the table).  Here the host
// reads the two files (ps_bam.cpp for the mapping), stages them and writes the text; the device counts:
//   k_bm_fastq      one lane per byte of a piece of the FASTQ: line starts from the byte before; a lane on the start of a
//                   "@SEQ_ID" line reads the line to its end (into the next piece where it runs on: the host appends that
//                   much), splits it and classes its bound field -> lines, positives, negatives, first bad line (:78-103)
//   k_bm_parse      one lane per record: QNAME split, Integer.parseInt of start and end -> status, numbers, bound class, where
//                   the truth contig stands in the name; first FATAL, first BADNUM, first "chr" contig (:113-133)
//   (host)          which of the two ends the loop: an error, or the number of records that count
//   k_bm_score      one lane per counted record: the sticky "chr" adjustment, chrM -> chrMT, the +-5 window -> TP, TN or the
//                   first reason why not (:134-159)
// Counters are summed per wave (ballot + popcount, one atomic per wave), minima taken by the wave's first set lane.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/parasuite_hip.h"
#include "ps_dev.h"
#include "ps_java.h"
#include "ps_pipeline.h"

namespace ps {

enum : unsigned { kBmOk = 0, kBmFatal = 1, kBmBadNum = 2 };              // per record (k_bm_parse)
enum : unsigned { kBmNeg = 0, kBmPos = 1, kBmOther = 2 };                // bound class: "0", "1", anything else
enum : int { kBmLines = 0, kBmPositives = 1, kBmNegatives = 2 };         // counters of pass 1
enum : int { kBmTp = 0, kBmTn = 1, kBmUnplaced = 2, kBmOtherContig = 3, kBmOutside = 4, kBmOtherBound = 5, kBmCounters = 6 };
constexpr unsigned kBmNone = 0xFFFFFFFFu;                                // no such record
constexpr unsigned long long kBmNoLine = ~0ull;
constexpr size_t kBmPiece = (size_t)64 << 20;                            // bytes of FASTQ per staged piece (PS_BENCH_PIECE overrides)

// ---- the rules for one name (__host__ too: they can be run without a device)

// String.split("\\|") of a FASTQ header or a QNAME: fields 2..5 (contig, start, end, bound field) as byte ranges of s, and the
// Java's two ways to die on it: fewer than six fields once the trailing empty ones are dropped (:84, :115-118), or a bound
// field made only of '-', which split("-") turns into an empty array (:84, :118).  The bound class is the text before the
// field's first '-'.
struct BmSplit { uint32_t off[4], len[4]; bool fatal; unsigned bound; };
__host__ __device__ inline BmSplit bm_split(const uint8_t *s, uint32_t n)
{
    BmSplit r; int f = 0, last_nonempty = -1; uint32_t beg = 0;
    for (int k = 0; k < 4; ++k) r.off[k] = r.len[k] = 0;
    for (uint32_t i = 0; i <= n; ++i) {
        if (i < n && s[i] != '|') continue;
        if (i > beg) last_nonempty = f;
        if (f >= 2 && f <= 5) { r.off[f - 2] = beg; r.len[f - 2] = i - beg; }
        ++f; beg = i + 1;
    }
    r.fatal = last_nonempty < 5; r.bound = kBmOther;
    if (r.fatal) return r;
    const uint8_t *b = s + r.off[3]; const uint32_t bl = r.len[3];
    uint32_t d = 0;
    while (d < bl && b[d] != '-') ++d;                                    // d: length of the text before the first '-'
    if (d == 0 && bl > 0) {                                               // starts with '-': all '-' is the empty array, else [0] is ""
        uint32_t k = 0;
        while (k < bl && b[k] == '-') ++k;
        r.fatal = k == bl;
    } else if (d == 1) r.bound = b[0] == '1' ? kBmPos : (b[0] == '0' ? kBmNeg : kBmOther);
    return r;
}

__host__ __device__ inline bool bm_is_chr(const uint8_t *s, uint32_t n) { return n >= 3 && s[0] == 'c' && s[1] == 'h' && s[2] == 'r'; }

// :134-159 for one record: the truth contig t[0, tl) as the Java rewrites it -- "chr" put in front or taken off by the sticky
// flag, then exactly "chrM" read as "chrMT" -- compared in place with the reference name c[0, cl), and the window with 32-bit
// wrap-around as Java ints have it.  Returns the counter the record adds to; unplaced: the record has no reference (c is "*").
__host__ __device__ inline int bm_score(const uint8_t *t, uint32_t tl, const uint8_t *c, uint32_t cl, bool unplaced, bool sticky,
                                        int32_t start, int32_t end, int32_t aln_start, int32_t aln_end, unsigned bound)
{
    const bool has = bm_is_chr(t, tl);
    const uint32_t add = sticky && !has ? 3u : 0u, skip = !sticky && has ? 3u : 0u, vl = add + tl - skip;
    auto at = [&](uint32_t k) -> uint8_t { return k < add ? (uint8_t)"chr"[k] : t[skip + k - add]; };
    bool same;
    if (vl == 4 && at(0) == 'c' && at(1) == 'h' && at(2) == 'r' && at(3) == 'M')
        same = cl == 5 && c[0] == 'c' && c[1] == 'h' && c[2] == 'r' && c[3] == 'M' && c[4] == 'T';
    else {
        same = vl == cl;
        for (uint32_t k = 0; same && k < vl; ++k) same = at(k) == c[k];
    }
    const int32_t lo = (int32_t)((uint32_t)start - 5u), hi = (int32_t)((uint32_t)end + 5u);
    const bool inside = lo <= aln_start && hi >= aln_end;
    if (same && inside && bound != kBmOther) return bound == kBmPos ? kBmTp : kBmTn;
    return unplaced ? kBmUnplaced : (!same ? kBmOtherContig : (!inside ? kBmOutside : kBmOtherBound));   // the first reason that applies
}

// ---- kernels.  Every lane of a wave reaches the ballots: no lane returns early.

__device__ __forceinline__ void bm_wave_count(bool p, unsigned long long *dst)
{
    const unsigned long long m = __ballot(p);
    if (m && (threadIdx.x & 63u) == 0u) atomicAdd(dst, (unsigned long long)__popcll(m));
}
// lanes of a wave hold ascending indexes: the first set lane has the wave's minimum
template <class T> __device__ __forceinline__ void bm_wave_min(bool p, T v, T *dst)
{
    const unsigned long long m = __ballot(p);
    if (m && (int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1) atomicMin(dst, v);
}

// buf holds `len` bytes of the file from offset `base` and behind them the rest of the line that is open at the piece's end
// (`avail` bytes in all); prev: the byte before the piece, -1 at the start of the file
__global__ void __launch_bounds__(256) k_bm_fastq(const uint8_t *buf, uint32_t len, uint32_t avail, int prev, unsigned long long base,
                                                 unsigned long long *cnt, unsigned long long *bad_line)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool start = false, pos = false, neg = false, bad = false;
    if (i < len) {
        const int p = i ? (int)buf[i - 1] : prev, c = buf[i];
        start = p < 0 || p == '\n' || (p == '\r' && c != '\n');          // "\r\n" is one line end (BufferedReader.readLine)
        if (start && avail - i >= 7u && c == '@' && buf[i + 1] == 'S' && buf[i + 2] == 'E' && buf[i + 3] == 'Q' && buf[i + 4] == '_' &&
            buf[i + 5] == 'I' && buf[i + 6] == 'D') {
            uint32_t e = i + 7;
            while (e < avail && buf[e] != '\n' && buf[e] != '\r') ++e;
            const BmSplit s = bm_split(buf + i, e - i);
            bad = s.fatal; pos = !bad && s.bound == kBmPos; neg = !bad && s.bound == kBmNeg;
        }
    }
    bm_wave_count(start, cnt + kBmLines);
    bm_wave_count(pos, cnt + kBmPositives);
    bm_wave_count(neg, cnt + kBmNegatives);
    bm_wave_min(bad, base + i, bad_line);
}

struct BmRecs {                        // the records as flat arrays; the reference table has one more entry, "*", at n_ref
    int n; const uint64_t *name_off; const uint8_t *name_len, *names;
    const int32_t *ref, *pos; const uint32_t *flag, *cig_off, *n_cig, *cigar;
    int n_ref; const uint32_t *ref_off, *ref_len; const uint8_t *ref_names, *ref_chr;
    int32_t *start, *end; uint32_t *truth; uint8_t *cls;                 // k_bm_parse -> k_bm_score: truth = offset | length << 16 of field 2 in the name, cls = bound | status << 4
};

__global__ void __launch_bounds__(256) k_bm_parse(BmRecs a, unsigned *first /* FATAL, BADNUM, chr */)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    unsigned status = kBmOk; bool chr = false;
    if (j < a.n) {
        const uint8_t *s = a.names + a.name_off[j];
        const BmSplit sp = bm_split(s, a.name_len[j]);
        int32_t st = 0, en = 0;
        if (sp.fatal) status = kBmFatal;                                  // :113-118 run before :127
        else if (!java_parse_int(s + sp.off[1], sp.len[1], st) || !java_parse_int(s + sp.off[2], sp.len[2], en)) status = kBmBadNum;
        a.start[j] = st; a.end[j] = en;
        a.truth[j] = sp.off[0] | (sp.len[0] << 16);
        a.cls[j] = (uint8_t)(sp.bound | (status << 4));
        chr = a.ref[j] >= 0 && a.ref_chr[a.ref[j]];
    }
    bm_wave_min(status == kBmFatal, (unsigned)j, first + 0);
    bm_wave_min(status == kBmBadNum, (unsigned)j, first + 1);
    bm_wave_min(chr, (unsigned)j, first + 2);
}

// records [0, n): n is where the loop ended.  getAlignmentEnd by the library's rule (parasuite_hip.h, ps_combine_genome_transcript)
__global__ void __launch_bounds__(256) k_bm_score(BmRecs a, int n, unsigned first_chr, unsigned long long *cnt)
{
    const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    int what = -1;
    if (j < n) {
        const uint32_t ref_len = (uint32_t)cigar_ref_span(a.cigar + a.cig_off[j], a.n_cig[j]);
        const int32_t aln_start = (int32_t)((uint32_t)a.pos[j] + 1u);     // htsjdk getAlignmentStart
        const int32_t aln_end = (a.flag[j] & 4u) ? 0 : (int32_t)((uint32_t)aln_start + ref_len - 1u);
        const int r = a.ref[j] < 0 ? a.n_ref : a.ref[j];
        const uint32_t tr = a.truth[j];
        what = bm_score(a.names + a.name_off[j] + (tr & 0xffffu), tr >> 16, a.ref_names + a.ref_off[r], a.ref_len[r], a.ref[j] < 0,
                        (unsigned)j >= first_chr, a.start[j], a.end[j], aln_start, aln_end, a.cls[j] & 15u);
    }
    for (int k = 0; k < kBmCounters; ++k) bm_wave_count(what == k, cnt + k);
}

// ---- host side

// :165-166, :200-225.  Java int arithmetic (it wraps) and float division: 0/0 is NaN, x/0 an infinity
BenchmarkRatios benchmark_ratios(const ps_benchmark_stats &st)
{
    const int32_t tp = (int32_t)st.n_tp, tn = (int32_t)st.n_tn, p = (int32_t)st.n_positives, n = (int32_t)st.n_negatives;
    auto add = [](int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); };
    auto sub = [](int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); };
    BenchmarkRatios r;
    r.fp = sub(p, tp); r.fn = sub(n, tn); r.matched = add(tp, tn);
    r.precision = (float)tp / (float)add(tp, r.fp);
    r.recall = (float)tp / (float)add(tp, r.fn);
    r.accuracy = (float)r.matched / (float)add(p, n);
    return r;
}
std::string benchmark_text(const ps_benchmark_stats &st, const BenchmarkRatios &r)
{
    return "matched correctly:\t" + std::to_string(r.matched) + "\nreadsProcessed:\t" + std::to_string(st.n_processed) +
           "\nall reads:\t" + std::to_string(st.n_reads) + "\nprecision:\t" + java_float_to_string(r.precision) +
           "\nrecall:\t" + java_float_to_string(r.recall) + "\naccuracy:\t" + java_float_to_string(r.accuracy);
}

namespace {
struct BmFile {                        // the FASTQ, mapped read-only (the bytes reach memory when a piece is staged)
    const uint8_t *p = nullptr; size_t n = 0; int fd = -1;
    ~BmFile() { if (p) munmap((void *)p, n); if (fd >= 0) close(fd); }
    void open(const char *path)
    {
        fd = ::open(path, O_RDONLY);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) throw Error(std::string("cannot open ") + path);
        n = (size_t)sb.st_size;
        if (!n) return;
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) throw Error(std::string("cannot read ") + path);
        p = (const uint8_t *)m;
    }
};
// read: the mapping through load_records (file, inflate or SAM encoding) and the FASTQ's bytes into the page-locked buffers
// (the page faults of the mapped file are the read); decode: the records flattened; copy: the pieces' H2D copies by their
// events, the record arrays' uploads by the clock; k_fastq: k_bm_fastq by its events; k_records: the two record kernels with the
// host's decision and the small downloads between them by the clock
struct BmTimes { double read = 0, decode = 0, copy = 0, k_fastq = 0, k_records = 0, write = 0; };
}  // namespace

void benchmark_run(const char *mapping_path, const char *out_path, const char *reads_path, int device, ps_benchmark_stats *stats)
{
    using clk = HostClock;
    const std::string who = "ps_benchmark_reads: ";
    if (!mapping_path || !mapping_path[0] || !out_path || !out_path[0] || !reads_path || !reads_path[0])
        throw Error(who + "mapping file, statistics file and reads file are required");
    OutFiles files(".benchmark-tmp"); const std::string tmp_path = files.add(out_path);
    files.refuse_inputs({mapping_path, reads_path}, who);
    require_device(device);                                                // before the files are read
    BmTimes tm; ps_benchmark_stats st{};
    size_t piece = kBmPiece;
    if (const char *e = std::getenv("PS_BENCH_PIECE")) piece = (size_t)std::max(1ll, std::atoll(e));   // tests: force many pieces
    piece = std::min(piece, (size_t)1 << 30);

    auto t0 = clk::now();
    BmFile fq; fq.open(reads_path);
    if (fq.n >= 2 && fq.p[0] == 31 && fq.p[1] == 139) throw Error(who + reads_path + " is gzip-compressed; the reads file must be plain text");
    BamFile B;
    load_records(mapping_path, 8, B);
    if (B.n() > (size_t)INT_MAX) throw Error(who + "more than 2^31 - 1 records");
    tm.read = ms_since(t0);

    StreamGuard sg; hipStream_t s = sg.s;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } };   // declared behind buffers a copy may still read: runs before they are let go

    // ---- pass 1: the FASTQ in pieces through two page-locked buffers; one piece is copied and counted while the next is staged
    DevBuf<unsigned long long> d_cnt1; d_cnt1.alloc(4);
    {
        const unsigned long long init[4] = {0, 0, 0, kBmNoLine};
        d_cnt1.upload(init, 4, s); PS_HIP(hipStreamSynchronize(s));
    }
    {
        PinBuf pin[2]; DevBuf<uint8_t> dev[2]; EventPair ev_copy[2], ev_kernel[2]; bool used[2] = {false, false};
        Drain drain{s};                                                    // an error below unwinds pin[]: no copy may be in flight then
        auto retire = [&](int k) {
            if (!used[k]) return;
            tm.k_fastq += ev_kernel[k].ms(); tm.copy += ev_copy[k].ms(); used[k] = false;   // the kernel is the later of the two
        };
        int prev = -1; size_t k = 0;
        for (size_t off = 0; off < fq.n; off += piece, ++k) {
            const size_t len = std::min(piece, fq.n - off);
            // a piece that does not end on a line end has a line open, which runs to q: those bytes are staged twice, here and with
            // their own piece (nothing at 64 MiB; with the tests' PS_BENCH_PIECE=1 every line is staged once per byte of it)
            size_t q = off + len;
            if (fq.p[q - 1] != '\n' && fq.p[q - 1] != '\r') while (q < fq.n && fq.p[q] != '\n' && fq.p[q] != '\r') ++q;
            const size_t avail = q - off;
            if (avail > (size_t)UINT_MAX) throw Error(who + "a line of " + reads_path + " is longer than 2^32 bytes");
            const int slot = (int)(k & 1);
            retire(slot);
            const auto r0 = clk::now();
            void *h = pin[slot].get(avail);
            std::memcpy(h, fq.p + off, avail);
            tm.read += ms_since(r0);
            if (dev[slot].n < avail) dev[slot].alloc(avail + avail / 8);
            ev_copy[slot].start(s);
            PS_HIP(hipMemcpyAsync(dev[slot].p, h, avail, hipMemcpyHostToDevice, s));
            ev_copy[slot].stop(s); ev_kernel[slot].start(s);
            hipLaunchKernelGGL(k_bm_fastq, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, dev[slot].p, (uint32_t)len, (uint32_t)avail, prev,
                               (unsigned long long)off, d_cnt1.p, d_cnt1.p + 3);
            PS_HIP(hipGetLastError());
            ev_kernel[slot].stop(s);
            used[slot] = true;
            prev = fq.p[off + len - 1];
        }
        retire(0); retire(1);
    }
    unsigned long long c1[4];
    d_cnt1.download(c1, 4, s); PS_HIP(hipStreamSynchronize(s));
    if (c1[3] != kBmNoLine) {                                              // the Java's uncaught ArrayIndexOutOfBounds
        unsigned long long line = 0;
        for (size_t i = 0; i <= (size_t)c1[3]; ++i) line += i == 0 || fq.p[i - 1] == '\n' || (fq.p[i - 1] == '\r' && fq.p[i] != '\n');
        throw Error(who + "line " + std::to_string(line) + " of " + reads_path + " starts with @SEQ_ID but has fewer than six '|' fields, or a sixth field made of '-' only");
    }
    if (c1[kBmLines] % 4 != 0) throw Error(who + reads_path + " has " + std::to_string(c1[kBmLines]) + " lines, which is not a multiple of 4");
    if (c1[kBmLines] > (unsigned long long)INT_MAX) throw Error(who + "more than 2^31 - 1 lines in " + reads_path);
    st.n_lines = c1[kBmLines]; st.n_reads = c1[kBmLines] / 4; st.n_positives = c1[kBmPositives]; st.n_negatives = c1[kBmNegatives];

    // ---- pass 2: the records as flat arrays
    t0 = clk::now();
    const int n = (int)B.n(); const size_t nn = (size_t)std::max(1, n), n_ref = B.refs.size();
    st.n_records = (uint64_t)n;
    RecTable R;
    try { flatten_records(B, kRecCigar | kRecNames, nullptr, 8, R); } catch (const std::exception &e) { throw Error(who + e.what()); }
    std::vector<uint32_t> ref_off(n_ref + 1), ref_len(n_ref + 1); std::vector<uint8_t> ref_chr(n_ref + 1, 0), ref_names;
    for (size_t r = 0; r <= n_ref; ++r) {                                  // entry n_ref: "*", the name of no reference
        const std::string nm = r < n_ref ? B.refs[r].first : std::string("*");
        ref_off[r] = (uint32_t)ref_names.size(); ref_len[r] = (uint32_t)nm.size();
        ref_names.insert(ref_names.end(), nm.begin(), nm.end());
        ref_chr[r] = bm_is_chr((const uint8_t *)nm.data(), (uint32_t)nm.size());   // chr.startsWith("chr"), once per @SQ entry
    }
    tm.decode = ms_since(t0);

    t0 = clk::now();
    DevRecTable d; DevBuf<uint8_t> d_rnames, d_rchr, d_cls; DevBuf<int32_t> d_start, d_end;
    DevBuf<uint32_t> d_roff, d_rlen, d_truth; DevBuf<unsigned> d_first; DevBuf<unsigned long long> d_cnt2;
    d.upload(R, s);
    upload(d_roff, ref_off, s); upload(d_rlen, ref_len, s); upload(d_rnames, ref_names, s); upload(d_rchr, ref_chr, s);
    d_start.alloc(nn); d_end.alloc(nn); d_truth.alloc(nn); d_cls.alloc(nn); d_first.alloc(3); d_cnt2.alloc(kBmCounters);
    const unsigned none[3] = {kBmNone, kBmNone, kBmNone};
    d_first.upload(none, 3, s); d_cnt2.zero(s);
    PS_HIP(hipStreamSynchronize(s));
    tm.copy += ms_since(t0);

    t0 = clk::now();
    BmRecs a;
    a.n = n; a.name_off = d.name_off.p; a.name_len = d.name_len.p; a.names = d.names.p; a.ref = d.ref.p; a.pos = d.pos.p; a.flag = d.flag.p;
    a.cig_off = d.cig_off.p; a.n_cig = d.n_cig.p; a.cigar = d.cigar.p; a.n_ref = (int)n_ref; a.ref_off = d_roff.p; a.ref_len = d_rlen.p;
    a.ref_names = d_rnames.p; a.ref_chr = d_rchr.p; a.start = d_start.p; a.end = d_end.p; a.truth = d_truth.p; a.cls = d_cls.p;
    unsigned first[3] = {kBmNone, kBmNone, kBmNone};
    if (n) {
        hipLaunchKernelGGL(k_bm_parse, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, d_first.p);
        PS_HIP(hipGetLastError());
        d_first.download(first, 3, s);
        PS_HIP(hipStreamSynchronize(s));
    }
    // the Java dies at the first short name unless an unparsable number has ended its loop before (:113-128, :177)
    if (first[0] != kBmNone && first[0] < first[1]) {
        const uint8_t *p = B.rec((size_t)first[0]);
        throw Error(who + "record " + std::to_string(first[0] + 1) + " (" + std::string((const char *)p + 36, (size_t)p[12] - 1) +
                    "): the name has fewer than six '|' fields, or a sixth field made of '-' only");
    }
    const int limit = first[1] != kBmNone ? (int)first[1] : n;
    st.n_processed = (uint64_t)limit; st.bad_number_record = first[1] != kBmNone ? (uint64_t)first[1] + 1 : 0;
    unsigned long long c2[kBmCounters] = {0, 0, 0, 0, 0, 0};
    if (limit) {
        hipLaunchKernelGGL(k_bm_score, dim3((unsigned)((limit + 255) / 256)), dim3(256), 0, s, a, limit, first[2], d_cnt2.p);
        PS_HIP(hipGetLastError());
        d_cnt2.download(c2, kBmCounters, s);
        PS_HIP(hipStreamSynchronize(s));
    }
    tm.k_records = ms_since(t0);
    st.n_tp = c2[kBmTp]; st.n_tn = c2[kBmTn]; st.n_unplaced = c2[kBmUnplaced]; st.n_other_contig = c2[kBmOtherContig];
    st.n_outside = c2[kBmOutside]; st.n_other_bound = c2[kBmOtherBound];

    // ---- the text
    t0 = clk::now();
    const BenchmarkRatios rt = benchmark_ratios(st);
    const std::string text = benchmark_text(st, rt);
    st.precision = rt.precision; st.recall = rt.recall; st.accuracy = rt.accuracy;
    try { write_text_file(tmp_path, text); files.publish_all(); files.keep(); } catch (const std::exception &e) { throw Error(who + e.what()); }
    tm.write = ms_since(t0);
    if (stats) *stats = st;
    if (std::getenv("PS_VERBOSE"))
        std::fprintf(stderr, "[parasuite-hip] ps_benchmark_reads: TP=%lld; TN=%lld; FP=%lld; FN=%lld; %llu reads, %llu records, %llu processed "
                             "(%llu unplaced, %llu on another contig, %llu outside the window, %llu with another bound class); "
                             "read + stage %.1f ms, decode %.1f ms, copy %.1f ms, kernels %.2f ms (FASTQ pass %.2f, record passes %.2f), write %.2f ms\n",
                     (long long)st.n_tp, (long long)st.n_tn, (long long)rt.fp, (long long)rt.fn,
                     (unsigned long long)st.n_reads, (unsigned long long)st.n_records, (unsigned long long)st.n_processed, (unsigned long long)st.n_unplaced,
                     (unsigned long long)st.n_other_contig, (unsigned long long)st.n_outside, (unsigned long long)st.n_other_bound,
                     tm.read, tm.decode, tm.copy, tm.k_fastq + tm.k_records, tm.k_fastq, tm.k_records, tm.write);
}

}  // namespace ps
