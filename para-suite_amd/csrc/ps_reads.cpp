// ps_reads.cpp -- read input: FASTQ / FASTA files (plain, gzip or BGZF: ps_inflate.h) as ReadSets, whole or streamed in pieces of
// whole records (host only).
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "ps_inflate.h"
#include "ps_reads.h"

namespace ps {

static inline uint8_t code_of(int ch)
{
    switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1;
                  case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}

// FASTQ / FASTA; read name = header up to the first white space, a trailing /1 or /2 removed
// one parser pass over buf[i0, i1): appends to rs (offsets relative to rs's own arrays)
static void parse_reads_range(const char *buf, size_t i0, size_t i1, ReadSet &rs, bool &any_qual)
{
    struct Lut { uint8_t v[256]; Lut() { for (int c = 0; c < 256; ++c) v[c] = code_of(c); } };
    static const Lut lut_obj;                       // initialised once, safely, however many parser threads arrive
    const uint8_t *lut = lut_obj.v;
    size_t i = i0;
    const size_t n = i1;
    while (i < n) {
        while (i < n && buf[i] != '@' && buf[i] != '>') ++i;
        if (i >= n) break;
        const bool fq = buf[i] == '@';
        size_t s = ++i;
        while (i < n && !std::isspace((unsigned char)buf[i])) ++i;
        size_t nl = i - s;
        if (nl > 2 && buf[s + nl - 2] == '/' && (buf[s + nl - 1] == '1' || buf[s + nl - 1] == '2')) nl -= 2;
        rs.names.insert(rs.names.end(), buf + s, buf + s + nl);
        rs.name_off.push_back((int64_t)rs.names.size());
        const char *eol = (const char *)std::memchr(buf + i, '\n', n - i);
        i = eol ? (size_t)(eol - buf) + 1 : n;
        const size_t before = rs.seq.size();
        const char stop = fq ? '+' : '>';
        while (i < n && buf[i] != stop) {                         // sequence lines
            eol = (const char *)std::memchr(buf + i, '\n', n - i);
            size_t e = eol ? (size_t)(eol - buf) : n, e2 = e;
            while (e2 > i && !std::isgraph((unsigned char)buf[e2 - 1])) --e2;     // trailing CR / blanks
            const size_t at = rs.seq.size();
            rs.seq.resize(at + (e2 - i));
            for (size_t j = i; j < e2; ++j) rs.seq[at + (j - i)] = lut[(unsigned char)buf[j]];
            i = e < n ? e + 1 : n;
        }
        const int32_t len = (int32_t)(rs.seq.size() - before);
        rs.len.push_back(len);
        rs.off.push_back((int64_t)rs.seq.size());
        const size_t qbefore = rs.qual.size();
        if (fq && i < n) {
            eol = (const char *)std::memchr(buf + i, '\n', n - i);
            i = eol ? (size_t)(eol - buf) + 1 : n;
            while (i < n && (int32_t)(rs.qual.size() - qbefore) < len) {           // quality lines
                eol = (const char *)std::memchr(buf + i, '\n', n - i);
                size_t e = eol ? (size_t)(eol - buf) : n, e2 = e;
                while (e2 > i && !std::isgraph((unsigned char)buf[e2 - 1])) --e2;
                size_t take = e2 - i, room = (size_t)len - (rs.qual.size() - qbefore);
                if (take > room) take = room;
                rs.qual.insert(rs.qual.end(), buf + i, buf + i + take);
                i = e < n ? e + 1 : n;
            }
            any_qual = true;
        }
        rs.qual.resize(qbefore + (size_t)len, '!');
        ++rs.n;
    }
}

// ---- record boundaries ----------------------------------------------------------------------------------------
// A piece of the input must begin at a record.  A line that starts with '@' need not be a header (a quality string may
// start with '@'), so a candidate is VERIFIED by walking the record: header, sequence lines up to the '+' line, quality
// lines holding exactly as many characters as the sequence -- and what follows must be the next header or the end.
// Returns the index behind the record (the start of the next one); 0 if [i, n) does not hold a whole well-formed record
// at i.  at_eof: n is the end of the input (the last line may lack its newline).
static size_t record_end(const char *b, size_t i, size_t n, bool at_eof)
{
    if (i >= n) return 0;
    auto line_end = [&](size_t p) { const char *e = (const char *)std::memchr(b + p, '\n', n - p); return e ? (size_t)(e - b) : n; };
    auto graph_len = [&](size_t p, size_t e) { while (e > p && !std::isgraph((unsigned char)b[e - 1])) --e; return e - p; };
    if (b[i] == '>') {                                   // FASTA: up to the next '>' at a line start
        size_t p = line_end(i);
        if (p >= n) return at_eof ? n : 0;
        for (++p; p < n; ) { if (b[p] == '>') return p; const size_t e = line_end(p); if (e >= n) return at_eof ? n : 0; p = e + 1; }
        return at_eof ? n : 0;
    }
    if (b[i] != '@') return 0;
    size_t p = line_end(i);
    if (p >= n) return 0;
    ++p;
    size_t S = 0, Q = 0;
    for (;;) {                                           // sequence lines
        if (p >= n) return 0;
        if (b[p] == '+') break;
        const size_t e = line_end(p);
        if (e >= n) return 0;
        S += graph_len(p, e); p = e + 1;
    }
    if (S == 0) return 0;                                // no boundary is placed on an empty record: a quality line '@..' followed by
                                                         // one '+..' and one '@..' would verify as one
    { const size_t e = line_end(p); if (e >= n) return 0; p = e + 1; }       // the '+' line
    while (Q < S) {                                      // quality lines
        if (p >= n) return 0;
        const size_t e = line_end(p);
        Q += graph_len(p, e);
        if (e >= n) return (Q == S && at_eof) ? n : 0;
        p = e + 1;
    }
    if (Q != S) return 0;
    if (p < n && b[p] != '@') return 0;
    return p;
}
// first verified record start at or behind `from` (a line start is looked for first), looking at no more than max_lines
// lines; n if there is none.  One record can verify by coincidence when the candidate is a quality line (header and
// sequence of the next record counted as "sequence", lengths happening to add up), so three records in a row must verify
// -- or the input must end behind fewer (at_eof only: a window of a stream that ends earlier rejects the candidate).
static size_t find_record_start(const char *b, size_t from, size_t n, bool at_eof, int max_lines, char mark /* '@' FASTQ, '>' FASTA: the input's first byte */)
{
    size_t i = from;
    if (i > 0 && i < n && b[i - 1] != '\n') { const char *e = (const char *)std::memchr(b + i, '\n', n - i); i = e ? (size_t)(e - b) + 1 : n; }
    for (int t = 0; t < max_lines && i < n; ++t) {
        if (b[i] == mark) {                              // (a FASTQ quality line may start with '>' as well as with '@')
            size_t p = i; int good = 0;
            for (; good < 3 && p < n; ++good) { const size_t e = record_end(b, p, n, at_eof); if (!e) break; p = e; }
            if (good == 3 || (good > 0 && p >= n && at_eof)) return i;
        }
        const char *e = (const char *)std::memchr(b + i, '\n', n - i);
        i = e ? (size_t)(e - b) + 1 : n;
    }
    return n;
}
// record starts that split [lo, hi) of the file image into about `parts` pieces; a cut is made only where a record start
// verifies -- otherwise that piece simply stays larger
static std::vector<size_t> cut_records(const char *b, size_t lo, size_t hi, int parts)
{
    std::vector<size_t> cut(1, lo);
    if (parts > 1 && hi - lo > (size_t)(1 << 20) && (b[lo] == '@' || b[lo] == '>')) {
        for (int t = 1; t < parts; ++t) {
            const size_t i = find_record_start(b, lo + (hi - lo) / (size_t)parts * (size_t)t, hi, true, 64, b[lo]);
            if (i < hi && i > cut.back()) cut.push_back(i);
        }
    }
    cut.push_back(hi);
    return cut;
}
static double g_t_fread = 0, g_t_cut = 0, g_t_par = 0, g_t_merge = 0;   // PS_VERBOSE >= 2: where the parser's time goes
// parse [lo, hi) of the file image on `threads` threads and APPEND the reads to rs.  Every thread parses its range into arrays of its
// own; the ranges' sizes then give every range its place in rs, and the threads copy their parts there side by side (one thread
// joining the parts cost more than the parsing: 0.5 s against 0.3 s per 5 M reads on 8 cores).
static void parse_span(const char *b, size_t lo, size_t hi, int threads, ReadSet &rs)
{
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    const auto tc0 = std::chrono::steady_clock::now();
    const std::vector<size_t> cut = cut_records(b, lo, hi, threads);
    const int parts = (int)cut.size() - 1;
    const auto tc1 = std::chrono::steady_clock::now();
    std::vector<ReadSet> piece((size_t)parts);
    std::vector<char> anyq((size_t)parts, 0);
    auto work = [&](int t) {
        ReadSet &r = piece[t];
        const size_t bytes = cut[t + 1] - cut[t];
        r.seq.reserve(bytes / 2 + 64); r.qual.reserve(bytes / 2 + 64);          // a FASTQ record is at most half bases
        r.off.push_back(0); r.name_off.push_back(0);
        bool aq = false;
        parse_reads_range(b, cut[t], cut[t + 1], r, aq);
        anyq[t] = aq;
    };
    auto fan = [&](const std::function<void(int)> &f) { std::vector<std::thread> th; for (int t = 1; t < parts; ++t) th.emplace_back(f, t); f(0); for (auto &x : th) x.join(); };
    fan(work);
    const auto tc2 = std::chrono::steady_clock::now();
    g_t_cut += std::chrono::duration<double>(tc1 - tc0).count(); g_t_par += std::chrono::duration<double>(tc2 - tc1).count();
    if (rs.off.empty()) { rs.off.push_back(0); rs.name_off.push_back(0); }
    std::vector<size_t> n0((size_t)parts + 1), s0((size_t)parts + 1), m0((size_t)parts + 1);
    n0[0] = (size_t)rs.n; s0[0] = rs.seq.size(); m0[0] = rs.names.size();
    bool any_qual = rs.has_qual;
    for (int t = 0; t < parts; ++t) {
        n0[t + 1] = n0[t] + (size_t)piece[t].n; s0[t + 1] = s0[t] + piece[t].seq.size(); m0[t + 1] = m0[t] + piece[t].names.size();
        any_qual = any_qual || anyq[t];
    }
    const size_t tn = n0[parts], ts = s0[parts], tm = m0[parts];
    auto grow = [](auto &v, size_t need) { if (v.capacity() < need) v.reserve(need + need / 2); v.resize(need); };     // in large steps: a piece is appended to window by window
    grow(rs.len, tn); grow(rs.off, tn + 1); grow(rs.name_off, tn + 1); grow(rs.seq, ts); grow(rs.qual, ts); grow(rs.names, tm);
    auto place = [&](int t) {
        ReadSet &r = piece[t];
        if (r.n == 0) return;
        std::memcpy(rs.len.data() + n0[t], r.len.data(), (size_t)r.n * sizeof(int32_t));
        int64_t *o = rs.off.data() + n0[t], *m = rs.name_off.data() + n0[t];
        const int64_t so = (int64_t)s0[t], no = (int64_t)m0[t];
        for (int64_t k = 1; k <= r.n; ++k) { o[k] = r.off[k] + so; m[k] = r.name_off[k] + no; }
        std::memcpy(rs.seq.data() + s0[t], r.seq.data(), r.seq.size());
        std::memcpy(rs.qual.data() + s0[t], r.qual.data(), r.qual.size());
        std::memcpy(rs.names.data() + m0[t], r.names.data(), r.names.size());
        r = ReadSet();
    };
    fan(place);
    rs.n = (int64_t)tn; rs.has_qual = any_qual;
    g_t_merge += std::chrono::duration<double>(std::chrono::steady_clock::now() - tc2).count();
}
static void parser_times(int threads)
{
    if (const char *e = std::getenv("PS_VERBOSE")) if (std::atoi(e) >= 2)
        std::fprintf(stderr, "[parasuite-hip]     parser: reading %.0f ms, cutting %.0f ms, parsing on %d threads %.0f ms, placing the threads' parts %.0f ms (sums over the windows)\n", 1e3 * g_t_fread, 1e3 * g_t_cut, threads, 1e3 * g_t_par, 1e3 * g_t_merge);
    g_t_fread = g_t_cut = g_t_par = g_t_merge = 0;
}
// A FASTQ input that was cut off behind the '+' line of its last record: "@name", one sequence line, "+..." and the end.  The record
// has bases and no quality line, and the input fails the call (the parser would make up qualities for it).  b[0, n) is the end of
// the input from a record start on; only this plain shape is recognised, every other end of an input is parsed as it was.
static void refuse_cut_off_fastq(const char *b, size_t n, const char *path)
{
    size_t e = n;
    while (e > 0 && !std::isgraph((unsigned char)b[e - 1])) --e;              // blanks and line ends behind the last line
    auto line_start = [&](size_t end) { size_t s = end; while (s > 0 && b[s - 1] != '\n') --s; return s; };
    if (e == 0) return;
    const size_t l1 = line_start(e);                                          // the last line: a '+' line?
    if (b[l1] != '+' || l1 < 2) return;
    const size_t l2 = line_start(l1 - 1);                                     // before it: one line of bases
    if (l2 < 2 || l2 == l1 - 1 || b[l2] == '+' || b[l2] == '@') return;
    const size_t l3 = line_start(l2 - 1);                                     // before that: the header
    if (b[l3] != '@' || record_end(b, l3, n, true) != 0) return;
    size_t m = l3 + 1;
    while (m < l2 && !std::isspace((unsigned char)b[m])) ++m;
    throw Error(std::string(path) + ": the last FASTQ record (" + std::string(b + l3 + 1, m - l3 - 1) + ") is cut off after its '+' line: it has no quality line");
}

void load_reads(const char *path, ReadSet &rs, int threads)
{
    rs = ReadSet();
    load_reads_chunked(path, threads, ~(size_t)0 >> 2, [&](ReadSet &&piece) { rs = std::move(piece); });
    if (rs.off.empty()) { rs.off.push_back(0); rs.name_off.push_back(0); }
}

void load_reads_chunked(const char *path, int threads, size_t chunk_bytes, const std::function<void(ReadSet &&)> &sink, size_t first_bytes,
                        const std::function<bool()> *hungry, size_t hungry_min_bytes)
{
    if (chunk_bytes < 4096) chunk_bytes = 4096;
    size_t unit = (size_t)64 << 20;
    if (const char *e = std::getenv("PS_UNIT_MB")) unit = (size_t)std::max(1, std::atoi(e)) << 20;
    unit = std::min(unit, chunk_bytes);
    // plain, gzip or BGZF (ps_inflate.h); a compressed input's text has no known size and takes the branches a FIFO takes below
    ByteSource src(path, "cannot open reads ", unit);
    const bool sized = src.size_known();             // a plain regular file
    const off_t text_bytes = sized ? (off_t)src.size() : 0;
    // the first piece may be smaller (the stages behind the parser start sooner), the following ones double up to chunk_bytes
    size_t cur = first_bytes && first_bytes < chunk_bytes ? std::max<size_t>(first_bytes, 4096) : chunk_bytes;
    RawVec<char> buf; size_t have = 0; bool eof = false; char mark = 0; off_t file_at = 0;
    ReadSet acc; size_t acc_bytes = 0;
    auto flush = [&]() { if (acc.n) { sink(std::move(acc)); cur = std::min(chunk_bytes, cur * 2); } acc = ReadSet(); acc_bytes = 0; };
    while (!eof || have) {
        const size_t fine = std::min<size_t>((size_t)1 << 20, unit);                                  // a piece ends within this of its size
        const size_t win = std::min(unit, cur > acc_bytes + fine ? cur - acc_bytes : unit);          // the last window of a piece is what is missing to its size (a piece already at its size is taking the end of the input along: whole windows)
        const size_t want = win > have ? win : have + win;       // what is carried over from a window that could not be cut fills a window alone: it grows
        if (buf.size() < want + 1) buf.resize(want + 1);
        const auto tr0 = std::chrono::steady_clock::now();
        if (!eof && have < want) {
            const size_t got = src.read(buf.data() + have, want - have, threads);
            if (got < want - have) eof = true;
            have += got; file_at += (off_t)got;
        }
        g_t_fread += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
        if (!mark && have) mark = buf[0];
        size_t cut = have;
        if (!eof) {
            // the last record start that verifies: walk records from a start found in the window's last 256 KB
            const size_t from = have > ((size_t)256 << 10) ? have - ((size_t)256 << 10) : 0;
            size_t i = find_record_start(buf.data(), from, have, false, 4096, mark), last = 0;
            while (i < have) { last = i; const size_t e = record_end(buf.data(), i, have, false); if (!e || e >= have) break; i = e; }
            if (last == 0) continue;                                               // nothing to cut at: the window grows
            cut = last;
        }
        if (eof && cut && mark == '@') refuse_cut_off_fastq(buf.data(), cut, path);
        if (cut) {
            const size_t tiny = cur / 8;                                                                       // an end of the input not worth a launch of its own
            const bool to_the_end = sized && (size_t)std::max<off_t>(0, text_bytes - file_at) + have <= tiny;  // this window and all behind it
            if (acc_bytes && acc_bytes + cut > cur + fine && !to_the_end) flush();    // this window would take the piece well over its size (a window that had to grow)
            const bool first_window = acc.n == 0;
            parse_span(buf.data(), 0, cut, threads, acc);
            if (first_window && acc.n && cur > cut && cur < (~(size_t)0 >> 3)) {     // a piece's arrays are sized once, from what its first window held
                const double f = 1.05 * (double)cur / (double)cut;
                acc.len.reserve((size_t)(f * (double)acc.n) + 64); acc.off.reserve((size_t)(f * (double)acc.n) + 65); acc.name_off.reserve((size_t)(f * (double)acc.n) + 65);
                acc.seq.reserve((size_t)(f * (double)acc.seq.size()) + 64); acc.qual.reserve((size_t)(f * (double)acc.seq.size()) + 64);
                acc.names.reserve((size_t)(f * (double)acc.names.size()) + 64);
            }
            acc_bytes += cut;
            // no piece is cut off just in front of the end of the input: what is left would be a launch of its own (>= 0.3 s for 0.6 M reads,
            // measured) -- the piece takes it along, up to an eighth over its size
            const size_t rest = sized ? (size_t)std::max<off_t>(0, text_bytes - file_at) + (have - cut) : ~(size_t)0;
            const bool tiny_rest = !eof && rest <= tiny;
            if (!tiny_rest && (acc_bytes + fine > cur || (hungry && acc_bytes >= hungry_min_bytes && (*hungry)()))) flush();
        }
        std::memmove(buf.data(), buf.data() + cut, have - cut);
        have -= cut;
        if (eof && cut == 0) break;
    }
    flush();
    parser_times(threads);
}

void reads_from_codes(int64_t n, int len, const uint8_t *codes, ReadSet &rs)
{
    rs = ReadSet();
    rs.n = n; rs.len.assign((size_t)n, len); rs.off.resize((size_t)n + 1); rs.name_off.resize((size_t)n + 1);
    rs.seq.assign(codes, codes + (size_t)n * len);
    for (auto &c : rs.seq) if (c > 4) c = 4;
    char nm[32];
    rs.name_off[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        rs.off[i] = i * len;
        int l = std::snprintf(nm, sizeof nm, "r%lld", (long long)i);
        rs.names.insert(rs.names.end(), nm, nm + l);
        rs.name_off[i + 1] = (int64_t)rs.names.size();
    }
    rs.off[n] = n * (int64_t)len;
    rs.has_qual = false;
}

// host-only: parse reads the way ps_map does (whole file on `threads` threads, or streamed in windows of chunk_bytes) and
// summarise what came out -- {reads, bases, order-sensitive hash of names/sequences/qualities, pieces}
void parse_check(const char *reads_path, int threads, size_t chunk_bytes, uint64_t out[4])
{
    uint64_t n = 0, bases = 0, h = 1469598103934665603ull, pieces = 0;
    auto mix = [&](const void *p, size_t len) { const unsigned char *c = (const unsigned char *)p; for (size_t i = 0; i < len; ++i) { h ^= c[i]; h *= 1099511628211ull; } h ^= 0xff; h *= 1099511628211ull; };
    auto eat = [&](const ReadSet &rs) {
        ++pieces;
        for (int64_t i = 0; i < rs.n; ++i) {
            size_t nl; const char *nm = rs.name(i, nl);
            mix(nm, nl); mix(rs.seq.data() + rs.off[i], (size_t)rs.len[i]); mix(rs.qual.data() + rs.off[i], (size_t)rs.len[i]);
            bases += (uint64_t)rs.len[i];
        }
        n += (uint64_t)rs.n;
    };
    if (chunk_bytes == 0) { ReadSet rs; load_reads(reads_path, rs, threads); eat(rs); }
    else if (const char *e = std::getenv("PS_PARSE_CHECK_HUNGRY")) {       // tests: a consumer that always waits, as ps_map's GPU worker does at the start: pieces go out at `e` bytes
        const std::function<bool()> hungry = []() { return true; };
        load_reads_chunked(reads_path, threads, chunk_bytes, [&](ReadSet &&rs) { eat(rs); }, 0, &hungry, (size_t)std::max(1, std::atoi(e)));
    }
    else load_reads_chunked(reads_path, threads, chunk_bytes, [&](ReadSet &&rs) { eat(rs); });
    out[0] = n; out[1] = bases; out[2] = h; out[3] = pieces;
}

}  // namespace ps
