// ps_bam.cpp -- SAM text -> BAM (BGZF), MAPQ filter, coordinate / name sort and .bai index, on SAM or BAM input.
//
// §8f rank 3: what /root/reference/src/src/mapping/PARAsuiteMapping.java:102-133 (`samtools view -bS`,
// `samtools view -q <mapq> -b`) and Mapping.java:85-108 (`samtools sort`, `samtools index`) spawn four
// processes and three rewrites of the data for.  Formats follow the public SAM/BAM specification (SAMv1:
// BGZF blocks of at most 64 KiB with the BC extra field, BAM records, binning index with 16 kb linear index);
// integer tags take the smallest type as htslib's SAM parser does.  Host code only (zlib), no device work in this file: the BGZF
// blocks of every writer go through bgzf_batch(), which hands them to the device compressor when one is registered (ps_bam.h), and
// every sort through sort_for_write(), which hands sort and gather to the hook registered for its order (ps_bamsort.hip) the same way
// and returns the body of the file (ps_bam.h: BamBody) that write_bam then writes.
// PS_VERBOSE: write_bam prints one line with the ms of its stages (sort, offsets + gather, compression, file write, .bai) on stderr.
#include <zlib.h>
#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#include "ps_bam.h"
#include "ps_error.h"
#include "ps_inflate.h"
#include "ps_java.h"

namespace ps {
namespace {

inline void put32(std::string &o, uint32_t v) { char b[4] = {(char)(v & 0xff), (char)((v >> 8) & 0xff), (char)((v >> 16) & 0xff), (char)(v >> 24)}; o.append(b, 4); }
inline void put16(std::string &o, uint16_t v) { char b[2] = {(char)(v & 0xff), (char)(v >> 8)}; o.append(b, 2); }
inline void put64(std::string &o, uint64_t v) { put32(o, (uint32_t)v); put32(o, (uint32_t)(v >> 32)); }

// UCSC binning scheme (SAMv1 §5.3)
inline int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

typedef BamRec Rec;        // encoded record: bytes [off, off+len) of its part

struct Field { const char *p; size_t n; };

static int base4(char c)
{
    switch (c) {
        case '=': return 0; case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'M': case 'm': return 3;
        case 'G': case 'g': return 4; case 'R': case 'r': return 5; case 'S': case 's': return 6; case 'V': case 'v': return 7;
        case 'T': case 't': return 8; case 'W': case 'w': return 9; case 'Y': case 'y': return 10; case 'H': case 'h': return 11;
        case 'K': case 'k': return 12; case 'D': case 'd': return 13; case 'B': case 'b': return 14; default: return 15;
    }
}
static long to_long(Field f) { return std::strtol(std::string(f.p, f.n).c_str(), nullptr, 10); }

// one SAM alignment line -> BAM record appended to o; false if filtered out
static bool encode_line(const char *line, size_t n, const std::map<std::string, int> &ref_id, int min_mapq, std::string &o, Rec &r)
{
    Field f[11]; size_t i = 0; int k = 0;
    while (k < 11) {
        const char *e = (const char *)std::memchr(line + i, '\t', n - i);
        size_t j = e ? (size_t)(e - line) : n;
        f[k].p = line + i; f[k].n = j - i; ++k;
        i = j < n ? j + 1 : n;
        if (!e && k < 11) throw Error("SAM line with fewer than 11 fields: " + std::string(line, std::min<size_t>(n, 80)));
    }
    const long flag = to_long(f[1]), pos1 = to_long(f[3]), mapq = to_long(f[4]), pnext1 = to_long(f[7]), tlen = to_long(f[8]);
    if (mapq < min_mapq) return false;
    int ref = -1, rnext = -1;
    if (!(f[2].n == 1 && f[2].p[0] == '*')) {
        auto it = ref_id.find(std::string(f[2].p, f[2].n));
        if (it == ref_id.end()) throw Error("reference name not in the header: " + std::string(f[2].p, f[2].n));
        ref = it->second;
    }
    if (f[6].n == 1 && f[6].p[0] == '=') rnext = ref;
    else if (!(f[6].n == 1 && f[6].p[0] == '*')) {
        auto it = ref_id.find(std::string(f[6].p, f[6].n));
        if (it == ref_id.end()) throw Error("mate reference name not in the header");
        rnext = it->second;
    }
    // CIGAR
    std::vector<uint32_t> cig;
    int64_t ref_len = 0;
    if (!(f[5].n == 1 && f[5].p[0] == '*')) {
        uint32_t num = 0; bool any = false;
        for (size_t c = 0; c < f[5].n; ++c) {
            const char ch = f[5].p[c];
            if (ch >= '0' && ch <= '9') { num = num * 10 + (uint32_t)(ch - '0'); any = true; continue; }
            static const char ops[] = "MIDNSHP=X";
            const char *w = std::strchr(ops, ch);
            if (!w || !any) throw Error("bad CIGAR: " + std::string(f[5].p, f[5].n));
            const int op = (int)(w - ops);
            cig.push_back((num << 4) | (uint32_t)op);
            if (cigar_on_ref(op)) ref_len += num;
            num = 0; any = false;
        }
    }
    const int32_t pos = (int32_t)pos1 - 1;
    const int64_t end = pos + (ref_len > 0 ? ref_len : 1);
    const bool has_seq = !(f[9].n == 1 && f[9].p[0] == '*');
    const uint32_t l_seq = has_seq ? (uint32_t)f[9].n : 0;
    BamCore core{ref, pos, end, (int)mapq, (int)flag, (uint32_t)cig.size(), l_seq, rnext, (int32_t)pnext1 - 1, (int32_t)tlen};
    bam_rec_begin(o, core, f[0].p, f[0].n, r);
    bam_rec_cigar(o, cig.data(), cig.size());
    for (uint32_t c = 0; c < l_seq; c += 2) {
        const int hi = base4(f[9].p[c]), lo = c + 1 < l_seq ? base4(f[9].p[c + 1]) : 0;
        o.push_back((char)(uint8_t)((hi << 4) | lo));
    }
    if (f[10].n == 1 && f[10].p[0] == '*') o.append((size_t)l_seq, (char)0xff);
    else {
        if (f[10].n != l_seq) throw Error("SEQ and QUAL of different length");
        for (uint32_t c = 0; c < l_seq; ++c) o.push_back((char)(uint8_t)(f[10].p[c] - 33));
    }
    // optional fields TAG:TYPE:VALUE
    while (i < n) {
        const char *e = (const char *)std::memchr(line + i, '\t', n - i);
        const size_t j = e ? (size_t)(e - line) : n;
        const char *t = line + i; const size_t tn = j - i;
        i = j < n ? j + 1 : n;
        if (tn == 0) continue;
        if (tn < 5 || t[2] != ':' || t[4] != ':') throw Error("bad optional field: " + std::string(t, tn));
        const char ty = t[3]; const char *v = t + 5; const size_t vn = tn - 5;
        if (ty == 'A') bam_tag_char(o, t, vn ? v[0] : ' ');
        else if (ty == 'i') bam_tag_int(o, t, std::strtoll(std::string(v, vn).c_str(), nullptr, 10));
        else if (ty == 'f') { o.append(t, 2); o.push_back('f'); float fl = std::strtof(std::string(v, vn).c_str(), nullptr); uint32_t u; std::memcpy(&u, &fl, 4); put32(o, u); }
        else if (ty == 'Z' || ty == 'H') bam_tag_text(o, t, ty, v, vn);
        else throw Error(std::string("optional field type not supported: ") + ty);
    }
    bam_rec_end(o, r);
    return true;
}

// one BGZF block (gzip member with the BC extra field) of at most kBgzfBlock input bytes
static void bgzf_block(const char *src, size_t n, int level, std::string &out)
{
    std::vector<unsigned char> buf(n + n / 100 + 64);
    z_stream zs; std::memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw Error("deflateInit2 failed");
    zs.next_in = (Bytef *)const_cast<char *>(src); zs.avail_in = (uInt)n;
    zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { deflateEnd(&zs); throw Error("deflate failed"); }
    const size_t cn = zs.total_out;
    deflateEnd(&zs);
    if (18 + cn + 8 > 65536) throw Error("BGZF block too large");
    bgzf_member(buf.data(), cn, (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)src, (uInt)n), (uint32_t)n, out);
}

template <class F> static void par(int n, int threads, F f)
{
    std::vector<std::thread> th; std::vector<std::string> err((size_t)n);
    int next = 0;
    while (next < n) {
        th.clear();
        for (int t = 0; t < threads && next < n; ++t, ++next) { const int id = next; th.emplace_back([&, id]() { try { f(id); } catch (const std::exception &e) { err[id] = e.what(); if (err[id].empty()) err[id] = "error"; } }); }
        for (auto &x : th) x.join();
    }
    for (auto &e : err) if (!e.empty()) throw Error(e);
}

// The one place where BGZF blocks are made: comp[k] becomes the whole member (header, deflate payload, CRC32, ISIZE) of spans[k],
// each span at most kBgzfBlock bytes.  On host threads with zlib (bgzf_host_compress), or -- the whole list at once -- by the
// compressor that the library registered (ps_bgzf.hip: ps_bgzf_device, PS_BGZF_GPU); `level` means nothing to that one.
std::atomic<BgzfBatchFn> g_bgzf_device{nullptr};
static void bgzf_batch(const std::vector<BgzfSpan> &spans, int level, int threads, std::vector<std::string> &comp)
{
    comp.assign(spans.size(), std::string());
    if (spans.empty()) return;
    if (const BgzfBatchFn fn = g_bgzf_device.load()) fn(spans.data(), spans.size(), comp.data());
    else bgzf_host_compress(spans.data(), spans.size(), level, threads, comp.data());
}

static int clamp_threads(int t) { return t < 1 ? 1 : (t > 64 ? 64 : t); }

}  // namespace

void bgzf_set_device_compressor(BgzfBatchFn fn) { g_bgzf_device.store(fn); }
void bgzf_member(const void *payload, size_t n_payload, uint32_t crc, uint32_t isize, std::string &out)
{
    static const unsigned char head[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0};
    const size_t total = 18 + n_payload + 8;
    out.reserve(out.size() + total);
    out.append((const char *)head, 16); put16(out, (uint16_t)(total - 1));
    out.append((const char *)payload, n_payload);
    put32(out, crc); put32(out, isize);
}
void bgzf_host_compress(const BgzfSpan *spans, size_t n_spans, int level, int threads, std::string *comp)
{
    const int T = clamp_threads(threads);
    for (size_t k = 0; k < n_spans; ++k) { if (spans[k].n > kBgzfBlock) throw Error("a BGZF span of more than 0xff00 bytes"); comp[k].clear(); }
    par(T, T, [&](int t) { for (size_t k = (size_t)t; k < n_spans; k += (size_t)T) bgzf_block(spans[k].p, spans[k].n, level, comp[k]); });
}

namespace {

struct Data {                       // a BAM in memory: header, reference table, encoded records in parts
    std::string text; std::vector<std::pair<std::string, uint32_t>> refs;
    std::vector<std::string> enc; std::vector<Rec> recs; uint64_t n_in = 0;
};

static void header_sorted(std::string &text, const char *so)
{
    if (text.compare(0, 3, "@HD") == 0) {
        const size_t e = text.find('\n');
        std::string hd = text.substr(0, e);
        const size_t at = hd.find("\tSO:");
        if (at != std::string::npos) { size_t q = hd.find('\t', at + 1); hd.erase(at, (q == std::string::npos ? hd.size() : q) - at); }
        hd += std::string("\tSO:") + so;
        text = hd + text.substr(e);
    } else text = std::string("@HD\tVN:1.6\tSO:") + so + "\n" + text;
}

// ---- SAM text -> Data
static void load_sam(const char *sam_path, int min_mapq, int threads, Data &d)
{
    FILE *f = std::fopen(sam_path, "rb");
    if (!f) throw Error(std::string("cannot open ") + sam_path);
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    std::vector<char> buf((size_t)sz + 1);
    if (sz && std::fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) { std::fclose(f); throw Error(std::string("short read on ") + sam_path); }
    std::fclose(f);
    const size_t n = (size_t)sz; const char *b = buf.data();
    std::map<std::string, int> ref_id;
    size_t body = 0;
    while (body < n && b[body] == '@') {
        const char *e = (const char *)std::memchr(b + body, '\n', n - body);
        const size_t j = e ? (size_t)(e - b) : n;
        std::string line(b + body, j - body);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.compare(0, 3, "@SQ") == 0) {
            std::string name; long ln = 0; size_t p = 0;
            while (p < line.size()) {
                size_t q = line.find('\t', p); if (q == std::string::npos) q = line.size();
                if (line.compare(p, 3, "SN:") == 0) name = line.substr(p + 3, q - p - 3);
                else if (line.compare(p, 3, "LN:") == 0) ln = std::strtol(line.substr(p + 3, q - p - 3).c_str(), nullptr, 10);
                p = q + 1;
            }
            if (name.empty() || ln <= 0) throw Error("bad @SQ line: " + line);
            ref_id[name] = (int)d.refs.size(); d.refs.emplace_back(name, (uint32_t)ln);
        }
        d.text += line; d.text.push_back('\n');
        body = j < n ? j + 1 : n;
    }
    // records, encoded in parallel over ranges of whole lines
    std::vector<size_t> cut(1, body);
    for (int t = 1; t < threads; ++t) {
        size_t at = body + (n - body) / (size_t)threads * (size_t)t;
        const char *e = at < n ? (const char *)std::memchr(b + at, '\n', n - at) : nullptr;
        at = e ? (size_t)(e - b) + 1 : n;
        if (at > cut.back() && at < n) cut.push_back(at);
    }
    cut.push_back(n);
    const int parts = (int)cut.size() - 1;
    d.enc.assign((size_t)parts, std::string()); std::vector<std::vector<Rec>> recs((size_t)parts);
    std::vector<uint64_t> n_in((size_t)parts, 0);
    par(parts, threads, [&](int t) {
        std::string &o = d.enc[t]; o.reserve((cut[t + 1] - cut[t]));
        size_t i = cut[t];
        while (i < cut[t + 1]) {
            const char *e = (const char *)std::memchr(b + i, '\n', cut[t + 1] - i);
            size_t j = e ? (size_t)(e - b) : cut[t + 1], j2 = j;
            if (j2 > i && b[j2 - 1] == '\r') --j2;
            if (j2 > i) {
                Rec r; r.part = t;
                ++n_in[t];
                if (encode_line(b + i, j2 - i, ref_id, min_mapq, o, r)) recs[t].push_back(r);
            }
            i = j + 1;
        }
    });
    size_t m = 0; for (auto &v : recs) m += v.size();
    d.recs.reserve(m);
    for (int t = 0; t < parts; ++t) { d.recs.insert(d.recs.end(), recs[t].begin(), recs[t].end()); d.n_in += n_in[t]; }
}

// ---- BGZF file -> uncompressed bytes; block starts (compressed offset, uncompressed offset)
struct Blocks { std::string data; std::vector<std::pair<uint64_t, uint64_t>> starts; uint64_t file_bytes = 0; };
static void inflate_bgzf(const char *path, int threads, Blocks &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) throw Error(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    std::vector<unsigned char> raw((size_t)sz);
    if (sz && std::fread(raw.data(), 1, (size_t)sz, f) != (size_t)sz) { std::fclose(f); throw Error(std::string("short read on ") + path); }
    std::fclose(f);
    out.file_bytes = (uint64_t)sz;
    // the header and the inflate of one block are ps_inflate.h's, shared with the byte source of the text inputs
    struct B { size_t at, bsize, hl; uint32_t isize; uint64_t u; };
    std::vector<B> bl; size_t at = 0; uint64_t u = 0;
    while (at < raw.size()) {
        size_t hl = 0, bsize = 0; const char *why = nullptr;
        if (gz_member_header(raw.data() + at, raw.size() - at, hl, bsize, why) <= 0 || bsize < hl + 8) throw Error(std::string("not a BGZF file: ") + path);
        if (at + bsize > raw.size()) throw Error(std::string("truncated BGZF block in ") + path);
        const uint32_t isize = bgzf_isize(raw.data() + at, bsize);
        if (isize > kBgzfMaxOut) throw Error(std::string("corrupt BGZF block in ") + path);
        bl.push_back(B{at, bsize, hl, isize, u});
        u += isize; at += bsize;
    }
    out.data.assign((size_t)u, '\0');
    out.starts.clear();
    for (const B &b : bl) out.starts.emplace_back((uint64_t)b.at, b.u);
    const int T = threads;
    par(T, T, [&](int t) {
        for (size_t k = (size_t)t; k < bl.size(); k += (size_t)T) {
            const B &b = bl[k];
            if (const char *e = bgzf_inflate_block(raw.data() + b.at, b.bsize, b.hl, b.isize ? &out.data[(size_t)b.u] : nullptr, b.isize))
                throw Error(std::string("corrupt BGZF block in ") + path + ": " + e + " at compressed byte " + std::to_string(b.at));
        }
    });
}
static uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint32_t rd32(const std::string &s, size_t at) { return rd32((const uint8_t *)s.data() + at); }

// ---- BAM file -> Data (records stay as they are; their place in the file is kept for indexing)
static void load_bam(const char *path, int threads, Data &d, Blocks *keep_blocks, std::vector<uint64_t> *rec_u)
{
    Blocks local; Blocks &bk = keep_blocks ? *keep_blocks : local;
    inflate_bgzf(path, threads, bk);
    const std::string &s = bk.data;
    if (s.size() < 12 || s.compare(0, 4, "BAM\1") != 0) throw Error(std::string("not a BAM file: ") + path);
    const uint32_t l_text = rd32(s, 4);
    d.text = s.substr(8, l_text);
    while (!d.text.empty() && d.text.back() == '\0') d.text.pop_back();
    size_t at = 8 + (size_t)l_text;
    const uint32_t n_ref = rd32(s, at); at += 4;
    for (uint32_t r = 0; r < n_ref; ++r) {
        const uint32_t ln = rd32(s, at);
        d.refs.emplace_back(s.substr(at + 4, ln ? ln - 1 : 0), rd32(s, at + 4 + ln));
        at += 8 + (size_t)ln;
    }
    d.enc.assign(1, std::string());
    d.enc[0].assign(s, at, std::string::npos);
    const std::string &e = d.enc[0];
    const size_t base_u = at;
    size_t p = 0;
    while (p + 4 <= e.size()) {
        const uint32_t bs = rd32(e, p);
        if (bs < 32 || p + 4 + bs > e.size()) throw Error(std::string("corrupt BAM record in ") + path);
        Rec r; r.part = 0; r.off = p; r.len = 4 + (size_t)bs;
        r.ref = (int32_t)rd32(e, p + 4); r.pos = (int32_t)rd32(e, p + 8);
        const uint32_t w = rd32(e, p + 12), fl = rd32(e, p + 16);
        const uint32_t l_name = w & 0xff, n_cig = fl & 0xffff;
        r.flag = fl >> 16;
        int64_t ref_len = 0;
        const size_t cig_at = p + 36 + l_name;                   // words beyond the record's end (a corrupt record: flatten_records names it) are not read
        for (uint32_t c = 0; c < n_cig && cig_at + 4 * c + 4 <= p + 4 + bs; ++c) { const uint32_t v = rd32(e, cig_at + 4 * c); if (cigar_on_ref((int)(v & 15))) ref_len += v >> 4; }
        r.end = (int32_t)(r.pos + (ref_len > 0 ? ref_len : 1));
        d.recs.push_back(r);
        if (rec_u) rec_u->push_back((uint64_t)(base_u + p));
        p += 4 + bs;
    }
    d.n_in = d.recs.size();
    if (!keep_blocks) { bk.data.clear(); bk.data.shrink_to_fit(); }
}
static int rec_mapq(const Data &d, const Rec &r) { return (int)((rd32(d.enc[r.part], r.off + 12) >> 8) & 0xff); }
static const char *rec_name(const Data &d, const Rec &r) { return d.enc[r.part].data() + r.off + 36; }

// read names as `samtools sort -n` orders them: digit runs compare as numbers
static int strnum_cmp(const char *a, const char *b)
{
    const unsigned char *pa = (const unsigned char *)a, *pb = (const unsigned char *)b;
    while (*pa && *pb) {
        if (std::isdigit(*pa) && std::isdigit(*pb)) {
            while (*pa == '0') ++pa;
            while (*pb == '0') ++pb;
            const unsigned char *ea = pa, *eb = pb;
            while (std::isdigit(*ea)) ++ea;
            while (std::isdigit(*eb)) ++eb;
            if (ea - pa != eb - pb) return (ea - pa) < (eb - pb) ? -1 : 1;
            for (; pa < ea; ++pa, ++pb) if (*pa != *pb) return *pa < *pb ? -1 : 1;
        } else {
            if (*pa != *pb) return *pa < *pb ? -1 : 1;
            ++pa; ++pb;
        }
    }
    return *pa ? 1 : (*pb ? -1 : 0);
}

// virtual offsets of the records of an existing layout, then the .bai
struct Layout { std::vector<uint64_t> vbeg, vend; };
static void write_bai(const std::string &bai_path, const Data &d, const Layout &lay)
{
    struct RefIdx { std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins; std::vector<uint64_t> lin; uint64_t beg = 0, end = 0, n_map = 0, n_unmap = 0; bool any = false; };
    std::vector<RefIdx> idx(d.refs.size());
    uint64_t n_no_coor = 0;
    for (size_t i = 0; i < d.recs.size(); ++i) {
        const Rec &r = d.recs[i];
        if (r.ref < 0) { ++n_no_coor; continue; }
        if ((size_t)r.ref >= idx.size()) throw Error("record refers to a reference that is not in the header");
        RefIdx &x = idx[(size_t)r.ref];
        const uint64_t vb = lay.vbeg[i], ve = lay.vend[i];
        if (!x.any) { x.beg = vb; x.any = true; }
        x.end = ve;
        if (r.flag & 4) ++x.n_unmap; else ++x.n_map;
        const uint32_t bin = (uint32_t)reg2bin(r.pos, r.end);
        auto &ch = x.bins[bin];
        if (!ch.empty() && (ch.back().second >> 16 == vb >> 16 || ch.back().second == vb)) ch.back().second = ve;     // same compressed block or adjacent: extend
        else ch.emplace_back(vb, ve);
        const size_t w0 = (size_t)(r.pos >> 14), w1 = (size_t)((r.end - 1) >> 14);
        if (x.lin.size() <= w1) x.lin.resize(w1 + 1, 0);
        for (size_t w = w0; w <= w1; ++w) if (x.lin[w] == 0) x.lin[w] = vb;
    }
    std::string bai;
    bai.append("BAI\1", 4); put32(bai, (uint32_t)d.refs.size());
    for (RefIdx &x : idx) {
        put32(bai, (uint32_t)(x.bins.size() + (x.any ? 1 : 0)));
        for (auto &kv : x.bins) {
            put32(bai, kv.first); put32(bai, (uint32_t)kv.second.size());
            for (auto &c : kv.second) { put64(bai, c.first); put64(bai, c.second); }
        }
        if (x.any) { put32(bai, 37450u); put32(bai, 2u); put64(bai, x.beg); put64(bai, x.end); put64(bai, x.n_map); put64(bai, x.n_unmap); }
        for (size_t w = 1; w < x.lin.size(); ++w) if (x.lin[w] == 0) x.lin[w] = x.lin[w - 1];
        put32(bai, (uint32_t)x.lin.size());
        for (uint64_t v : x.lin) put64(bai, v);
    }
    put64(bai, n_no_coor);
    write_text_file(bai_path, bai);
}

using Clock = std::chrono::steady_clock;
static double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

static std::string bam_header(const Data &d)        // magic, l_text, text, n_ref, the references
{
    std::string head;
    head.append("BAM\1", 4); put32(head, (uint32_t)d.text.size()); head += d.text; put32(head, (uint32_t)d.refs.size());
    for (auto &r : d.refs) { put32(head, (uint32_t)r.first.size() + 1); head += r.first; head.push_back('\0'); put32(head, r.second); }
    return head;
}
static const unsigned char eof_block[28] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// the two orders, each stated once.  Coordinate: the reference id as unsigned (-1, no reference, sorts last), then the position.
// Name: strnum_cmp, then the first read of a pair before the second; name(r): where r's NUL-terminated name starts.
struct CoordinateLess { bool operator()(const Rec &x, const Rec &y) const { const uint32_t a = (uint32_t)x.ref, c = (uint32_t)y.ref; return a != c ? a < c : x.pos < y.pos; } };
template <class NameOf> static void sort_in_order(std::vector<Rec> &recs, bool by_name, NameOf name)
{
    if (by_name)
        std::stable_sort(recs.begin(), recs.end(), [&](const Rec &x, const Rec &y) {
            const int c = strnum_cmp(name(x), name(y));
            return c ? c < 0 : ((x.flag >> 6) & 3) < ((y.flag >> 6) & 3);
        });
    else std::stable_sort(recs.begin(), recs.end(), CoordinateLess());
}

// where every record starts when the records lie back to back in this order (n + 1 offsets), and their bytes put there on threads;
// part(r): the start of the buffer that r.off counts from
static std::vector<uint64_t> stream_offsets(const std::vector<Rec> &recs)
{
    std::vector<uint64_t> uoff(recs.size() + 1, 0);
    for (size_t i = 0; i < recs.size(); ++i) uoff[i + 1] = uoff[i] + recs[i].len;
    return uoff;
}
template <class PartOf> static void gather(const std::vector<Rec> &recs, const std::vector<uint64_t> &uoff, int T, char *dst, PartOf part)
{
    const size_t n = recs.size();
    par(T, T, [&](int t) { for (size_t i = n * (size_t)t / (size_t)T; i < n * ((size_t)t + 1) / (size_t)T; ++i) std::memcpy(dst + uoff[i], part(recs[i]) + recs[i].off, recs[i].len); });
}

// ---- Data (records in d.recs order) -> BGZF file (+ .bai).  body says where the records' bytes are (ps_bam.h); a device stream is
// used up, a host stream -- the sort's, or the one gathered here -- is left in body for the caller that keeps the file.  The parts are dropped.
static void write_bam(Data &d, BamBody &body, const char *bam_path, bool write_index, int threads, BamStats *stats, int level = 6)
{
    const bool verbose = std::getenv("PS_VERBOSE") != nullptr;
    double ms_gather = 0, ms_comp = 0, ms_file = 0, ms_bai = 0;
    Clock::time_point t0 = Clock::now();
    const std::string head = bam_header(d);
    const size_t BLK = kBgzfBlock;
    const size_t head_blocks = (head.size() + BLK - 1) / BLK;           // own blocks: samtools flushes after the header too
    const std::vector<Rec> &all = d.recs;
    const std::vector<uint64_t> uoff = stream_offsets(all);
    const uint64_t body_bytes = uoff[all.size()];
    const size_t body_blocks = (size_t)((body_bytes + BLK - 1) / BLK);
    const bool resident = body.device != nullptr, came_with_sort = !body.in_parts && !resident;
    if (body.in_parts) {
        body.host.assign((size_t)body_bytes, '\0');
        gather(all, uoff, threads, &body.host[0], [&](const Rec &r) { return d.enc[(size_t)r.part].data(); });
        body.in_parts = false;
    } else if (came_with_sort && body.host.size() != body_bytes) throw Error("internal: the sorted stream has not the records' size");
    for (auto &e : d.enc) { e.clear(); e.shrink_to_fit(); }
    ms_gather = ms_since(t0); t0 = Clock::now();
    const size_t n_blocks = head_blocks + body_blocks;
    std::vector<std::string> comp;
    {
        std::vector<BgzfSpan> spans; spans.reserve(n_blocks);
        bgzf_cut(head.data(), head.size(), spans);
        bgzf_cut(body.host.data(), body.host.size(), spans);
        bgzf_batch(spans, level, threads, comp);
        if (resident) {                                          // the header's blocks as ever; the body's from the stream on the device, which then goes back
            comp.resize(n_blocks);
            body.device->blocks(comp.data() + head_blocks);
            body.device.reset();
        }
    }
    ms_comp = ms_since(t0); t0 = Clock::now();
    // the times of the stages go to stderr and nowhere else
    auto stage_line = [&]() {
        if (!verbose) return;
        char sort_text[64] = "no sort";
        if (body.ms_sort >= 0) std::snprintf(sort_text, sizeof sort_text, "sort %.1f ms (%s)", body.ms_sort, body.route);
        std::fprintf(stderr, "[parasuite-hip] bam: %zu records, %.1f MB in %zu blocks: %s, offsets + gather %.1f ms%s, compression %.1f ms, file write %.1f ms, .bai %.1f ms\n",
                     all.size(), body_bytes / 1e6, n_blocks, sort_text, ms_gather, resident ? " (the stream stayed on the device)" : came_with_sort ? " (the stream came with the sort)" : "", ms_comp, ms_file, ms_bai);
    };
    std::vector<uint64_t> coff(n_blocks + 1, 0);
    for (size_t k = 0; k < n_blocks; ++k) coff[k + 1] = coff[k] + comp[k].size();
    FILE *o = std::fopen(bam_path, "wb");
    if (!o) throw Error(std::string("cannot write ") + bam_path);
    bool ok = true;
    for (size_t k = 0; k < n_blocks && ok; ++k) ok = std::fwrite(comp[k].data(), 1, comp[k].size(), o) == comp[k].size();
    ok = ok && std::fwrite(eof_block, 1, 28, o) == 28;
    ok = (std::fclose(o) == 0) && ok;
    if (!ok) throw Error(std::string("short write on ") + bam_path);
    if (stats) { stats->n_in = d.n_in; stats->n_out = all.size(); stats->bam_bytes = coff[n_blocks] + 28; }
    ms_file = ms_since(t0); t0 = Clock::now();
    if (!write_index) { stage_line(); return; }
    auto voff = [&](uint64_t u) -> uint64_t {           // virtual file offset of body byte u
        if (u == body_bytes && u % BLK == 0) return coff[n_blocks] << 16;      // end of the last full block = start of the EOF block
        return (coff[head_blocks + (size_t)(u / BLK)] << 16) | (u % BLK);
    };
    Layout lay; lay.vbeg.resize(all.size()); lay.vend.resize(all.size());
    for (size_t i = 0; i < all.size(); ++i) { lay.vbeg[i] = voff(uoff[i]); lay.vend[i] = voff(uoff[i + 1]); }
    write_bai(std::string(bam_path) + ".bai", d, lay);
    ms_bai = ms_since(t0);
    stage_line();
}

// The sort in front of write_bam, and the body it leaves.  Each order has a hook of its own (ps_bam.h): the registered one sorts and
// gathers in one go, the host reorders d.recs by its permutation on threads, and the body is the hook's stream -- on the device only
// when the caller said that it may stay there.  Without a hook, or when the hook leaves the call alone: sort_in_order, and the body
// is still in the parts.
std::atomic<BamSortFn> g_sort_device{nullptr}, g_name_sort_device{nullptr};
static BamBody sort_for_write(Data &d, bool by_name, int threads, bool may_stay)
{
    const Clock::time_point t0 = Clock::now();
    BamBody body;
    const BamSortFn fn = by_name ? g_name_sort_device.load() : g_sort_device.load();
    if (fn) {
        std::vector<BgzfSpan> parts(d.enc.size());
        for (size_t k = 0; k < d.enc.size(); ++k) parts[k] = BgzfSpan{d.enc[k].data(), d.enc[k].size()};
        std::vector<uint32_t> perm;
        BamSortJob job{parts.data(), parts.size(), d.recs.data(), d.recs.size(), &perm, &body, may_stay};
        if (fn(job)) {
            if (perm.size() != d.recs.size()) throw Error("internal: the device sort returned no permutation");
            std::vector<Rec> in_order(d.recs.size());
            const int T = threads; const size_t n = d.recs.size();
            par(T, T, [&](int t) { for (size_t i = n * (size_t)t / (size_t)T; i < n * ((size_t)t + 1) / (size_t)T; ++i) { if (perm[i] >= n) throw Error("internal: the device sort returned no permutation"); in_order[i] = d.recs[perm[i]]; } });
            d.recs.swap(in_order);
            body.in_parts = false; body.route = "device";
            body.ms_sort = ms_since(t0);
            return body;
        }
    }
    sort_in_order(d.recs, by_name, [&](const Rec &r) { return rec_name(d, r); });
    body.ms_sort = ms_since(t0);
    return body;
}

}  // namespace

void bam_sort_set_device_hook(BamSortFn fn) { g_sort_device.store(fn); }
void bam_name_sort_set_device_hook(BamSortFn fn) { g_name_sort_device.store(fn); }
int bam_name_cmp(const char *a, const char *b) { return strnum_cmp(a, b); }

// these run once per field of every record of ps_map_to_bam: raw stores into storage grown once per call, no append per byte
static inline void st16(char *d, uint32_t v) { d[0] = (char)(v & 0xff); d[1] = (char)((v >> 8) & 0xff); }
static inline void st32(char *d, uint32_t v) { st16(d, v); st16(d + 2, v >> 16); }
static inline char *grow(std::string &o, size_t n) { const size_t at = o.size(); o.resize(at + n); return &o[at]; }
void bam_rec_begin(std::string &o, const BamCore &c, const char *name, size_t name_len, BamRec &r)
{
    if (name_len > 254) throw Error("read name longer than 254 characters");
    r.ref = c.ref; r.pos = c.pos; r.end = (int32_t)c.end; r.flag = (uint32_t)c.flag; r.off = o.size(); r.len = 0;
    char *d = grow(o, 36 + name_len + 1);
    st32(d, 0);                                             // block_size: bam_rec_end
    st32(d + 4, (uint32_t)c.ref); st32(d + 8, (uint32_t)c.pos);
    d[12] = (char)(uint8_t)(name_len + 1); d[13] = (char)(uint8_t)c.mapq;
    st16(d + 14, (uint32_t)reg2bin(c.pos, c.end));
    st16(d + 16, c.n_cigar); st16(d + 18, (uint32_t)c.flag);
    st32(d + 20, c.l_seq); st32(d + 24, (uint32_t)c.rnext); st32(d + 28, (uint32_t)c.pnext); st32(d + 32, (uint32_t)c.tlen);
    std::memcpy(d + 36, name, name_len); d[36 + name_len] = '\0';
}
void bam_rec_cigar(std::string &o, const uint32_t *words, size_t n) { char *d = grow(o, 4 * n); for (size_t j = 0; j < n; ++j) st32(d + 4 * j, words[j]); }
void bam_tag_int(std::string &o, const char *tag, long long v)
{
    char t[7] = {tag[0], tag[1]}; size_t n;
    if (v < 0) {
        if (v >= -128) { t[2] = 'c'; t[3] = (char)(int8_t)v; n = 4; }
        else if (v >= -32768) { t[2] = 's'; st16(t + 3, (uint32_t)(uint16_t)(int16_t)v); n = 5; }
        else { t[2] = 'i'; st32(t + 3, (uint32_t)(int32_t)v); n = 7; }
    } else if (v <= 255) { t[2] = 'C'; t[3] = (char)(uint8_t)v; n = 4; }
    else if (v <= 65535) { t[2] = 'S'; st16(t + 3, (uint32_t)v); n = 5; }
    else { t[2] = 'I'; st32(t + 3, (uint32_t)v); n = 7; }
    o.append(t, n);
}
void bam_tag_char(std::string &o, const char *tag, char v) { const char t[4] = {tag[0], tag[1], 'A', v}; o.append(t, 4); }
void bam_tag_text_open(std::string &o, const char *tag, char type) { const char t[3] = {tag[0], tag[1], type}; o.append(t, 3); }
void bam_tag_text_close(std::string &o) { o.push_back('\0'); }
void bam_tag_text(std::string &o, const char *tag, char type, const char *v, size_t n)
{
    char *d = grow(o, 3 + n + 1);
    d[0] = tag[0]; d[1] = tag[1]; d[2] = type; std::memcpy(d + 3, v, n); d[3 + n] = '\0';
}
void bam_rec_end(std::string &o, BamRec &r)
{
    r.len = o.size() - r.off;
    st32(&o[r.off], (uint32_t)(r.len - 4));
}

// ---- records straight from memory (ps_map_to_bam)
struct BamSink::Impl {
    Data d; std::string path; bool sort = false, index = false, by_name = false; int threads = 1, level = 6;
    FILE *f = nullptr; uint64_t bytes = 0, n_out = 0; bool failed = false;
    // a sorted sink keeps the buffer as one more part, which its records then name
    void keep_part(std::string &&records, std::vector<BamRec> &recs)
    {
        for (BamRec &r : recs) r.part = (int)d.enc.size();
        d.enc.push_back(std::move(records));
        d.recs.insert(d.recs.end(), recs.begin(), recs.end());
    }
    // an unsorted one compresses the spans side by side and appends the blocks to the file
    void append(const std::vector<BgzfSpan> &spans, int T)
    {
        std::vector<std::string> comp;
        bgzf_batch(spans, level, T, comp);
        for (const std::string &blk : comp) { if (std::fwrite(blk.data(), 1, blk.size(), f) != blk.size()) failed = true; bytes += blk.size(); }
    }
};
BamSink::BamSink(const std::string &header_text, const std::vector<std::pair<std::string, uint32_t>> &refs, const char *bam_path,
                 bool sort_by_coordinate, bool write_index, int threads, int level, bool sort_by_name) : p(new Impl())
{
    if (sort_by_name && (sort_by_coordinate || write_index)) { delete p; p = nullptr; throw Error("a name-sorted BAM is neither coordinate-sorted nor indexed"); }
    if (write_index && !sort_by_coordinate) { delete p; p = nullptr; throw Error("a .bai index needs coordinate-sorted output"); }
    p->d.text = header_text; p->d.refs = refs; p->path = bam_path; p->sort = sort_by_coordinate; p->index = write_index;
    p->threads = clamp_threads(threads); p->level = level < 0 ? 0 : (level > 9 ? 9 : level);
    if (sort_by_name) { p->sort = p->by_name = true; header_sorted(p->d.text, "queryname"); return; }
    if (p->sort) { header_sorted(p->d.text, "coordinate"); return; }
    p->f = std::fopen(bam_path, "wb");
    if (!p->f) { const std::string m = std::string("cannot write ") + bam_path; delete p; p = nullptr; throw Error(m); }
    const std::string head = bam_header(p->d);
    std::vector<BgzfSpan> spans;
    bgzf_cut(head.data(), head.size(), spans);
    try { p->append(spans, 1); } catch (...) { std::fclose(p->f); delete p; p = nullptr; throw; }
}
BamSink::~BamSink() { if (p) { if (p->f) std::fclose(p->f); delete p; } }
// Unsorted: every buffer is cut into its own BGZF blocks (a record may span two blocks, a block never spans two buffers); all blocks
// of the call are compressed side by side.
void BamSink::add(std::vector<std::string> &records, std::vector<std::vector<BamRec>> &recs, uint64_t n_in)
{
    p->d.n_in += n_in;
    if (p->sort) { for (size_t k = 0; k < records.size(); ++k) p->keep_part(std::move(records[k]), recs[k]); return; }
    std::vector<BgzfSpan> spans;
    for (size_t k = 0; k < records.size(); ++k) { p->n_out += recs[k].size(); bgzf_cut(records[k].data(), records[k].size(), spans); }
    p->append(spans, p->threads);
    records.clear(); recs.clear();
}
void BamSink::add(const char *records, size_t n_bytes, std::vector<BamRec> &recs, uint64_t n_in)
{
    p->d.n_in += n_in;
    if (p->sort) p->keep_part(std::string(records, n_bytes), recs);
    else {
        p->n_out += recs.size();
        std::vector<BgzfSpan> spans;
        bgzf_cut(records, n_bytes, spans);
        p->append(spans, p->threads);
    }
    recs.clear();
}
void BamSink::finish(BamStats *stats, BamFile *keep)
{
    if (keep && !p->sort) throw Error("internal: only a sorted BAM is kept in memory");
    if (p->sort) {
        BamBody body = sort_for_write(p->d, p->by_name, p->threads, keep == nullptr);
        if (keep && body.device) throw Error("internal: a kept file needs its records on the host");
        write_bam(p->d, body, p->path.c_str(), p->index, p->threads, stats, p->level);
        if (keep) {                                             // the file's records, in file order, for the step that would read it back: the stream is their one part
            uint64_t at = 0;
            for (Rec &r : p->d.recs) { r.part = 0; r.off = (size_t)at; at += r.len; }
            *keep = BamFile();
            keep->sort_order = p->by_name ? "queryname" : "coordinate";
            keep->text.swap(p->d.text); keep->refs.swap(p->d.refs); keep->recs.swap(p->d.recs);
            keep->enc.assign(1, std::string()); keep->enc[0].swap(body.host);
        }
        return;
    }
    bool ok = !p->failed && std::fwrite(eof_block, 1, 28, p->f) == 28;
    ok = (std::fclose(p->f) == 0) && ok;
    p->f = nullptr;
    if (!ok) throw Error(std::string("short write on ") + p->path);
    if (stats) { stats->n_in = p->d.n_in; stats->n_out = p->n_out; stats->bam_bytes = p->bytes + 28; }
}

void sam_to_bam(const char *sam_path, const char *bam_path, int min_mapq, bool sort_by_coordinate, bool write_index, int threads, BamStats *stats)
{
    threads = clamp_threads(threads);
    if (write_index && !sort_by_coordinate) throw Error("a .bai index needs coordinate-sorted output");
    OutFiles files(".bam-tmp"); const std::string t = add_bam(files, bam_path, write_index);
    files.refuse_inputs({sam_path}, "ps_sam_to_bam: ");
    Data d;
    load_sam(sam_path, min_mapq, threads, d);
    BamBody body;
    if (sort_by_coordinate) { header_sorted(d.text, "coordinate"); body = sort_for_write(d, false, threads, true); }
    write_bam(d, body, t.c_str(), write_index, threads, stats);
    files.publish_all(); files.keep();
}

// `samtools view -q <mapq> -b in.bam -o out.bam`
void bam_view(const char *in_bam, const char *out_bam, int min_mapq, int threads, BamStats *stats)
{
    threads = clamp_threads(threads);
    OutFiles files(".bam-tmp"); const std::string t = files.add(out_bam);
    files.refuse_inputs({in_bam}, "ps_bam_view: ");
    Data d;
    load_bam(in_bam, threads, d, nullptr, nullptr);
    if (min_mapq > 0) {
        std::vector<Rec> keep; keep.reserve(d.recs.size());
        for (const Rec &r : d.recs) if (rec_mapq(d, r) >= min_mapq) keep.push_back(r);
        d.recs.swap(keep);
    }
    BamBody body;
    write_bam(d, body, t.c_str(), false, threads, stats);
    files.publish_all(); files.keep();
}

// `samtools sort [-n] in.bam -o out.bam`
void bam_sort(const char *in_bam, const char *out_bam, bool by_name, int threads, BamStats *stats)
{
    threads = clamp_threads(threads);
    OutFiles files(".bam-tmp"); const std::string t = files.add(out_bam);
    files.refuse_inputs({in_bam}, "ps_bam_sort: ");
    Data d;
    load_bam(in_bam, threads, d, nullptr, nullptr);
    header_sorted(d.text, by_name ? "queryname" : "coordinate");
    BamBody body = sort_for_write(d, by_name, threads, true);
    write_bam(d, body, t.c_str(), false, threads, stats);
    files.publish_all(); files.keep();
}

// `samtools index in.bam`: <in.bam>.bai for a coordinate-sorted file, the file itself is not rewritten
void bam_index(const char *bam, int threads)
{
    threads = clamp_threads(threads);
    OutFiles files(".bam-tmp"); const std::string t = files.add(std::string(bam) + ".bai");
    files.refuse_inputs({bam}, "ps_bam_index: ");
    Data d; Blocks bk; std::vector<uint64_t> rec_u;
    load_bam(bam, threads, d, &bk, &rec_u);
    for (size_t i = 1; i < d.recs.size(); ++i) if (CoordinateLess()(d.recs[i], d.recs[i - 1])) throw Error(std::string("not sorted by coordinate: ") + bam);
    auto voff = [&](uint64_t u) -> uint64_t {           // uncompressed offset -> (compressed block start << 16) | offset inside
        size_t lo = 0, hi = bk.starts.size();
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (bk.starts[mid].second <= u) lo = mid; else hi = mid; }
        // an offset that is exactly a block boundary belongs to the start of the later block (skip empty blocks except the last)
        return (bk.starts[lo].first << 16) | (u - bk.starts[lo].second);
    };
    const uint64_t total = bk.data.size();
    auto voff_end = [&](uint64_t u) -> uint64_t {       // the end of the data is "the last data block, past its last byte"
        if (u < total || u == 0) return voff(u);
        size_t lo = 0, hi = bk.starts.size();
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (bk.starts[mid].second <= u - 1) lo = mid; else hi = mid; }
        return (bk.starts[lo].first << 16) | (u - bk.starts[lo].second);
    };
    Layout lay; lay.vbeg.resize(d.recs.size()); lay.vend.resize(d.recs.size());
    for (size_t i = 0; i < d.recs.size(); ++i) { lay.vbeg[i] = voff(rec_u[i]); lay.vend[i] = voff_end(rec_u[i] + d.recs[i].len); }
    write_bai(t, d, lay);
    files.publish_all(); files.keep();
}

static std::string header_sort_order(const std::string &text)
{
    if (text.compare(0, 3, "@HD") != 0) return std::string();
    const std::string hd = text.substr(0, text.find('\n'));
    const size_t at = hd.find("\tSO:");
    if (at == std::string::npos) return std::string();
    const size_t e = hd.find('\t', at + 1);
    return hd.substr(at + 4, e == std::string::npos ? e : e - at - 4);
}
static void load_any(const char *path, int threads, Data &d)
{
    unsigned char mg[2] = {0, 0};
    { FILE *f = std::fopen(path, "rb"); if (!f) throw Error(std::string("cannot open ") + path); const size_t g = std::fread(mg, 1, 2, f); (void)g; std::fclose(f); }
    if (mg[0] == 31 && mg[1] == 139) load_bam(path, threads, d, nullptr, nullptr); else load_sam(path, -1, threads, d);
}

void load_records(const char *path, int threads, BamFile &out)
{
    threads = clamp_threads(threads);
    Data d;
    load_any(path, threads, d);
    out = BamFile();
    out.sort_order = header_sort_order(d.text);
    out.text.swap(d.text); out.refs.swap(d.refs); out.enc.swap(d.enc); out.recs.swap(d.recs);
}

void scan_records(const char *records, uint64_t n_bytes, std::vector<BamRec> &recs)
{
    recs.clear();
    const uint8_t *b = (const uint8_t *)records;
    uint64_t p = 0;
    while (p < n_bytes) {
        const uint64_t number = recs.size() + 1;
        if (n_bytes - p < 4) throw Error("record " + std::to_string(number) + " runs past the end of the buffer");
        const uint32_t bs = rd32(b + p);
        if (bs < 32) throw Error("record " + std::to_string(number) + " has a block_size of " + std::to_string(bs) + ", below the 32 fixed bytes");
        if ((uint64_t)bs + 4 > n_bytes - p) throw Error("record " + std::to_string(number) + " runs past the end of the buffer");
        Rec r; r.part = 0; r.off = (size_t)p; r.len = 4 + (size_t)bs;
        r.ref = (int32_t)rd32(b + p + 4); r.pos = (int32_t)rd32(b + p + 8); r.end = r.pos < 0x7fffffff ? r.pos + 1 : r.pos; r.flag = rd32(b + p + 16) >> 16;
        recs.push_back(r);
        p += 4 + (uint64_t)bs;
    }
}

static void sort_and_gather(const char *records, std::vector<BamRec> &recs, bool by_name, int threads, char *dst)
{
    sort_in_order(recs, by_name, [&](const Rec &r) { return records + r.off + 36; });
    gather(recs, stream_offsets(recs), clamp_threads(threads), dst, [&](const Rec &) { return records; });
}
void sort_records_host(const char *records, std::vector<BamRec> &recs, int threads, char *dst) { sort_and_gather(records, recs, false, threads, dst); }
void sort_records_host_by_name(const char *records, std::vector<BamRec> &recs, int threads, char *dst) { sort_and_gather(records, recs, true, threads, dst); }

void flatten_records(const BamFile &f, unsigned columns, const std::vector<int32_t> *rows, int threads, RecTable &out)
{
    threads = clamp_threads(threads);
    const bool cig = columns & kRecCigar, sq = columns & kRecSeq, ql = columns & kRecQual, nm = columns & kRecNames;
    const size_t n = rows ? rows->size() : f.n();
    auto row = [&](size_t j) { return rows ? (size_t)(*rows)[j] : j; };
    out = RecTable();
    out.columns = columns; out.refs = f.refs; out.sort_order = f.sort_order;
    out.ref.resize(n); out.pos.resize(n); out.l_seq.resize(n); out.flag.resize(n);
    if (cig) { out.cig_off.resize(n); out.n_cig.resize(n); }
    if (sq || ql) out.seq_off.resize(n);
    if (nm) { out.name_off.resize(n); out.name_len.resize(n); }
    // a record: block_size, 32 fixed bytes (l_read_name at 12, n_cigar_op at 16, l_seq at 20), name with its NUL, CIGAR, SEQ, QUAL, tags
    uint64_t words = 0, bases = 0, name_bytes = 0;
    for (size_t j = 0; j < n; ++j) {
        const BamRec &r = f.recs[row(j)]; const uint8_t *p = f.rec(row(j));
        const uint32_t l_name = p[12], n_cig = p[16] | ((uint32_t)p[17] << 8), l_seq = rd32(p + 20);
        if (r.ref < -1 || r.ref >= (int32_t)f.refs.size()) throw Error("record " + std::to_string(row(j) + 1) + " refers to a reference that is not in the header");
        if (l_name < 1 || 36 + (uint64_t)l_name + 4 * (uint64_t)n_cig + (sq || ql ? ((uint64_t)l_seq + 1) / 2 : 0) + (ql ? (uint64_t)l_seq : 0) > r.len)
            throw Error("corrupt record " + std::to_string(row(j) + 1));
        out.ref[j] = r.ref; out.pos[j] = r.pos; out.flag[j] = r.flag; out.l_seq[j] = (int32_t)l_seq;
        if (cig) { out.n_cig[j] = n_cig; out.cig_off[j] = (uint32_t)words; words += n_cig; }
        if (sq || ql) { out.seq_off[j] = bases; bases += ((uint64_t)l_seq + 1) / 2 * 2; }
        if (nm) { out.name_len[j] = (uint8_t)(l_name - 1); out.name_off[j] = name_bytes; name_bytes += l_name - 1; }
    }
    if (words > 0xffffffffull) throw Error("more than 2^32 CIGAR operations");
    out.cigar.resize((size_t)words); out.names.resize((size_t)name_bytes);
    if (sq) out.seq.assign((size_t)(bases / 2), 0);
    if (ql) out.qual.assign((size_t)bases, 0xff);
    par(threads, threads, [&](int t) {
        for (size_t j = n * (size_t)t / (size_t)threads; j < n * ((size_t)t + 1) / (size_t)threads; ++j) {
            const uint8_t *p = f.rec(row(j)), *cg = p + 36 + p[12], *bs = cg + 4 * (size_t)(p[16] | ((uint32_t)p[17] << 8));
            const size_t l_seq = (size_t)(uint32_t)out.l_seq[j];
            if (nm && out.name_len[j]) std::memcpy(&out.names[(size_t)out.name_off[j]], p + 36, out.name_len[j]);
            if (cig) for (uint32_t c = 0; c < out.n_cig[j]; ++c) out.cigar[out.cig_off[j] + c] = rd32(cg + 4 * c);
            if (sq && l_seq) std::memcpy(&out.seq[(size_t)(out.seq_off[j] / 2)], bs, (l_seq + 1) / 2);
            if (ql && l_seq) std::memcpy(&out.qual[(size_t)out.seq_off[j]], bs + (l_seq + 1) / 2, l_seq);
        }
    });
}

void load_rec_table(const char *path, unsigned columns, int threads, RecTable &out)
{
    BamFile f;
    load_records(path, threads, f);
    flatten_records(f, columns, nullptr, threads, out);
}

// ExtractWeakMappingReads.java:40-94.  The FASTQ text and the list of kept records are complete before either file is written: a
// second copy in memory of every weak read's bases and qualities next to the encoded records; if that ever matters, check the
// error conditions in a first pass over the records and stream the text in a second.  An error leaves nothing behind (§4m).
void extract_weak_reads(const char *path, const char *out_bam, const char *out_fastq, int mapq_threshold, int threads, ExtractStats *stats)
{
    threads = clamp_threads(threads);
    if (!path || !out_bam || !out_fastq || !out_bam[0] || !out_fastq[0]) throw Error("ps_extract_weak_reads: mapping file, output BAM and output FASTQ are required");
    OutFiles files(".extract-tmp"); const std::string t_bam = files.add(out_bam), t_fq = files.add(out_fastq);
    files.refuse_inputs({path}, "ps_extract_weak_reads: ", " may not be the input file ");
    if (same_file(out_bam, out_fastq)) throw Error("ps_extract_weak_reads: the BAM and the FASTQ output are the same file");
    Data d;
    load_any(path, threads, d);
    static const char nt16[] = "=ACMGRSVTWYHKDBN";
    std::string fq; std::vector<Rec> keep; keep.reserve(d.recs.size());
    uint64_t n_weak = 0;
    for (const Rec &r : d.recs) {
        if (rec_mapq(d, r) >= mapq_threshold) { keep.push_back(r); continue; }
        const std::string &e = d.enc[r.part];
        const uint32_t l_name = rd32(e, r.off + 12) & 0xff, n_cig = rd32(e, r.off + 16) & 0xffff, l_seq = rd32(e, r.off + 20);
        const unsigned char *sq = (const unsigned char *)e.data() + r.off + 36 + l_name + 4 * (size_t)n_cig, *ql = sq + (l_seq + 1) / 2;
        const char *name = rec_name(d, r);
        if (l_seq == 0) throw Error(std::string("ps_extract_weak_reads: record ") + name + " has MAPQ below " + std::to_string(mapq_threshold) + " and no SEQ ('*'): it cannot be written as FASTQ");
        if (ql[0] == 0xff) throw Error(std::string("ps_extract_weak_reads: record ") + name + " has MAPQ below " + std::to_string(mapq_threshold) + " and no QUAL ('*'): it cannot be written as FASTQ");
        ++n_weak;
        fq.push_back('@'); fq.append(name); fq.push_back('\n');
        const size_t at = fq.size();
        fq.resize(at + 2 * (size_t)l_seq + 3);
        char *s = &fq[at], *q = s + l_seq + 3;
        s[l_seq] = '\n'; s[l_seq + 1] = '+'; s[l_seq + 2] = '\n';
        const bool rev = (r.flag & 16u) != 0;
        for (uint32_t i = 0; i < l_seq; ++i) {
            char c = nt16[(sq[i >> 1] >> ((~i & 1u) << 2)) & 15];
            if (rev) switch (c) { case 'A': c = 'T'; break; case 'C': c = 'G'; break; case 'G': c = 'C'; break; case 'T': c = 'A'; break; default: break; }
            const uint32_t to = rev ? l_seq - 1 - i : i;
            s[to] = c; q[to] = (char)(ql[i] + 33);
        }
        fq.push_back('\n');
    }
    const uint64_t n_records = d.recs.size();
    d.recs.swap(keep);
    BamStats bs; BamBody body;
    write_bam(d, body, t_bam.c_str(), false, threads, &bs);
    write_text_file(t_fq, fq);
    files.publish_all(); files.keep();
    if (stats) { stats->n_records = n_records; stats->n_weak = n_weak; stats->n_kept = bs.n_out; stats->bam_bytes = bs.bam_bytes; }
}

// ExtractNotMappedReads.java:33-88: "@" + QNAME, one line per record, in file order, whatever the flags
void extract_read_names(const char *path, const char *out_file, int threads, NamesStats *stats)
{
    threads = clamp_threads(threads);
    if (!path || !path[0] || !out_file || !out_file[0]) throw Error("ps_extract_read_names: mapping file and output file are required");
    OutFiles files(".names-tmp"); const std::string t = files.add(out_file);
    files.refuse_inputs({path}, "ps_extract_read_names: ", " may not be the input file ");
    Data d;
    load_any(path, threads, d);
    std::string text;
    for (const Rec &r : d.recs) { text.push_back('@'); text.append(rec_name(d, r)); text.push_back('\n'); }
    write_text_file(t, text);
    files.publish_all(); files.keep();
    if (stats) { stats->n_records = d.recs.size(); stats->out_bytes = text.size(); }
}

}  // namespace ps
