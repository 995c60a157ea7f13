// ps_records.hip -- record output: a located batch as SAM text, BAM records or the error-profile stage's record table.
// Host code only: everything read here is in host memory once batch_locate has run.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <fcntl.h>
#include <unistd.h>
#include "ps_pipeline.h"
#include "ps_par.h"

namespace ps {

// one read's alignment record: from the host-finished subset, else assembled from the device records
void Batch::hit_of(int64_t g, Hit &h) const
{
    if (h_class[g] & PS_CLS_HOST) {
        auto it = std::lower_bound(sub.begin(), sub.end(), g, [](const SubRead &s, int64_t v) { return s.g < v; });
        h = it->hit;
        return;
    }
    const SelRec &s = h_sel[g]; const FinRec &f = h_fin[g];
    h = Hit();
    h.sa = s.sa; h.type = f.type; h.pos = f.type ? f.pos : -1; h.strand = f.strand; h.mapq = f.mapq;
    h.n_mm = s.n_mm; h.n_gapo = s.n_gapo; h.n_gape = s.n_gape; h.ref_shift = s.ref_shift; h.score = s.score; h.c1 = s.c1; h.c2 = s.c2;
    if (s.n_gapo && s.type) {
        auto it = std::lower_bound(dev_cigars.begin(), dev_cigars.end(), g, [](const DevCigar &c, int64_t v) { return c.g < v; });
        if (it != dev_cigars.end() && it->g == g) { h.n_cigar = it->n; std::memcpy(h.cigar, it->c, sizeof h.cigar); }
    }
}

// ------------------------------------------------------------------ SAM -------
static inline int host_pac(const uint8_t *pac, int64_t p) { return (pac[(size_t)p >> 2] >> ((~p & 3) << 1)) & 3; }
static void put_int(std::string &o, long v)            // a dozen numbers per SAM line: no snprintf
{
    char b[24]; int n = 24;
    unsigned long u = v < 0 ? 0ul - (unsigned long)v : (unsigned long)v;
    do { b[--n] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) b[--n] = '-';
    o.append(b + n, (size_t)(24 - n));
}
static int64_t ref_span(int n, const uint32_t *c, int len)
{
    if (!n) return len;
    int64_t x = 0;
    for (int j = 0; j < n; ++j) { int op = c[j] & 0xf; if (op == 0 || op == 2) x += c[j] >> 4; }
    return x;
}
// MD string and edit distance by direct comparison with the reference
static void cal_md(const RefSeq &ref, int n_cigar, const uint32_t *cigar, int len, int64_t pos, const uint8_t *seq, std::string &md, int &nm)
{
    int64_t x = pos, y = 0; int u = 0; nm = 0; md.clear();
    const uint8_t *pac = ref.pac_data();
    auto cmp = [&](int l) {
        for (int z = 0; z < l && x + z < ref.l_pac; ++z) {
            int c = host_pac(pac, x + z);
            if (seq[y + z] > 3 || c != seq[y + z]) { put_int(md, u); md.push_back("ACGTN"[c]); ++nm; u = 0; } else ++u;
        }
    };
    if (n_cigar) {
        for (int k = 0; k < n_cigar; ++k) {
            int l = (int)(cigar[k] >> 4), op = (int)(cigar[k] & 0xf);
            if (op == 0) { cmp(l); x += l; y += l; }
            else if (op == 1 || op == 3) { y += l; if (op == 1) nm += l; }
            else if (op == 2) {
                put_int(md, u); md.push_back('^');
                for (int z = 0; z < l && x + z < ref.l_pac; ++z) md.push_back("ACGT"[host_pac(pac, x + z)]);
                u = 0; x += l; nm += l;
            }
        }
    } else cmp(len);
    put_int(md, u);
}

// SAM text goes through a raw cursor into storage the caller has made large enough (Room): a line is ~35 small pieces, and one
// std::string append per piece was most of the 1.3 us per read and thread that the writer -- the last stage of ps_map -- spent.
namespace {
struct Cur {
    char *p;
    inline void ch(char c) { *p++ = c; }
    inline void mem(const char *s, size_t n) { std::memcpy(p, s, n); p += n; }
    template <size_t N> inline void lit(const char (&s)[N]) { std::memcpy(p, s, N - 1); p += N - 1; }
    inline void num(long v)
    {
        static const char D2[] = "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
        unsigned long u = (unsigned long)v;
        if (v < 0) { *p++ = '-'; u = 0ul - u; }
        if (u < 10) { *p++ = (char)('0' + u); return; }
        if (u < 100) { std::memcpy(p, D2 + 2 * u, 2); p += 2; return; }
        char b[24]; int n = 24;
        while (u >= 100) { const unsigned long r = u % 100; u /= 100; n -= 2; std::memcpy(b + n, D2 + 2 * r, 2); }
        if (u >= 10) { n -= 2; std::memcpy(b + n, D2 + 2 * u, 2); } else b[--n] = (char)('0' + u);
        std::memcpy(p, b + n, (size_t)(24 - n)); p += 24 - n;
    }
    inline void cigar(int n, const uint32_t *c, int len)
    {
        if (n) for (int j = 0; j < n; ++j) { num((long)(c[j] >> 4)); ch("MIDS"[c[j] & 0xf]); }
        else { num(len); ch('M'); }
    }
};
// storage with `used` bytes taken: at least `need` more, the string's size being the storage (grown in large steps, never shrunk here)
inline char *room(std::string &o, size_t used, size_t need)
{
    if (o.size() < used + need) o.resize(std::max(o.size() + o.size() / 2, used + need + ((size_t)1 << 16)));
    return &o[0] + used;
}
}
// the XA list of a read (alternative hits, `samse -n 3`): chr,(+|-)pos,CIGAR,NM;
static void xa_cur(const Batch &b, const Hit &h, int len, std::string &o, size_t &used)
{
    const RefSeq &ref = b.ctx->ix.ref;
    for (int j = 0; j < h.n_multi; ++j) {
        const Multi &m = b.multis[h.multi_begin + j];
        int sid = 0;
        ref.cnt_ambi(m.pos, (int)ref_span(m.n_cigar, m.cigar, len), &sid);
        const Contig &mc = ref.contigs[sid];
        Cur c{room(o, used, mc.name.size() + 64 + 12 * (size_t)PS_MAX_CIGAR)};
        char *const c0 = c.p;
        c.mem(mc.name.data(), mc.name.size()); c.ch(','); c.ch(m.strand ? '-' : '+'); c.num((long)(m.pos - mc.offset + 1)); c.ch(',');
        c.cigar(m.n_cigar, m.cigar, len);
        c.ch(','); c.num(m.gap + m.mm); c.ch(';');
        used += (size_t)(c.p - c0);
    }
}
static void xa_text(const Batch &b, const Hit &h, int len, std::string &o)        // appended to a string (the BAM route)
{
    size_t used = o.size();
    xa_cur(b, h, len, o, used);
    o.resize(used);
}
// ---- one located read as an output record.  Every route -- SAM text, BAM record, profile table -- takes what a hit IS from here.
namespace {
struct Placed {
    Hit h; int len; const uint8_t *seq; const char *qual, *name; size_t name_len;      // qual null: the input had none
    const Contig *ct;                                      // null: unmapped
    int seqid, span, nn, flag, mapq;                       // unmapped: seqid -1, flag 4, and MAPQ 0 for every filter
    int64_t pos;                                           // 0-based on the contig; unmapped -1
    bool bridges;                                          // runs over the end of its contig: flag 4, position kept
    bool mapped() const { return ct != nullptr; }
};
inline void place(const Batch &b, int64_t g, Placed &p)
{
    const ReadSet &rs = b.rs; const RefSeq &ref = b.ctx->ix.ref;
    b.hit_of(g, p.h);
    const Hit &h = p.h;
    p.len = rs.len[g];
    p.seq = rs.seq.data() + rs.off[g];
    p.qual = rs.has_qual ? rs.qual.data() + rs.off[g] : nullptr;
    p.name = rs.name(g, p.name_len);
    p.ct = nullptr; p.seqid = -1; p.span = 0; p.nn = 0; p.flag = 4; p.mapq = 0; p.pos = -1; p.bridges = false;
    if (h.type == 0) return;
    p.span = (int)ref_span(h.n_cigar, h.cigar, p.len);
    p.nn = ref.cnt_ambi(h.pos, p.span, &p.seqid);
    p.ct = &ref.contigs[p.seqid];
    p.pos = h.pos - p.ct->offset;
    p.bridges = p.pos + p.span > p.ct->len;
    p.flag = (p.bridges ? 4 : 0) | (h.strand ? 16 : 0);
    p.mapq = h.mapq;
}
// what the tags of a mapped read need beyond its place: MD and NM from the read as the reference strand shows it
struct Tags { const std::string *md; int nm; char xt; };
inline void tags_of(const Batch &b, const Placed &p, Tags &t)
{
    static thread_local std::string md;
    const Hit &h = p.h; const int len = p.len;
    uint8_t tmp_small[256]; std::vector<uint8_t> tmp_big;
    uint8_t *tmp = tmp_small;
    if (len > 256) { tmp_big.resize((size_t)len); tmp = tmp_big.data(); }
    const uint8_t *oriented = p.seq;
    if (h.strand) { for (int i = 0; i < len; ++i) { uint8_t c = p.seq[len - 1 - i]; tmp[i] = c > 3 ? c : (uint8_t)(3 - c); } oriented = tmp; }
    cal_md(b.ctx->ix.ref, h.n_cigar, h.cigar, len, h.pos, oriented, md, t.nm);
    t.md = &md;
    t.xt = p.nn > 10 ? 'N' : "NURM"[h.type];
}
// the tags of a mapped read in the order samse prints them.  A sink takes the tag's name and its SAM prefix, both literals
#define PS_TAG(name, type) name, "\t" name ":" type ":"
template <class Sink> inline void put_tags(const Batch &b, const Placed &p, const Tags &t, Sink &s)
{
    const Hit &h = p.h;
    s.chr(PS_TAG("XT", "A"), t.xt); s.num(PS_TAG("NM", "i"), t.nm);
    if (p.nn) s.num(PS_TAG("XN", "i"), p.nn);
    s.num(PS_TAG("X0", "i"), h.c1);
    if (h.c1 <= b.ctx->opt.max_top2) s.num(PS_TAG("X1", "i"), h.c2);
    s.num(PS_TAG("XM", "i"), h.n_mm); s.num(PS_TAG("XO", "i"), h.n_gapo); s.num(PS_TAG("XG", "i"), h.n_gapo + h.n_gape);
    s.text(PS_TAG("MD", "Z"), t.md->data(), t.md->size());
    if (h.n_multi) s.xa(PS_TAG("XA", "Z"), b, p);
}
#undef PS_TAG
// CIGAR as BAM words (soft clip is 4 there, 3 here; an ungapped hit has no words of its own: <len>M)
inline int cigar_words(const Hit &h) { return h.n_cigar ? h.n_cigar : 1; }
inline int bam_cigar(const Hit &h, int len, uint32_t *out)
{
    for (int j = 0; j < h.n_cigar; ++j) { const uint32_t op = h.cigar[j] & 0xfu; out[j] = (h.cigar[j] & ~0xfu) | (op == 3 ? 4u : op); }
    if (!h.n_cigar) out[0] = (uint32_t)len << 4;
    return cigar_words(h);
}
// bases as BAM nibbles, two to a byte, in the record's orientation: (len + 1) / 2 bytes at d
inline void pack_nibbles(const uint8_t *seq, int len, bool rc, uint8_t *d)
{
    static const uint8_t NIB[5] = {1, 2, 4, 8, 15}, NIB_RC[5] = {8, 4, 2, 1, 15};
    for (int i = 0; i < len; i += 2) {
        const uint8_t hi = rc ? NIB_RC[seq[len - 1 - i]] : NIB[seq[i]];
        const uint8_t lo = i + 1 < len ? (rc ? NIB_RC[seq[len - 2 - i]] : NIB[seq[i + 1]]) : 0;
        d[i >> 1] = (uint8_t)(hi << 4 | lo);
    }
}
// per-read loops over [.., g1): the reference bases of a read further on (MD tag) are a cache miss each
inline void prefetch_ref(const Batch &b, const uint8_t *pac, int64_t g, int64_t g1)
{
    if (g + 8 < g1 && !(b.h_class[g + 8] & PS_CLS_HOST) && b.h_fin[g + 8].type) __builtin_prefetch(pac + ((size_t)b.h_fin[g + 8].pos >> 2));
}

struct SamTags {                // tags as text behind the cursor; the XA list makes its own room, the cursor then moves behind it
    std::string &o; size_t &used; Cur c; char *c0;
    template <size_t N> inline void chr(const char *, const char (&pre)[N], char v) { c.lit(pre); c.ch(v); }
    template <size_t N> inline void num(const char *, const char (&pre)[N], long v) { c.lit(pre); c.num(v); }
    template <size_t N> inline void text(const char *, const char (&pre)[N], const char *v, size_t n) { c.lit(pre); c.mem(v, n); }
    template <size_t N> inline void xa(const char *, const char (&pre)[N], const Batch &b, const Placed &p)
    { c.lit(pre); used += (size_t)(c.p - c0); xa_cur(b, p.h, p.len, o, used); c.p = c0 = room(o, used, 1); }
};
struct BamTags {
    std::string &o;
    void chr(const char *tag, const char *, char v) { bam_tag_char(o, tag, v); }
    void num(const char *tag, const char *, long v) { bam_tag_int(o, tag, v); }
    void text(const char *tag, const char *, const char *v, size_t n) { bam_tag_text(o, tag, 'Z', v, n); }
    void xa(const char *tag, const char *, const Batch &b, const Placed &p) { bam_tag_text_open(o, tag, 'Z'); xa_text(b, p.h, p.len, o); bam_tag_text_close(o); }
};
}

// one line at o[used...]; `used` moves on.  o.size() is storage, not content (room()).
static void sam_line(const Batch &b, int64_t g, std::string &o, size_t &used)
{
    Placed p; place(b, g, p);
    Tags t{nullptr, 0, 0};
    if (p.mapped()) tags_of(b, p, t);
    const int len = p.len;
    // everything but the XA list: name, 11 columns (two of them the read), at most 9 tags of <= 26 characters, MD
    char *const c0 = room(o, used, p.name_len + 2 * (size_t)len + (p.ct ? p.ct->name.size() + t.md->size() : 0) + 12 * (size_t)PS_MAX_CIGAR + 384);
    SamTags s{o, used, Cur{c0}, c0};
    Cur &c = s.c;
    c.mem(p.name, p.name_len);
    auto put_seq = [&]() {
        const uint8_t *seq = p.seq; const char *qual = p.qual; const int strand = p.h.strand;
        char *d = c.p;
        if (!strand) for (int i = 0; i < len; ++i) d[i] = "ACGTN"[seq[i]];
        else for (int i = 0; i < len; ++i) d[i] = "TGCAN"[seq[len - 1 - i]];
        d[len] = '\t';
        d += len + 1;
        if (qual) { if (!strand) std::memcpy(d, qual, (size_t)len); else for (int i = 0; i < len; ++i) d[i] = qual[len - 1 - i]; d += len; }
        else *d++ = '*';
        c.p = d;
    };
    if (!p.mapped()) c.lit("\t4\t*\t0\t0\t*\t*\t0\t0\t");
    else {
        c.ch('\t'); c.num(p.flag); c.ch('\t'); c.mem(p.ct->name.data(), p.ct->name.size()); c.ch('\t');
        c.num((long)(p.pos + 1)); c.ch('\t'); c.num(p.mapq); c.ch('\t');
        c.cigar(p.h.n_cigar, p.h.cigar, len);
        c.lit("\t*\t0\t0\t");
    }
    put_seq();
    if (p.mapped()) put_tags(b, p, t, s);
    c.ch('\n');
    used += (size_t)(c.p - s.c0);
}

// the same record as a BAM record (ps_map_to_bam: no SAM text in between); false: below the MAPQ filter (not stored)
static bool bam_record(const Batch &b, int64_t g, int min_mapq, std::string &o, BamRec &r)
{
    Placed p; place(b, g, p);
    if (p.mapq < min_mapq) return false;
    const int len = p.len; const bool rc = p.h.strand != 0;
    uint32_t cig[PS_HIT_CIGAR];
    static_assert(sizeof cig == sizeof p.h.cigar, "bam_cigar writes up to as many words as a Hit holds");
    const int n_cig = p.mapped() ? bam_cigar(p.h, len, cig) : 0;
    bam_rec_begin(o, BamCore{p.seqid, (int32_t)p.pos, p.pos + (p.span > 0 ? p.span : 1), p.mapq, p.flag, (uint32_t)n_cig, (uint32_t)len}, p.name, p.name_len, r);
    bam_rec_cigar(o, cig, (size_t)n_cig);
    const size_t at = o.size(), nb = (size_t)(len + 1) / 2;
    o.resize(at + nb + (size_t)len);
    uint8_t *d = reinterpret_cast<uint8_t *>(&o[at]);
    pack_nibbles(p.seq, len, rc, d);
    d += nb;
    if (!p.qual) std::memset(d, 0xff, (size_t)len);
    else if (!rc) for (int i = 0; i < len; ++i) d[i] = (uint8_t)(p.qual[i] - 33);
    else for (int i = 0; i < len; ++i) d[i] = (uint8_t)(p.qual[len - 1 - i] - 33);
    if (p.mapped()) { Tags t; tags_of(b, p, t); BamTags s{o}; put_tags(b, p, t, s); }
    bam_rec_end(o, r);
    return true;
}
// the records of a located batch that pass the MAPQ filter as BAM records: one buffer per host thread, the buffers in input order
void batch_bam_records(const Batch &b, int min_mapq, int threads, std::vector<std::string> &enc, std::vector<std::vector<BamRec>> &recs)
{
    if (!b.located) throw Error("BAM records before locate");
    const size_t N = (size_t)b.rs.n;
    const int nt = par_threads(N, threads);
    enc.assign((size_t)nt, std::string()); recs.assign((size_t)nt, std::vector<BamRec>());
    const auto t0 = std::chrono::steady_clock::now();
    par_for(N, threads, [&](size_t g0, size_t g1, int t) {
        std::string &o = enc[t]; o.reserve((g1 - g0) * 176);
        const uint8_t *pac = b.ctx->ix.ref.pac_data();
        for (size_t g = g0; g < g1; ++g) {
            prefetch_ref(b, pac, (int64_t)g, (int64_t)g1);
            BamRec r; r.part = 0; if (bam_record(b, (int64_t)g, min_mapq, o, r)) recs[t].push_back(r);
        }
    });
    static const bool verbose = std::getenv("PS_VERBOSE") != nullptr && std::atoi(std::getenv("PS_VERBOSE")) >= 2;
    if (verbose) std::fprintf(stderr, "[parasuite-hip]     BAM records of %lld reads: building on %d threads %.0f ms\n", (long long)N, nt,
                              1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}
// the host-finished reads alone, for the device route (ps_bamrec.hip) to splice into its stream: the same bam_record()
void batch_bam_records_sub(const Batch &b, int min_mapq, int threads, std::vector<std::string> &enc, std::vector<BamRec> &recs)
{
    if (!b.located) throw Error("BAM records before locate");
    const size_t M = b.sub.size();
    const int nt = par_threads(M, threads);
    enc.assign((size_t)nt, std::string()); recs.assign(M, BamRec{-1, -1, 0, 4, 0, 0, 0});
    par_for(M, threads, [&](size_t i0, size_t i1, int t) {
        std::string &o = enc[t]; o.reserve((i1 - i0) * 256);
        for (size_t i = i0; i < i1; ++i) {
            BamRec r; r.part = t; r.len = 0;
            if (bam_record(b, b.sub[i].g, min_mapq, o, r)) recs[i] = r; else recs[i].part = t;
        }
    });
}

void batch_profile_records(const Batch &b, int min_mapq, int threads, ProfRecords &out)
{
    if (!b.located) throw Error("profile records before locate");
    const size_t N = (size_t)b.rs.n;
    const int nt = par_threads(N, threads);
    // pass 1: which reads are in the filtered file as placed records (a bridging one carries flag 4 there), and how much they hold
    std::vector<uint8_t> keep(N, 0);
    std::vector<size_t> t_rec(nt + 1, 0), t_cig(nt + 1, 0), t_base(nt + 1, 0);
    par_for(N, threads, [&](size_t g0, size_t g1, int t) {
        size_t nr = 0, nc = 0, nb = 0;
        for (size_t g = g0; g < g1; ++g) {
            Placed p; place(b, (int64_t)g, p);
            if (!p.mapped() || p.mapq < min_mapq || p.bridges) continue;
            keep[g] = 1; ++nr; nc += (size_t)cigar_words(p.h); nb += (size_t)p.len + ((size_t)p.len & 1);
        }
        t_rec[t] = nr; t_cig[t] = nc; t_base[t] = nb;
    });
    out.columns = kRecCigar | kRecSeq;
    size_t r0 = out.n(), c0 = out.cigar.size(), b0 = out.seq.size() * 2;     // every record starts on a whole byte
    std::vector<size_t> br(nt + 1), bc(nt + 1), bb(nt + 1);
    br[0] = r0; bc[0] = c0; bb[0] = b0;
    for (int t = 0; t < nt; ++t) { br[t + 1] = br[t] + t_rec[t]; bc[t + 1] = bc[t] + t_cig[t]; bb[t + 1] = bb[t] + t_base[t]; }
    out.gpos.resize(br[nt]); out.l_seq.resize(br[nt]); out.flag.resize(br[nt]); out.cig_off.resize(br[nt]); out.n_cig.resize(br[nt]); out.seq_off.resize(br[nt]);
    out.cigar.resize(bc[nt]); out.seq.resize(bb[nt] / 2);
    // pass 2: fill, every thread its own range
    par_for(N, threads, [&](size_t g0, size_t g1, int t) {          // the same ranges as in pass 1
        size_t r = br[t], c = bc[t], bs = bb[t];
        for (size_t g = g0; g < g1; ++g) {
            if (!keep[g]) continue;
            Placed p; place(b, (int64_t)g, p);          // a second look-up of the contig (cnt_ambi) for the kept reads: the price of one resolver
            out.gpos[r] = p.h.pos; out.l_seq[r] = p.len; out.flag[r] = (uint32_t)p.flag;
            out.cig_off[r] = (uint32_t)c; out.seq_off[r] = (uint64_t)bs;
            out.n_cig[r] = (uint32_t)bam_cigar(p.h, p.len, &out.cigar[c]); c += out.n_cig[r];
            pack_nibbles(p.seq, p.len, p.h.strand != 0, out.seq.data() + bs / 2);
            bs += (size_t)p.len + ((size_t)p.len & 1);
            ++r;
        }
    });
}

// @SQ per reference sequence in FASTA order, then our @PG: what upstream's samse prints before the first record -- also when
// there is no record at all (bwa_print_sam_SQ runs before the read loop)
std::string sam_header(const RefSeq &ref, const char *pg_line)
{
    std::string h;
    for (const Contig &c : ref.contigs) { h += "@SQ\tSN:"; h += c.name; h += "\tLN:"; put_int(h, c.len); h.push_back('\n'); }
    if (pg_line && pg_line[0]) { h += pg_line; h += "\n"; }
    return h;
}

void batch_write_sam(Batch &b, const char *path, bool header, const char *pg_line, int threads, bool append, SamScratch *scratch)
{
    if (!b.located) throw Error("write_sam before locate");
    const int fd = ::open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0644);
    if (fd < 0) throw Error(std::string("cannot write ") + path);
    struct Closer { int fd; bool done = false; ~Closer() { if (!done) ::close(fd); } } closer{fd};
    off_t at = append ? ::lseek(fd, 0, SEEK_END) : 0;
    if (at < 0) throw Error(std::string("cannot seek in ") + path);
    auto put = [&](const char *p, size_t n, off_t where) {           // the whole buffer at its place in the file
        while (n) { const ssize_t w = ::pwrite(fd, p, n, where); if (w <= 0) return false; p += w; n -= (size_t)w; where += w; }
        return true;
    };
    if (header) {
        const std::string h = sam_header(b.ctx->ix.ref, pg_line);
        if (!put(h.data(), h.size(), at)) throw Error(std::string("short write on ") + path);
        at += (off_t)h.size();
    }
    const int64_t N = b.rs.n;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    // rounds of threads x 64k reads: every thread formats its range; the text of a round is then written -- each buffer at its
    // own offset (pwrite), by a few I/O threads side by side -- while the next round is formatted.  (One writer thread managed
    // ~1 GB/s and was the slowest stage of ps_map at 2 GB of SAM per 10 M reads.)
    const int64_t chunk = 1 << 16;
    SamScratch own;
    std::vector<std::string> *bufs = scratch ? scratch->bufs : own.bufs;
    for (int k = 0; k < 2; ++k) if (bufs[k].size() < (size_t)threads) bufs[k].resize((size_t)threads);
    std::vector<off_t> where[2] = {std::vector<off_t>((size_t)threads, 0), std::vector<off_t>((size_t)threads, 0)};
    std::vector<size_t> lens[2] = {std::vector<size_t>((size_t)threads, 0), std::vector<size_t>((size_t)threads, 0)};
    std::thread io; std::atomic<bool> io_ok{true};
    const int n_io = std::max(1, std::min(8, threads));
    int which = 0;
    static const bool verbose = std::getenv("PS_VERBOSE") != nullptr && std::atoi(std::getenv("PS_VERBOSE")) >= 2;
    double t_fmt = 0, t_wait = 0; const auto tw0 = std::chrono::steady_clock::now();
    for (int64_t base = 0; base < N; base += chunk * threads, which ^= 1) {
        const auto tf0 = std::chrono::steady_clock::now();
        std::vector<std::string> &out = bufs[which];          // the I/O threads may still hold the other set
        std::vector<size_t> &used = lens[which];
        auto fmt = [&](int t) {
            int64_t g0 = base + chunk * t, g1 = std::min(N, g0 + chunk);
            std::string &o = out[t];                           // storage: its size is what it can hold, used[t] what it does hold
            size_t u = 0;
            if (g0 < g1) room(o, 0, (size_t)(g1 - g0) * 224);
            const uint8_t *pac = b.ctx->ix.ref.pac_data();
            for (int64_t g = g0; g < g1; ++g) {
                prefetch_ref(b, pac, g, g1);
                sam_line(b, g, o, u);
            }
            used[t] = u;
        };
        { std::vector<std::thread> th; for (int t = 1; t < threads; ++t) th.emplace_back(fmt, t); fmt(0); for (auto &x : th) x.join(); }
        const auto tf1 = std::chrono::steady_clock::now();
        if (io.joinable()) io.join();
        t_fmt += std::chrono::duration<double>(tf1 - tf0).count(); t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - tf1).count();
        if (!io_ok) break;
        std::vector<off_t> &wh = where[which];
        for (int t = 0; t < threads; ++t) { wh[t] = at; at += (off_t)used[t]; }
        io = std::thread([&out, &wh, &used, &put, &io_ok, n_io, threads]() {
            auto part = [&](int k) { for (int t = k; t < threads; t += n_io) if (used[t] && !put(out[t].data(), used[t], wh[t])) io_ok = false; };
            std::vector<std::thread> th; for (int k = 1; k < n_io; ++k) th.emplace_back(part, k); part(0); for (auto &x : th) x.join();
        });
    }
    const auto tl0 = std::chrono::steady_clock::now();
    if (io.joinable()) io.join();
    if (verbose) std::fprintf(stderr, "[parasuite-hip]     SAM text of %lld reads: %.0f ms (formatting on %d threads %.0f ms, waiting for the previous round's pwrite %.0f ms, last round's pwrite %.0f ms), %.0f MB\n", (long long)N,
                              1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count(), threads, 1e3 * t_fmt, 1e3 * t_wait, 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count(), at / 1048576.0);
    if (!io_ok) throw Error(std::string("short write on ") + path);
    closer.done = true;
    if (::close(fd) != 0) throw Error(std::string("cannot close ") + path);
}

}  // namespace ps
