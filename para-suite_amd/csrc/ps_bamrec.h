// ps_bamrec.h -- the BAM record of one located read, stated once for host and device: how large it is and its bytes.
//
// What ps_records.hip's bam_record() makes through ps_bam.cpp's record calls (place, tags_of, put_tags, cal_md, pack_nibbles,
// bam_tag_int), as two functions over one flat input -- no std::string, no table in memory, no recursion: the same code runs as a
// lane of k_bamrec_size / k_bamrec_fill (ps_bamrec.hip) and under g++ alone (tests/bamrec_check.cpp).  No HIP header here.
// The host route stays the oracle of this file; folding it onto this header is a later change.
#pragma once
#include "ps_types.h"

namespace ps {

// the read, its hit as Batch::hit_of assembles it (SelRec, FinRec, optional CIGAR), the reference side
struct RecIn {
    const char *name; uint32_t name_len;         // without NUL; at most 254 (checked on the host before anything is launched)
    const uint8_t *seq;                          // codes 0..4, read orientation
    const char *qual;                            // null: the input had none
    int32_t len;
    int32_t type; int64_t pos;                   // type 0: unmapped; pos on the packed forward strand
    int32_t strand, mapq, n_mm, n_gapo, n_gape, c1, c2;
    const uint32_t *cigar; int32_t n_cigar;      // the library's words (len << 4 | op, MIDS); 0: ungapped
    const uint8_t *pac; int64_t l_pac;
    const int64_t *contig_off; const int32_t *contig_len; int32_t n_contigs;
    const int64_t *hole_off; const int32_t *hole_len; int32_t n_holes;
    int32_t max_top2;
};
// BamRec's key fields, and what the MAPQ filter looks at (unmapped: 0)
struct RecKey { int32_t ref, pos, end; uint32_t flag; int32_t mapq; };

PS_HD int bamrec_reg2bin(int64_t beg, int64_t end)          // UCSC binning scheme (SAMv1 5.3)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
PS_HD int bamrec_pac(const uint8_t *pac, int64_t p) { return (pac[(size_t)p >> 2] >> ((~p & 3) << 1)) & 3; }
PS_HD int bamrec_span(const RecIn &in)
{
    if (!in.n_cigar) return in.len;
    int64_t x = 0;
    for (int j = 0; j < in.n_cigar; ++j) { const int op = (int)(in.cigar[j] & 0xf); if (op == 0 || op == 2) x += in.cigar[j] >> 4; }
    return (int)x;
}
// RefSeq::pos2rid and RefSeq::cnt_ambi over the flat tables
PS_HD int bamrec_contig(const RecIn &in, int64_t pos)
{
    if (pos >= in.l_pac) return -1;
    int left = 0, mid = 0, right = in.n_contigs;
    while (left < right) {
        mid = (left + right) >> 1;
        if (pos >= in.contig_off[mid]) {
            if (mid == in.n_contigs - 1) break;
            if (pos < in.contig_off[mid + 1]) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}
PS_HD int bamrec_holes(const RecIn &in, int64_t pos, int len)
{
    int left = 0, right = in.n_holes;
    while (left < right) {
        const int mid = (left + right) >> 1;
        const int64_t ho = in.hole_off[mid]; const int hl = in.hole_len[mid];
        if (pos >= ho + hl) left = mid + 1;
        else if (pos + len <= ho) right = mid;
        else {
            if (pos >= ho) return ho + hl < pos + len ? (int)(ho + hl - pos) : len;
            return ho + hl < pos + len ? hl : len - (int)(ho - pos);
        }
    }
    return 0;
}

struct RecPlace { int32_t seqid, span, nn, flag, mapq; int64_t pos; bool mapped; };
PS_HD void bamrec_place(const RecIn &in, RecPlace &p)
{
    p.seqid = -1; p.span = 0; p.nn = 0; p.flag = 4; p.mapq = 0; p.pos = -1; p.mapped = false;
    if (in.type == 0) return;
    p.span = bamrec_span(in);
    p.seqid = bamrec_contig(in, in.pos);
    if (p.seqid < 0) p.seqid = 0;                // a position past the text: the host route does not survive it either
    p.nn = bamrec_holes(in, in.pos, p.span);
    p.pos = in.pos - in.contig_off[p.seqid];
    const bool bridges = p.pos + p.span > in.contig_len[p.seqid];
    p.flag = (bridges ? 4 : 0) | (in.strand ? 16 : 0);
    p.mapq = in.mapq;
    p.mapped = true;
}
PS_HD void bamrec_key(const RecIn &in, RecKey &k)
{
    RecPlace p; bamrec_place(in, p);
    k.ref = p.seqid; k.pos = (int32_t)p.pos; k.end = (int32_t)(p.pos + (p.span > 0 ? p.span : 1)); k.flag = (uint32_t)p.flag; k.mapq = p.mapq;
}

// where the bytes go: counted, or written
struct BamrecCount { uint32_t n = 0; PS_HD void put(uint8_t) { ++n; } };
struct BamrecWrite { uint8_t *p; PS_HD void put(uint8_t v) { *p++ = v; } };
struct BamrecNone { PS_HD void put(uint8_t) {} };

template <class S> PS_HD void bamrec_num(S &s, uint32_t v)          // decimal, no buffer
{
    uint32_t d = 1;
    while (v / d >= 10) d *= 10;
    for (; d; d /= 10) s.put((uint8_t)('0' + (v / d) % 10));
}
// the read base at reference-strand position y
PS_HD int bamrec_oriented(const RecIn &in, int y)
{
    if (!in.strand) return in.seq[y];
    const int c = in.seq[in.len - 1 - y];
    return c > 3 ? c : 3 - c;
}
// cal_md: the MD string into s, returns NM
template <class S> PS_HD int bamrec_md(const RecIn &in, S &s)
{
    int64_t x = in.pos; int y = 0, nm = 0; uint32_t u = 0;
    const int n_ops = in.n_cigar ? in.n_cigar : 1;
    for (int k = 0; k < n_ops; ++k) {
        const int l = in.n_cigar ? (int)(in.cigar[k] >> 4) : in.len, op = in.n_cigar ? (int)(in.cigar[k] & 0xf) : 0;
        if (op == 0) {
            for (int z = 0; z < l && x + z < in.l_pac && y + z < in.len; ++z) {
                const int c = bamrec_pac(in.pac, x + z), r = bamrec_oriented(in, y + z);
                if (r > 3 || c != r) { bamrec_num(s, u); s.put((uint8_t)("ACGT"[c])); ++nm; u = 0; } else ++u;
            }
            x += l; y += l;
        } else if (op == 1 || op == 3) { y += l; if (op == 1) nm += l; }
        else if (op == 2) {
            bamrec_num(s, u); s.put((uint8_t)'^');
            for (int z = 0; z < l && x + z < in.l_pac; ++z) s.put((uint8_t)("ACGT"[bamrec_pac(in.pac, x + z)]));
            u = 0; x += l; nm += l;
        }
    }
    bamrec_num(s, u);
    return nm;
}
template <class S> PS_HD void bamrec_tag_int(S &s, char a, char b, long long v)      // bam_tag_int: the smallest type that holds v
{
    s.put((uint8_t)a); s.put((uint8_t)b);
    int n; char t;
    if (v < 0) { if (v >= -128) { t = 'c'; n = 1; } else if (v >= -32768) { t = 's'; n = 2; } else { t = 'i'; n = 4; } }
    else if (v <= 255) { t = 'C'; n = 1; } else if (v <= 65535) { t = 'S'; n = 2; } else { t = 'I'; n = 4; }
    s.put((uint8_t)t);
    const uint32_t w = (uint32_t)(int32_t)v;
    for (int j = 0; j < n; ++j) s.put((uint8_t)(w >> (8 * j)));
}
// the tags of a mapped read in samse's order; nm: what bamrec_md returned
template <class S> PS_HD void bamrec_tags(const RecIn &in, const RecPlace &p, int nm, S &s)
{
    s.put('X'); s.put('T'); s.put('A'); s.put((uint8_t)(p.nn > 10 ? 'N' : "NURM"[in.type & 3]));
    bamrec_tag_int(s, 'N', 'M', nm);
    if (p.nn) bamrec_tag_int(s, 'X', 'N', p.nn);
    bamrec_tag_int(s, 'X', '0', in.c1);
    if (in.c1 <= in.max_top2) bamrec_tag_int(s, 'X', '1', in.c2);
    bamrec_tag_int(s, 'X', 'M', in.n_mm); bamrec_tag_int(s, 'X', 'O', in.n_gapo); bamrec_tag_int(s, 'X', 'G', in.n_gapo + in.n_gape);
    s.put('M'); s.put('D'); s.put('Z');
    bamrec_md(in, s);
    s.put(0);
}

PS_HD uint32_t bamrec_size(const RecIn &in)
{
    RecPlace p; bamrec_place(in, p);
    uint32_t n = 36 + in.name_len + 1 + (p.mapped ? 4u * (uint32_t)(in.n_cigar ? in.n_cigar : 1) : 0u) + ((uint32_t)in.len + 1) / 2 + (uint32_t)in.len;
    if (p.mapped) { BamrecNone none; const int nm = bamrec_md(in, none); BamrecCount c; bamrec_tags(in, p, nm, c); n += c.n; }
    return n;
}
PS_HD void bamrec_put32(uint8_t *d, uint32_t v) { d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24); }
// exactly bamrec_size(in) bytes at dst
PS_HD void bamrec_fill(const RecIn &in, uint8_t *dst)
{
    RecPlace p; bamrec_place(in, p);
    const int len = in.len; const bool rc = in.strand != 0;      // as bam_record(): the strand alone.  An unmapped read has strand 0, a hit whose CIGAR came back empty keeps its strand with type 0 and is written in that orientation
    const uint32_t n_cig = p.mapped ? (uint32_t)(in.n_cigar ? in.n_cigar : 1) : 0u;
    const int64_t end = p.pos + (p.span > 0 ? p.span : 1);
    uint8_t *d = dst;
    bamrec_put32(d + 4, (uint32_t)p.seqid); bamrec_put32(d + 8, (uint32_t)(int32_t)p.pos);
    d[12] = (uint8_t)(in.name_len + 1); d[13] = (uint8_t)p.mapq;
    const uint32_t bin = (uint32_t)bamrec_reg2bin((int32_t)p.pos, end);
    d[14] = (uint8_t)bin; d[15] = (uint8_t)(bin >> 8);
    d[16] = (uint8_t)n_cig; d[17] = (uint8_t)(n_cig >> 8); d[18] = (uint8_t)p.flag; d[19] = (uint8_t)((uint32_t)p.flag >> 8);
    bamrec_put32(d + 20, (uint32_t)len); bamrec_put32(d + 24, 0xffffffffu); bamrec_put32(d + 28, 0xffffffffu); bamrec_put32(d + 32, 0);
    d += 36;
    for (uint32_t i = 0; i < in.name_len; ++i) d[i] = (uint8_t)in.name[i];
    d[in.name_len] = 0;
    d += in.name_len + 1;
    for (uint32_t j = 0; j < n_cig; ++j, d += 4) {
        uint32_t w = (uint32_t)len << 4;
        if (in.n_cigar) { const uint32_t op = in.cigar[j] & 0xfu; w = (in.cigar[j] & ~0xfu) | (op == 3 ? 4u : op); }
        bamrec_put32(d, w);
    }
    for (int i = 0; i < len; i += 2, ++d) {          // pack_nibbles: 1 2 4 8 15, complemented 8 4 2 1 15
        const int a = rc ? in.seq[len - 1 - i] : in.seq[i];
        const int b = i + 1 < len ? (rc ? in.seq[len - 2 - i] : in.seq[i + 1]) : -1;
        const uint32_t hi = a > 3 ? 15u : (rc ? 8u >> a : 1u << a);
        const uint32_t lo = b < 0 ? 0u : (b > 3 ? 15u : (rc ? 8u >> b : 1u << b));
        *d = (uint8_t)(hi << 4 | lo);
    }
    if (!in.qual) for (int i = 0; i < len; ++i) d[i] = 0xff;
    else if (!rc) for (int i = 0; i < len; ++i) d[i] = (uint8_t)(in.qual[i] - 33);
    else for (int i = 0; i < len; ++i) d[i] = (uint8_t)(in.qual[len - 1 - i] - 33);
    d += len;
    if (p.mapped) { BamrecNone none; const int nm = bamrec_md(in, none); BamrecWrite w{d}; bamrec_tags(in, p, nm, w); d = w.p; }
    bamrec_put32(dst, (uint32_t)(d - dst) - 4);
}

}  // namespace ps
