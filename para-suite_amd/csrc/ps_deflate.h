// ps_deflate.h -- one BGZF block (at most 0xff00 input bytes) as one raw DEFLATE stream (RFC 1951) with its CRC32, written once
// for the device and for the host compiler (the pattern of ps_narrow.h / tests/hostsim).
//
// One block is the work of DF_NL = 64 lanes that share a DfShared (LDS on the device).  The algorithm is a sequence of REGIONS
// (DF_LANES) separated by DF_SYNC.  On the device a region runs once per lane and DF_SYNC is the workgroup barrier; the host
// build runs the lanes of a region one after the other.  Both give the same bytes because every region keeps to one rule: a lane
// writes only slots of its own or adds to shared words with commutative atomics whose result it does not use (max, add, or), and
// no lane reads in a region what another lane writes in that region.  The output is therefore a pure function of the input bytes:
// no dependence on which lane wins a race, on scheduling or on the launch shape.
//
// THE MATCH CANDIDATE.  Positions are taken in chunks of 64.  h(i) is a 13-bit multiplicative hash of the 4 bytes at i (positions
// with fewer than 4 bytes left have none).  The candidate of position i is the largest j below the start of i's chunk with
// h(j) == h(i): the table keeps one entry per hash, every position of a chunk is inserted with an atomic max after the whole
// chunk has looked its candidates up.  A candidate further back than 32768 is not used and no second one is looked for.  The
// match length is the common prefix of i and j, at most 258 and never past the block's end; below 4 it is no match.
//
// TOKENS.  Greedy: a token starts at 0; a token at i is the match of i if it has one, else the literal, and the next token starts
// at i + max(1, len[i]).  The chain is resolved per chunk by pointer doubling over the 64 positions (six rounds), the position
// where the chain enters the next chunk is carried.  Chunks that a match covers whole only insert their hashes.  Tokens go to
// global scratch (4 bytes each, at most n), the histograms of the 286 literal/length and 30 distance symbols to shared memory.
//
// ENCODINGS.  Stored, fixed Huffman and dynamic Huffman are priced exactly; the smallest in bytes is taken (on a tie stored, then
// fixed).  Dynamic: plain Huffman from the histograms (rank sort on all lanes, two-queue merge on one), depths limited to 15 by
// moving leaves until the Kraft sum is exactly one, least frequent symbols longest; the code-length alphabet with 16/17/18 runs
// over the joined length sequence, limited to 7 the same way; HLIT, HDIST and HCLEN trimmed.  A tree with no used symbol gets two
// codes of one bit (symbols 0 and 1), one used symbol gets one bit beside symbol 0 or 1: complete codes, as zlib writes them.
// The choice is made from the counts before anything is emitted, so a block never takes more than n + 5 bytes.
//
// EMISSION.  Tokens in groups of 64: each lane prices its token, an exclusive sum gives its bit offset, the lanes OR their bits
// into a window of shared words, whole words go to the output and the partial last word is carried into the next group.
//
// CRC32.  Each lane takes a slice of the input with the byte table in shared memory; the slices are combined with the operators
// x^(8 len) mod P (the crc32_combine construction).
#pragma once
#include <stdint.h>
#include <string.h>

namespace ps {

enum { DF_NL = 64, DF_HBITS = 13, DF_HSIZE = 1 << DF_HBITS, DF_MIN_MATCH = 4, DF_MAX_MATCH = 258, DF_MAX_DIST = 32768, DF_BLOCK = 0xff00,
       DF_STORED = 1, DF_FIXED = 2, DF_DYNAMIC = 4, DF_ALL = 7,
       DF_OUT_STRIDE = DF_BLOCK + 16 };                 // room for one block's output: n + 5 bytes rounded up to whole words

#ifdef PS_DF_DEVICE
#define DF_FN static __device__
#define DF_LANES(l) for (int l = (int)threadIdx.x, df_once_ = 0; df_once_ == 0; ++df_once_)
#define DF_SYNC() __syncthreads()
#define DF_ATOMIC_MAX(p, v) ((void)atomicMax((p), (v)))
#define DF_ATOMIC_ADD(p, v) ((void)atomicAdd((p), (v)))
#define DF_ATOMIC_OR(p, v) ((void)atomicOr((p), (v)))
#else
#define DF_FN static inline
#define DF_LANES(l) for (int l = 0; l < DF_NL; ++l)
#define DF_SYNC() ((void)0)
#define DF_ATOMIC_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define DF_ATOMIC_ADD(p, v) (*(p) += (v))
#define DF_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

// size of the DEFLATE stream, CRC32 of the input, BTYPE taken (0, 1, 2); depth: the deepest leaf of the plain Huffman trees before
// the limit (literal/length, distance, code lengths) -- what a test needs to know that its input reached the limit
struct DfResult { uint32_t bytes, crc, btype; uint16_t depth[3]; uint16_t pad_; };

struct DfShared {
    uint32_t htab[DF_HSIZE];                            // hash -> position + 1 (0: none)
    uint32_t fl[288], fd[32], fc[20];                   // histograms: literal/length, distance, code-length alphabet
    uint32_t crc_tab[256], crc_part[DF_NL];
    uint32_t wint[288];                                 // tree building: weights of the internal nodes
    uint16_t sorted[288], parent[576], depth[576];
    uint16_t lcode[288], dcode[32], ccode[20];          // codes, bit-reversed
    uint8_t llen[288], dlen[32], clen[20];
    uint8_t lens[320]; uint16_t rle[320];               // the joined length sequence and its run-length form (symbol | extra << 8)
    uint32_t hdr[160];                                  // block header bits (at most 17 + 57 + 316 * 14)
    uint32_t win[104];                                  // emission window of one group: 31 carried bits + 64 * 48
    uint64_t cm[2][DF_NL + 1]; uint8_t cj[2][DF_NL + 1];   // chain doubling: reach mask and jump, slot 64 = beyond the chunk
    uint16_t adv[DF_NL], mdist[DF_NL], nb[DF_NL], max_depth[4];
    uint32_t ntok, carry_pos, extra_bits, n_match, nused, nrle, hlit, hdist, hclen, hdr_bits, btype, out_bytes, gbits, gnext, carry;
};

DF_FN uint32_t df_ld32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
DF_FN uint64_t df_ld64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
DF_FN uint32_t df_hash(uint32_t v) { return (v * 2654435761u) >> (32 - DF_HBITS); }
DF_FN int df_popc64(uint64_t v) { return __builtin_popcountll(v); }
DF_FN int df_log2(uint32_t v) { return 31 - __builtin_clz(v); }      // v > 0

// common prefix of a and b, at most maxl (both have maxl bytes)
DF_FN int df_match_len(const uint8_t *a, const uint8_t *b, int maxl)
{
    int k = 0;
    while (k + 8 <= maxl) {
        const uint64_t x = df_ld64(a + k) ^ df_ld64(b + k);
        if (x) return k + (__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < maxl && a[k] == b[k]) ++k;
    return k;
}

// length 3..258 -> symbol 257..285, extra bits and their value; distance 1..32768 -> symbol 0..29 (RFC 1951 3.2.5, in closed form)
DF_FN void df_len_sym(int len, int &sym, int &eb, int &ev)
{
    const int l = len - 3;
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
    if (len == 258) { sym = 285; eb = 0; ev = 0; return; }
    eb = df_log2((uint32_t)l) - 2;
    sym = 261 + 4 * eb + ((l >> eb) & 3);
    ev = l & ((1 << eb) - 1);
}
DF_FN void df_dist_sym(int dist, int &sym, int &eb, int &ev)
{
    const int d = dist - 1;
    if (d < 4) { sym = d; eb = 0; ev = 0; return; }
    const int lg = df_log2((uint32_t)d);
    eb = lg - 1;
    sym = 2 * lg + ((d >> eb) & 1);
    ev = d & ((1 << eb) - 1);
}
DF_FN int df_fixed_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// tokens: a literal is its byte; a match is bit 31 | (len - 3) << 15 | (dist - 1)
DF_FN uint32_t df_tok_match(int len, int dist) { return 0x80000000u | ((uint32_t)(len - 3) << 15) | (uint32_t)(dist - 1); }

// CRC32 (reflected 0xedb88320): a(x) * b(x) mod P, and x^(8 n) mod P
DF_FN uint32_t df_multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
DF_FN uint32_t df_x8n(uint32_t n)
{
    uint32_t base = 0x80000000u >> 8, p = 0x80000000u;     // x^8; x^0
    for (; n; n >>= 1) {
        if (n & 1) p = df_multmodp(base, p);
        base = df_multmodp(base, base);
    }
    return p;
}

// Code lengths of at most maxbits for the symbols with f[s] > 0 (see the head of the file).  All lanes call it.
DF_FN void df_build(DfShared &sh, const uint32_t *f, int nsym, int maxbits, uint8_t *len, int which)
{
    DF_LANES(l) {
        for (int s = l; s < nsym; s += DF_NL) len[s] = 0;
        if (l == 0) { uint32_t m = 0; for (int s = 0; s < nsym; ++s) m += f[s] != 0; sh.nused = m; }
    }
    DF_SYNC();
    DF_LANES(l) {
        for (int s = l; s < nsym; s += DF_NL) {
            const uint32_t fs = f[s];
            if (!fs) continue;
            int r = 0;
            for (int t = 0; t < nsym; ++t) { const uint32_t ft = f[t]; r += (ft && (ft < fs || (ft == fs && t < s))) ? 1 : 0; }
            sh.sorted[r] = (uint16_t)s;
        }
    }
    DF_SYNC();
    DF_LANES(l) {
        if (l != 0) continue;
        const int m = (int)sh.nused;
        sh.max_depth[which] = (uint16_t)(m ? 1 : 0);
        if (m == 0) { len[0] = len[1] = 1; continue; }
        if (m == 1) { const int s = sh.sorted[0]; len[s] = 1; len[s ? 0 : 1] = 1; continue; }
        // two-queue merge: leaves 0..m-1 in rising weight, internal node k is node m + k, made in rising weight too
        int a = 0, b = 0;
        for (int k = 0; k < m - 1; ++k) {
            uint32_t w = 0;
            for (int pick = 0; pick < 2; ++pick) {
                int node;
                if (a < m && (b >= k || f[sh.sorted[a]] <= sh.wint[b])) { node = a; w += f[sh.sorted[a]]; ++a; }
                else { node = m + b; w += sh.wint[b]; ++b; }
                sh.parent[node] = (uint16_t)(m + k);
            }
            sh.wint[k] = w;
        }
        sh.depth[2 * m - 2] = 0;
        for (int k = 2 * m - 3; k >= 0; --k) sh.depth[k] = (uint16_t)(sh.depth[sh.parent[k]] + 1);
        uint32_t blc[16];
        for (int d = 0; d < 16; ++d) blc[d] = 0;
        int deepest = 0;
        for (int k = 0; k < m; ++k) { int d = sh.depth[k]; if (d > deepest) deepest = d; if (d > maxbits) d = maxbits; ++blc[d]; }
        sh.max_depth[which] = (uint16_t)deepest;
        // Kraft sum in units of 2^-maxbits; too large: the deepest leaf above the limit goes one level down, too small: a leaf of
        // the deepest level goes one up (every term and the target are multiples of that level's unit, so this lands exactly)
        const uint32_t target = 1u << maxbits;
        uint32_t kraft = 0;
        for (int d = 1; d <= maxbits; ++d) kraft += blc[d] << (maxbits - d);
        while (kraft > target) {
            int d = maxbits - 1;
            while (d > 0 && !blc[d]) --d;
            if (d == 0) break;                       // cannot happen: more than 2^maxbits leaves
            --blc[d]; ++blc[d + 1]; kraft -= 1u << (maxbits - d - 1);
        }
        while (kraft < target) {
            int d = maxbits;
            while (d > 1 && !blc[d]) --d;
            if (d <= 1) break;                       // cannot happen with two or more leaves
            --blc[d]; ++blc[d - 1]; kraft += 1u << (maxbits - d);
        }
        int at = 0;
        for (int d = maxbits; d >= 1; --d) for (uint32_t c = 0; c < blc[d]; ++c) len[sh.sorted[at++]] = (uint8_t)d;
    }
    DF_SYNC();
}

// canonical codes of the lengths, bit-reversed (one lane)
DF_FN void df_codes(const uint8_t *len, int nsym, uint16_t *code)
{
    uint32_t blc[16], next[16];
    for (int d = 0; d < 16; ++d) blc[d] = 0;
    for (int s = 0; s < nsym; ++s) ++blc[len[s]];
    blc[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int d = 1; d < 16; ++d) { c = (c + blc[d - 1]) << 1; next[d] = c; }
    for (int s = 0; s < nsym; ++s) {
        const int n = len[s];
        uint32_t v = 0;
        if (n) { const uint32_t x = next[n]++; for (int k = 0; k < n; ++k) v |= ((x >> k) & 1u) << (n - 1 - k); }
        code[s] = (uint16_t)v;
    }
}

struct DfBits {                                          // one lane's bit writer into words that start out zero
    uint32_t *w; uint32_t n;
    DF_FN void put(DfBits &b, uint32_t v, int nbits)
    {
        const uint32_t at = b.n >> 5, sh = b.n & 31;
        b.w[at] |= v << sh;
        if (sh + (uint32_t)nbits > 32) b.w[at + 1] |= v >> (32 - sh);
        b.n += (uint32_t)nbits;
    }
};

// the bits of one token (or of end-of-block: is_eob) under the codes in sh; at most 48
DF_FN void df_tok_bits(const DfShared &sh, uint32_t t, bool is_eob, uint64_t &bits, int &nbits)
{
    if (is_eob) { bits = sh.lcode[256]; nbits = sh.llen[256]; return; }
    if (!(t & 0x80000000u)) { bits = sh.lcode[t]; nbits = sh.llen[t]; return; }
    int ls, leb, lev, ds, deb, dev;
    df_len_sym((int)((t >> 15) & 0xff) + 3, ls, leb, lev);
    df_dist_sym((int)(t & 0x7fff) + 1, ds, deb, dev);
    bits = sh.lcode[ls]; nbits = sh.llen[ls];
    bits |= (uint64_t)lev << nbits; nbits += leb;
    bits |= (uint64_t)sh.dcode[ds] << nbits; nbits += sh.dlen[ds];
    bits |= (uint64_t)dev << nbits; nbits += deb;
}

// One block: src[0, n) with 1 <= n <= DF_BLOCK -> out32 (at least DF_OUT_STRIDE bytes, 4-byte aligned), tok: scratch of n words,
// allow: DF_STORED | DF_FIXED | DF_DYNAMIC the chooser may take (stored stays the fallback of a block that would grow).
// Every lane of the workgroup calls it with the same arguments.
DF_FN void df_block(DfShared &sh, const uint8_t *src, uint32_t n, uint32_t *out32, uint32_t *tok, uint32_t allow, DfResult *res)
{
    uint8_t *out = (uint8_t *)out32;
    // ---- set-up: tables cleared, CRC table
    DF_LANES(l) {
        for (int k = l; k < DF_HSIZE; k += DF_NL) sh.htab[k] = 0;
        for (int k = l; k < 288; k += DF_NL) sh.fl[k] = 0;
        if (l < 32) sh.fd[l] = 0;
        if (l < 20) sh.fc[l] = 0;
        for (int e = l; e < 256; e += DF_NL) { uint32_t c = (uint32_t)e; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1; sh.crc_tab[e] = c; }
        if (l == 0) { sh.ntok = 0; sh.carry_pos = 0; sh.extra_bits = 0; sh.n_match = 0; sh.cm[0][DF_NL] = sh.cm[1][DF_NL] = 0; sh.cj[0][DF_NL] = sh.cj[1][DF_NL] = DF_NL; }
    }
    DF_SYNC();
    // ---- CRC32 of the slices
    const uint32_t slice = (n + DF_NL - 1) / DF_NL;
    DF_LANES(l) {
        uint32_t a = (uint32_t)l * slice; if (a > n) a = n;
        uint32_t e = a + slice; if (e > n) e = n;
        uint32_t c = 0xffffffffu;
        for (uint32_t i = a; i < e; ++i) c = sh.crc_tab[(c ^ src[i]) & 0xff] ^ (c >> 8);
        sh.crc_part[l] = c ^ 0xffffffffu;
    }
    // ---- tokens, chunk by chunk
    for (uint32_t base = 0; base < n; base += DF_NL) {
        DF_SYNC();
        const bool covered = sh.carry_pos >= base + DF_NL;      // a match runs over the whole chunk: its positions are only inserted
        if (!covered) {
            DF_LANES(l) {
                const uint32_t i = base + (uint32_t)l;
                int len = 0; uint32_t dist = 0;
                if (i + 4 <= n) {
                    const uint32_t j1 = sh.htab[df_hash(df_ld32(src + i))];
                    if (j1 && i - (j1 - 1) <= DF_MAX_DIST) {
                        const uint32_t left = n - i;
                        len = df_match_len(src + i, src + (j1 - 1), (int)(left < DF_MAX_MATCH ? left : DF_MAX_MATCH));
                        dist = i - (j1 - 1);
                        if (len < DF_MIN_MATCH) len = 0;
                    }
                }
                sh.adv[l] = (uint16_t)(len ? len : 1);
                sh.mdist[l] = (uint16_t)(len ? dist - 1 : 0);
                uint32_t j = (uint32_t)l + (len ? (uint32_t)len : 1u);
                sh.cj[0][l] = (uint8_t)(i < n && j < DF_NL ? j : DF_NL);
                sh.cm[0][l] = i < n ? 1ull << l : 0;
            }
            DF_SYNC();
        }
        DF_LANES(l) {
            const uint32_t i = base + (uint32_t)l;
            if (i + 4 <= n) DF_ATOMIC_MAX(&sh.htab[df_hash(df_ld32(src + i))], i + 1);
        }
        if (covered) continue;
        for (int r = 0; r < 6; ++r) {
            const int cur = r & 1, nxt = cur ^ 1;
            DF_LANES(l) {
                const int j = sh.cj[cur][l];
                sh.cm[nxt][l] = sh.cm[cur][l] | sh.cm[cur][j];
                sh.cj[nxt][l] = sh.cj[cur][j];
            }
            DF_SYNC();
        }
        DF_LANES(l) {
            const uint64_t sel = sh.cm[0][sh.carry_pos - base];     // base <= carry_pos < base + 64 here
            if (!((sel >> l) & 1)) continue;
            const uint32_t i = base + (uint32_t)l;
            const uint32_t at = sh.ntok + (uint32_t)df_popc64(sel & ((1ull << l) - 1));
            const int len = sh.adv[l];
            if (len >= DF_MIN_MATCH) {
                const int dist = (int)sh.mdist[l] + 1;
                int ls, leb, lev, ds, deb, dev;
                df_len_sym(len, ls, leb, lev); df_dist_sym(dist, ds, deb, dev);
                tok[at] = df_tok_match(len, dist);
                DF_ATOMIC_ADD(&sh.fl[ls], 1u); DF_ATOMIC_ADD(&sh.fd[ds], 1u);
                DF_ATOMIC_ADD(&sh.extra_bits, (uint32_t)(leb + deb)); DF_ATOMIC_ADD(&sh.n_match, 1u);
            } else {
                tok[at] = src[i];
                DF_ATOMIC_ADD(&sh.fl[src[i]], 1u);
            }
        }
        DF_SYNC();
        DF_LANES(l) {
            if (l != 0) continue;
            const uint64_t sel = sh.cm[0][sh.carry_pos - base];
            if (!sel) continue;                                     // the last match ended at the block's end, inside this chunk
            const int last = 63 - __builtin_clzll(sel);
            sh.ntok += (uint32_t)df_popc64(sel);
            sh.carry_pos = base + (uint32_t)last + sh.adv[last];
        }
    }
    DF_SYNC();
    // ---- CRC combined; end-of-block counted
    DF_LANES(l) {
        if (l != 0) continue;
        sh.fl[256] = 1;
        const uint32_t op = df_x8n(slice);
        uint32_t crc = sh.crc_part[0];
        for (uint32_t k = 1; k < DF_NL; ++k) {
            uint32_t a = k * slice; if (a > n) a = n;
            uint32_t e = a + slice; if (e > n) e = n;
            if (e == a) break;
            crc = df_multmodp(e - a == slice ? op : df_x8n(e - a), crc) ^ sh.crc_part[k];
        }
        res->crc = crc;
    }
    DF_SYNC();
    // ---- dynamic code lengths, the code-length alphabet, the three prices
    df_build(sh, sh.fl, 286, 15, sh.llen, 0);
    df_build(sh, sh.fd, 30, 15, sh.dlen, 1);
    DF_LANES(l) {
        if (l != 0) continue;
        int hlit = 286, hdist = 30;
        while (hlit > 257 && !sh.llen[hlit - 1]) --hlit;
        while (hdist > 1 && !sh.dlen[hdist - 1]) --hdist;
        sh.hlit = (uint32_t)hlit; sh.hdist = (uint32_t)hdist;
        const int total = hlit + hdist;
        for (int k = 0; k < hlit; ++k) sh.lens[k] = sh.llen[k];
        for (int k = 0; k < hdist; ++k) sh.lens[hlit + k] = sh.dlen[k];
        int nr = 0, i = 0;
        while (i < total) {
            const int v = sh.lens[i];
            int run = 1;
            while (i + run < total && sh.lens[i + run] == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = run < 138 ? run : 138; sh.rle[nr++] = (uint16_t)(18 | ((r - 11) << 8)); ++sh.fc[18]; run -= r; }
                if (run >= 3) { sh.rle[nr++] = (uint16_t)(17 | ((run - 3) << 8)); ++sh.fc[17]; run = 0; }
                while (run-- > 0) { sh.rle[nr++] = 0; ++sh.fc[0]; }
            } else {
                sh.rle[nr++] = (uint16_t)v; ++sh.fc[v]; --run;
                while (run >= 3) { const int r = run < 6 ? run : 6; sh.rle[nr++] = (uint16_t)(16 | ((r - 3) << 8)); ++sh.fc[16]; run -= r; }
                while (run-- > 0) { sh.rle[nr++] = (uint16_t)v; ++sh.fc[v]; }
            }
        }
        sh.nrle = (uint32_t)nr;
    }
    DF_SYNC();
    df_build(sh, sh.fc, 19, 7, sh.clen, 2);
    DF_LANES(l) {
        if (l != 0) continue;
        const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && !sh.clen[order[hclen - 1]]) --hclen;
        sh.hclen = (uint32_t)hclen;
        uint64_t dyn = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen, fix = 3;
        for (uint32_t k = 0; k < sh.nrle; ++k) { const int s = sh.rle[k] & 0xff; dyn += sh.clen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0); }
        for (int s = 0; s < 286; ++s) { dyn += (uint64_t)sh.fl[s] * sh.llen[s]; fix += (uint64_t)sh.fl[s] * (uint64_t)df_fixed_len(s); }
        for (int s = 0; s < 30; ++s) dyn += (uint64_t)sh.fd[s] * sh.dlen[s];
        dyn += sh.extra_bits; fix += sh.extra_bits + 5 * (uint64_t)sh.n_match;
        const uint32_t b_stored = n + 5, b_fixed = (uint32_t)((fix + 7) >> 3), b_dyn = (uint32_t)((dyn + 7) >> 3);
        uint32_t best = 0, bytes = 0xffffffffu;
        if ((allow & DF_STORED)) { best = 0; bytes = b_stored; }
        if ((allow & DF_FIXED) && b_fixed < bytes) { best = 1; bytes = b_fixed; }
        if ((allow & DF_DYNAMIC) && b_dyn < bytes) { best = 2; bytes = b_dyn; }
        if (bytes > b_stored) { best = 0; bytes = b_stored; }      // the fallback of a block that would grow, whatever is allowed
        sh.btype = best; sh.out_bytes = bytes;
        res->bytes = bytes; res->btype = best; res->pad_ = 0;
        for (int k = 0; k < 3; ++k) res->depth[k] = sh.max_depth[k];
    }
    DF_SYNC();
    if (sh.btype == 0) {
        DF_LANES(l) {
            if (l == 0) { out[0] = 1; out[1] = (uint8_t)(n & 0xff); out[2] = (uint8_t)(n >> 8); out[3] = (uint8_t)(~n & 0xff); out[4] = (uint8_t)((~n >> 8) & 0xff); }
            for (uint32_t i = (uint32_t)l; i < n; i += DF_NL) out[5 + i] = src[i];
        }
        return;
    }
    // ---- codes and the block header
    DF_LANES(l) {
        for (int k = l; k < 160; k += DF_NL) sh.hdr[k] = 0;
        for (int k = l; k < 104; k += DF_NL) sh.win[k] = 0;
        if (sh.btype == 1) {
            for (int s = l; s < 288; s += DF_NL) sh.llen[s] = (uint8_t)df_fixed_len(s);
            if (l < 32) sh.dlen[l] = 5;
        } else {
            for (int s = 286 + l; s < 288; s += DF_NL) sh.llen[s] = 0;
            if (l >= 30 && l < 32) sh.dlen[l] = 0;
        }
    }
    DF_SYNC();
    DF_LANES(l) {
        if (l != 0) continue;
        df_codes(sh.llen, 288, sh.lcode); df_codes(sh.dlen, 32, sh.dcode);
        DfBits b{sh.hdr, 0};
        DfBits::put(b, 1, 1); DfBits::put(b, sh.btype, 2);
        if (sh.btype == 2) {
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            df_codes(sh.clen, 19, sh.ccode);
            DfBits::put(b, sh.hlit - 257, 5); DfBits::put(b, sh.hdist - 1, 5); DfBits::put(b, sh.hclen - 4, 4);
            for (uint32_t k = 0; k < sh.hclen; ++k) DfBits::put(b, sh.clen[order[k]], 3);
            for (uint32_t k = 0; k < sh.nrle; ++k) {
                const int s = sh.rle[k] & 0xff, ev = sh.rle[k] >> 8;
                DfBits::put(b, sh.ccode[s], sh.clen[s]);
                if (s >= 16) DfBits::put(b, (uint32_t)ev, s == 16 ? 2 : s == 17 ? 3 : 7);
            }
        }
        sh.hdr_bits = b.n;
    }
    DF_SYNC();
    DF_LANES(l) {
        const uint32_t full = sh.hdr_bits >> 5;
        for (uint32_t k = (uint32_t)l; k < full; k += DF_NL) out32[k] = sh.hdr[k];
        if (l == 0) { sh.win[0] = sh.hdr[full]; sh.gbits = sh.hdr_bits; }
    }
    DF_SYNC();
    // ---- the tokens and end-of-block, 64 at a time
    const uint32_t n_emit = sh.ntok + 1;
    for (uint32_t g = 0; g < n_emit; g += DF_NL) {
        DF_LANES(l) {
            const uint32_t t = g + (uint32_t)l;
            uint64_t bits = 0; int nbits = 0;
            if (t < n_emit) df_tok_bits(sh, t < sh.ntok ? tok[t] : 0, t == sh.ntok, bits, nbits);
            sh.nb[l] = (uint16_t)nbits;
        }
        DF_SYNC();
        DF_LANES(l) {
            const uint32_t t = g + (uint32_t)l;
            if (t >= n_emit) continue;
            uint64_t bits = 0; int nbits = 0;
            df_tok_bits(sh, t < sh.ntok ? tok[t] : 0, t == sh.ntok, bits, nbits);
            uint32_t off = sh.gbits;
            for (int k = 0; k < l; ++k) off += sh.nb[k];
            const uint32_t w = (off >> 5) - (sh.gbits >> 5), s = off & 31;
            DF_ATOMIC_OR(&sh.win[w], (uint32_t)(bits << s));
            if (s + (uint32_t)nbits > 32) DF_ATOMIC_OR(&sh.win[w + 1], (uint32_t)(bits >> (32 - s)));
            if (s + (uint32_t)nbits > 64) DF_ATOMIC_OR(&sh.win[w + 2], (uint32_t)(bits >> (64 - s)));
        }
        DF_SYNC();
        DF_LANES(l) {
            uint32_t end = sh.gbits;
            for (int k = 0; k < DF_NL; ++k) end += sh.nb[k];
            const uint32_t w0 = sh.gbits >> 5, full = (end >> 5) - w0;
            for (uint32_t k = (uint32_t)l; k < full; k += DF_NL) out32[w0 + k] = sh.win[k];
            if (l == 0) { sh.carry = sh.win[full]; sh.gnext = end; }
        }
        DF_SYNC();
        DF_LANES(l) {
            for (int k = l; k < 104; k += DF_NL) sh.win[k] = k ? 0 : sh.carry;
            if (l == 0) sh.gbits = sh.gnext;
        }
        DF_SYNC();
    }
    DF_LANES(l) {
        if (l != 0) continue;
        const uint32_t w0 = sh.gbits >> 5, tail = ((sh.gbits & 31) + 7) >> 3;
        for (uint32_t k = 0; k < tail; ++k) out[4 * w0 + k] = (uint8_t)(sh.win[0] >> (8 * k));
    }
}

}  // namespace ps
