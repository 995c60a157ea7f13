// bamrec_check -- csrc/ps_bamrec.h under g++ alone (no HIP): cases from a file -> bamrec_size, the filled bytes and the key fields.
//
//   bamrec_check <cases> <out>
// cases:  ref <ACGT text>            the packed forward strand (l_pac bases, packed into exactly (l_pac + 3) / 4 bytes)
//         contigs <n> <off len>...
//         holes <n> <off len>...
//         max_top2 <v>
//         rec <name hex> <seq digits 0-4> <qual hex | -> <type> <pos> <strand> <mapq> <n_mm> <n_gapo> <n_gape> <c1> <c2> <n_cigar> <words>...
// out:    one line per rec: <size> <ref> <pos> <end> <flag> <mapq> <bytes hex>
// Every input array is a heap block of exactly its size and dst stands between guard bytes, so that a sanitizer build (and the
// guards without one) sees any byte read or written outside.  The record is filled twice over two different backgrounds: a byte
// of it that bamrec_fill leaves unwritten differs between the two.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "ps_bamrec.h"

static std::vector<uint8_t> unhex(const std::string &h)
{
    std::vector<uint8_t> o;
    for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return o;
}
template <class T> static T *exact(const std::vector<T> &v)      // a heap block of exactly v.size() elements (one, unread, when empty)
{
    T *p = (T *)std::malloc(std::max<size_t>(1, v.size() * sizeof(T)));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: bamrec_check <cases> <out>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    if (!in || !out) { std::fprintf(stderr, "bamrec_check: cannot open the files\n"); return 2; }
    std::vector<uint8_t> pac(1, 0); int64_t l_pac = 0;
    std::vector<int64_t> coff, hoff; std::vector<int32_t> clen, hlen; int max_top2 = 30;
    uint8_t *d_pac = nullptr; int64_t *d_coff = nullptr, *d_hoff = nullptr; int32_t *d_clen = nullptr, *d_hlen = nullptr;
    std::string line; long n_case = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what; s >> what;
        if (what == "ref") {
            std::string t; s >> t;
            l_pac = (int64_t)t.size();
            pac.assign((size_t)std::max<int64_t>(1, (l_pac + 3) / 4), 0);
            for (int64_t p = 0; p < l_pac; ++p) { const char *w = std::strchr("ACGT", t[(size_t)p]); pac[(size_t)p >> 2] |= (uint8_t)((w ? w - "ACGT" : 0) << ((~p & 3) << 1)); }
            std::free(d_pac); d_pac = exact(pac);
        } else if (what == "contigs" || what == "holes") {
            int n; s >> n;
            std::vector<int64_t> &o = what == "contigs" ? coff : hoff; std::vector<int32_t> &l = what == "contigs" ? clen : hlen;
            o.assign((size_t)n, 0); l.assign((size_t)n, 0);
            for (int k = 0; k < n; ++k) s >> o[k] >> l[k];
            if (what == "contigs") { std::free(d_coff); std::free(d_clen); d_coff = exact(o); d_clen = exact(l); }
            else { std::free(d_hoff); std::free(d_hlen); d_hoff = exact(o); d_hlen = exact(l); }
        } else if (what == "max_top2") s >> max_top2;
        else if (what == "rec") {
            ++n_case;
            std::string name_h, seq_s, qual_h; int n_cigar = 0;
            ps::RecIn r; std::memset(&r, 0, sizeof r);
            s >> name_h >> seq_s >> qual_h >> r.type >> r.pos >> r.strand >> r.mapq >> r.n_mm >> r.n_gapo >> r.n_gape >> r.c1 >> r.c2 >> n_cigar;
            std::vector<uint32_t> cig((size_t)n_cigar);
            for (int k = 0; k < n_cigar; ++k) s >> cig[k];
            if (!s) { std::fprintf(stderr, "bamrec_check: bad case %ld\n", n_case); return 2; }
            const std::vector<uint8_t> name = unhex(name_h), qual = qual_h == "-" ? std::vector<uint8_t>() : unhex(qual_h);
            std::vector<uint8_t> seq; for (char c : seq_s) seq.push_back((uint8_t)(c - '0'));
            uint8_t *p_name = exact(name), *p_seq = exact(seq), *p_qual = exact(qual); uint32_t *p_cig = exact(cig);
            r.name = (const char *)p_name; r.name_len = (uint32_t)name.size(); r.seq = p_seq; r.len = (int32_t)seq.size();
            r.qual = qual_h == "-" ? nullptr : (const char *)p_qual;
            r.cigar = p_cig; r.n_cigar = n_cigar;
            r.pac = d_pac; r.l_pac = l_pac; r.contig_off = d_coff; r.contig_len = d_clen; r.n_contigs = (int32_t)coff.size();
            r.hole_off = d_hoff; r.hole_len = d_hlen; r.n_holes = (int32_t)hoff.size(); r.max_top2 = max_top2;
            const uint32_t n = ps::bamrec_size(r);
            ps::RecKey k; ps::bamrec_key(r, k);
            const size_t G = 32;
            uint8_t *a = (uint8_t *)std::malloc(n + 2 * G), *b = (uint8_t *)std::malloc(n + 2 * G);
            std::memset(a, 0xA5, n + 2 * G); std::memset(b, 0x5A, n + 2 * G);
            ps::bamrec_fill(r, a + G); ps::bamrec_fill(r, b + G);
            for (size_t i = 0; i < G; ++i)
                if (a[i] != 0xA5 || a[G + n + i] != 0xA5 || b[i] != 0x5A || b[G + n + i] != 0x5A) { std::fprintf(stderr, "bamrec_check: case %ld wrote outside its %u bytes\n", n_case, n); return 1; }
            if (std::memcmp(a + G, b + G, n) != 0) { std::fprintf(stderr, "bamrec_check: case %ld left a byte of its %u unwritten\n", n_case, n); return 1; }
            out << n << ' ' << k.ref << ' ' << k.pos << ' ' << k.end << ' ' << k.flag << ' ' << k.mapq << ' ';
            static const char H[] = "0123456789abcdef";
            std::string hex; for (uint32_t i = 0; i < n; ++i) { hex.push_back(H[a[G + i] >> 4]); hex.push_back(H[a[G + i] & 15]); }
            out << hex << '\n';
            std::free(a); std::free(b); std::free(p_name); std::free(p_seq); std::free(p_qual); std::free(p_cig);
        }
    }
    std::free(d_pac); std::free(d_coff); std::free(d_clen); std::free(d_hoff); std::free(d_hlen);
    return out.good() ? 0 : 1;
}
