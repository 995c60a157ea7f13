// collapse_check.cpp -- stand-alone driver of csrc/ps_collapse.h for tests/test_collapse_cpu.py (host compiler, sanitizers on).
//   collapse_check <hash_bits> <reads.txt>
// reads.txt: one read per line, letters ACGT and N.  The reads are packed the way a bin packs them (ps_pipeline.hip: word-major,
// 16 bases / 32 N flags per word, every bit behind a read's end zero, an N packed as base code 0, the word counts of the longest
// read, a length per read), then the chain of the device stages runs on the host: key -> stable sort of (key, index) -> heads
// -> rep_of.  Prints rep_of, one line per read in input order.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "ps_collapse.h"

using namespace ps;

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: collapse_check <hash_bits> <reads.txt>\n"); return 2; }
    const int hash_bits = std::atoi(argv[1]);
    std::ifstream in(argv[2]);
    std::vector<std::string> reads;
    for (std::string line; std::getline(in, line);) if (!line.empty()) reads.push_back(line);
    const size_t n = reads.size();
    if (!n) { std::fprintf(stderr, "no reads\n"); return 2; }
    int len = 0;
    for (const std::string &r : reads) len = std::max(len, (int)r.size());
    const int n_bw = (len + 15) / 16, n_mw = (len + 31) / 32;
    std::vector<uint32_t> bases((size_t)n_bw * n, 0), nmask((size_t)n_mw * n, 0);
    std::vector<int32_t> lens(n);
    for (size_t r = 0; r < n; ++r) {
        lens[r] = (int32_t)reads[r].size();
        for (int j = 0; j < lens[r]; ++j) {
            const char c = reads[r][(size_t)j];
            const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
            if (code <= 3) bases[(size_t)(j / 16) * n + r] |= (uint32_t)code << (2 * (j & 15));
            else nmask[(size_t)(j / 32) * n + r] |= 1u << (j & 31);
        }
    }
    std::vector<uint64_t> key(n);
    for (size_t r = 0; r < n; ++r) key[r] = collapse_key(bases.data(), nmask.data(), lens.data(), n, r, n_bw, n_mw, len, hash_bits);
    std::vector<int32_t> perm(n);
    for (size_t r = 0; r < n; ++r) perm[r] = (int32_t)r;
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
    std::vector<int32_t> rep_of(n, -1);
    int32_t rep = -1;
    for (size_t j = 0; j < n; ++j) {
        if (collapse_is_head(bases.data(), nmask.data(), lens.data(), n, perm.data(), j, n_bw, n_mw)) rep = perm[j];
        rep_of[(size_t)perm[j]] = rep;
    }
    for (size_t r = 0; r < n; ++r) std::printf("%d\n", rep_of[r]);
    return 0;
}
