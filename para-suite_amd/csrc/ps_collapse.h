// ps_collapse.h -- the grouping rule of the collapsed search (ps_collapse.hip): which reads of a bin are THE SAME READ, so
// that one of them is searched and the others take its result.  A read's hit list is a function of its bases, its N
// positions, its length and the cost model; the bin fixes the model, so identity is those three.  Nothing from HIP is
// included: tests/test_collapse_cpu.py builds this header with the host compiler and runs the whole chain on the host.
//
// A bin stores its reads word-major: word w of read r is bases[w * n + r] (n_bw words of 16 bases) and nmask[w * n + r]
// (n_mw words of 32 flags), lens[r] its length when the bin is ragged (nullptr: every read has the bin's length).  The
// packing leaves every bit behind a read's end zero and packs an N as base code 0, so
//   - the length is part of identity: a 30-base read and the 36-base read that continues it with As have the same words;
//   - the N mask is part of identity: ...A... and ...N... have the same base words;
//   - a read and its reverse complement are different reads (nothing here folds strands).
//
// Groups are EXACT: the key only brings candidates next to each other in a stable sort of (key, local index); two reads
// share a group only after collapse_equal() has compared every word and the length.  Groups may be INCOMPLETE: where reads
// of equal key and different sequence interleave in the sorted order (A B A), the run of As is cut in two and the second
// part gets a representative of its own.  That costs a search, never a wrong result.
#pragma once
#include "ps_types.h"

namespace ps {

PS_HD uint64_t collapse_mix(uint64_t h, uint64_t v)             // one word into the running key (the finaliser of splitmix64)
{
    h = (h ^ v) + 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    return h ^ (h >> 31);
}

// the key of read r: every base word, every mask word, the length.  hash_bits < 64 keeps the low bits only (tests: colliding
// keys become common and collapse_equal() is what separates them)
PS_HD uint64_t collapse_key(const uint32_t *bases, const uint32_t *nmask, const int32_t *lens, size_t n, size_t r, int n_bw, int n_mw, int len, int hash_bits)
{
    uint64_t h = collapse_mix(0, (uint64_t)(uint32_t)(lens ? lens[r] : len));
    for (int w = 0; w < n_bw; ++w) h = collapse_mix(h, bases[(size_t)w * n + r]);
    for (int w = 0; w < n_mw; ++w) h = collapse_mix(h, 0x100000000ull | nmask[(size_t)w * n + r]);
    return hash_bits >= 64 ? h : (hash_bits <= 0 ? 0 : h & ((1ull << hash_bits) - 1ull));
}

// the same read: same length, same base words, same mask words
PS_HD bool collapse_equal(const uint32_t *bases, const uint32_t *nmask, const int32_t *lens, size_t n, size_t a, size_t b, int n_bw, int n_mw)
{
    if (lens && lens[a] != lens[b]) return false;
    for (int w = 0; w < n_bw; ++w) if (bases[(size_t)w * n + a] != bases[(size_t)w * n + b]) return false;
    for (int w = 0; w < n_mw; ++w) if (nmask[(size_t)w * n + a] != nmask[(size_t)w * n + b]) return false;
    return true;
}

// The head rule.  perm: the reads in (key, local index) order.  The read at sorted position j opens a group unless it equals
// its predecessor in that order, compared in full; a group's head is its representative, so a representative maps to itself.
PS_HD bool collapse_is_head(const uint32_t *bases, const uint32_t *nmask, const int32_t *lens, size_t n, const int32_t *perm, size_t j, int n_bw, int n_mw)
{
    return j == 0 || !collapse_equal(bases, nmask, lens, n, (size_t)perm[j - 1], (size_t)perm[j], n_bw, n_mw);
}

}  // namespace ps
