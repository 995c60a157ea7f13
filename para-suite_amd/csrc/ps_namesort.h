// ps_namesort.h -- the name order of BAM records (`samtools sort -n`: ps_bam.cpp's strnum_cmp, then first of pair before second) as
// a key that sorts by its bytes, stated once for host and device (the pattern of ps_bamsort.h: no HIP header here; ps_bamsort.hip
// runs it in k_namesort_rows, tests/namesort_check.cpp under the host compiler alone).
//
// THE KEY.  strnum_cmp cuts a name into maximal digit runs and single other bytes, and the cut does not depend on the other name.
// So every name has a byte key whose zero-padded memcmp order is the comparator:
//   a byte c that is no digit   -> c
//   a maximal run of digits     -> 0x30, then one byte: the run's length once its leading '0's are dropped (0 for a run of zeros,
//                                  254 at the most), then the digits that are left
//   the end of the name         -> zero bytes from there on
// A digit against another byte compares as the raw bytes do in strnum_cmp; every digit lies in 0x30..0x39 and no other byte does, so
// the one marker 0x30 stands for any digit there.  Two runs compare by the length without leading zeros, then digit by digit over
// that equal length; runs of zeros of any length are equal ("a0", "a00").  The name that ends first is the smaller one: every token
// begins with a byte that is not zero, so the padding never meets its like.  Names are bytes: 0x80 and above are no digits.
// A key is at most 2 * len + 1 bytes long ("1a1a...1").
//
// THE ROW.  L: the longest name of the call, without its NUL (254 at the most).  A row is W = namesort_words(L) 32-bit words:
// bytes [0, 4W - 1) are the key, zero padded (byte 4W - 2 is always zero), byte 4W - 1 is (flag >> 6) & 3, the tie-break of
// sort_records.  Bytes are packed big-endian, so comparing the words 0 .. W - 1 as unsigned numbers is the memcmp.  Rows are stored
// column-major: word w of record i at col[w * n + i].
//
// THE GENERATOR.  NsGen walks one name and hands out one key byte per call: the position in the name, the end of the digit run it
// is in, and where it stands (at a token's start, before the length byte, inside the digits).  Every loop is bounded by the name's
// length.  After the key's end it hands out zeros for ever.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "ps_types.h"

namespace ps {

enum { NS_NL = 64, NS_MAX_NAME = 254, NS_NAME_STRIDE = 65 };    // NS_NAME_STRIDE: words between two names of a group (256 bytes and one word: odd)
enum { NS_TOKEN = 0, NS_LENGTH = 1, NS_DIGITS = 2 };

PS_HD uint32_t namesort_words(uint32_t longest) { return (2 * longest + 3 + 3) >> 2; }
PS_HD bool namesort_digit(uint8_t c) { return c >= 0x30 && c <= 0x39; }

struct NsGen { uint32_t pos = 0, run_end = 0, mode = NS_TOKEN; };

PS_HD uint8_t namesort_next(NsGen &g, const uint8_t *name, uint32_t len)
{
    if (g.mode == NS_DIGITS) {
        const uint8_t c = name[g.pos++];
        if (g.pos == g.run_end) g.mode = NS_TOKEN;
        return c;
    }
    if (g.mode == NS_LENGTH) {
        const uint32_t left = g.run_end - g.pos;
        g.mode = left ? NS_DIGITS : NS_TOKEN;
        return (uint8_t)left;
    }
    if (g.pos >= len) return 0;
    const uint8_t c = name[g.pos];
    if (!namesort_digit(c)) { ++g.pos; return c; }
    uint32_t e = g.pos + 1;
    while (e < len && namesort_digit(name[e])) ++e;
    while (g.pos < e && name[g.pos] == 0x30) ++g.pos;
    g.run_end = e; g.mode = NS_LENGTH;
    return 0x30;
}

// the next four key bytes as one word of the row
PS_HD uint32_t namesort_next_word(NsGen &g, const uint8_t *name, uint32_t len)
{
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k) v = (v << 8) | namesort_next(g, name, len);
    return v;
}
// word w of a row of W words: the row's last byte is the pair byte
PS_HD uint32_t namesort_row_word(uint32_t key_word, uint32_t w, uint32_t W, uint32_t pair) { return w + 1 == W ? (key_word & ~(uint32_t)0xff) | (pair & 3u) : key_word; }
PS_HD uint32_t namesort_pair(uint32_t flag) { return (flag >> 6) & 3u; }

// one whole row, words `stride` apart (host: the check program and the tests' third opinion; the device takes the words one by one)
inline void namesort_row(const uint8_t *name, uint32_t len, uint32_t pair, uint32_t W, uint32_t *row, size_t stride)
{
    NsGen g;
    for (uint32_t w = 0; w < W; ++w) row[(size_t)w * stride] = namesort_row_word(namesort_next_word(g, name, len), w, W, pair);
}
inline int namesort_row_cmp(const uint32_t *a, const uint32_t *b, uint32_t W, size_t stride)
{
    for (uint32_t w = 0; w < W; ++w) { const uint32_t x = a[(size_t)w * stride], y = b[(size_t)w * stride]; if (x != y) return x < y ? -1 : 1; }
    return 0;
}
// the bits of a column that a sort has to look at: [begin, end) of the bits in which any two rows differ (diff = and ^ or, not zero)
PS_HD int namesort_begin_bit(uint32_t diff) { int b = 0; while (b < 31 && !((diff >> b) & 1u)) ++b; return b; }
PS_HD int namesort_end_bit(uint32_t diff) { int b = 32; while (b > 1 && !((diff >> (b - 1)) & 1u)) --b; return b; }

// ---- the host side of the device route (ps_bamsort.hip); BamSortJob: ps_bam.h
struct BamSortJob;
struct BamNameSortStats {
    uint32_t on_device = 0, key_words = 0; uint64_t n_records = 0, bytes = 0, n_calls_device = 0, n_calls_host = 0, n_resident = 0, n_passes = 0;
    double ms_upload = 0, ms_keys = 0, ms_sort = 0, ms_gather = 0, ms_download = 0;
};
// The switch of ps_bam_name_sort_device / PS_BAM_NAME_SORT_GPU: device >= 0 registers the route with ps_bam.cpp's name sort, -1 takes
// it out again and gives back the device and page-locked buffers that the coordinate switch does not need; either way this switch's
// counters start again.  Throws when there is no such device.
void bam_name_sort_set_device(int device);
void bam_name_sort_info(BamNameSortStats &out);
// One call of the route on `device`, whatever the switch says.  False, counted as a host call and nothing done: 2^32 records or more,
// a record whose name does not end inside it or is longer than 254 bytes, or more device memory needed than PS_BAM_SORT_MAX_MB
// -- decided before the first device call.  Calls share the coordinate route's buffers and are serialised with it.
bool bam_name_sort_device_run(BamSortJob &job, int device, BamNameSortStats *st);

}  // namespace ps
