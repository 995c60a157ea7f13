// ps_bamsort.h -- the coordinate order of BAM records and the gather of the sorted stream, stated once for host and device
// (the pattern of ps_bamrec.h and ps_deflate.h: no HIP header here; ps_bamsort.hip runs it as k_bamsort_gather, tests/bamsort_check.cpp
// under the host compiler alone).
//
// THE KEY.  (uint32_t)ref in the high word, (uint32_t)pos ^ 0x80000000 in the low word.  Ascending unsigned order of the key is the
// comparator of ps_bam.cpp's sort_records: ref compares as unsigned (-1, unplaced, sorts last), pos as signed; a stable sort of
// the keys keeps input order among equal ones, as std::stable_sort does.
//
// THE GATHER.  Record i of the sorted order is src[soff, soff + len) and goes to out[doff[i], doff[i + 1]); doff is the exclusive
// sum of the lengths in sorted order.  A GROUP is 64 consecutive records of the sorted order and the work of BS_NL = 64 lanes that
// share a BsShared (LDS on the device).  The group's destination is one contiguous byte range [beg, end); its sources are scattered
// and share no alignment with it.  The group is a sequence of REGIONS (BS_LANES) separated by BS_SYNC: on the device a region runs
// once per lane and BS_SYNC is the workgroup barrier, the host build runs the lanes of a region one after the other.  Both write the
// same bytes because no lane reads in a region what another lane writes in it, and two lanes never write the same byte.
//   1. Records [s, e) whose range fits BS_STAGE are staged: staging byte x stands for out[beg_al + x], beg_al = beg rounded down to
//      16.  For every record the lanes take the 4-byte words of the staging that its bytes touch; a lane builds its word from the one
//      or two aligned 4-byte source words that hold the bytes (a funnel shift in registers) and stores it whole, or -- where the
//      word is shared with the neighbouring record -- only the record's bytes of it.
//   2. The lanes copy the staging out in aligned 16-byte units.  A unit that reaches outside [beg, end) is shared with a
//      neighbouring group's range: only there bytes go out one by one, and none outside the range.
//   3. A record that alone is larger than the staging goes straight through: its lanes build each aligned 16-byte destination unit
//      from five aligned source words, the partial units at its two ends byte by byte.
// Source words are read whole and aligned, never outside [soff rounded down to 4, soff + len rounded up to 4): the source buffer
// starts at a multiple of 4 and is allocated up to a multiple of 4.  Every loop is bounded by a record length or the 64 lanes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "ps_types.h"

namespace ps {

enum { BS_NL = 64, BS_STAGE = 24576 };                  // 64 records of a 50-base read take ~12 KB, of a 101-base read ~19 KB

PS_HD uint64_t bamsort_key(int32_t ref, int32_t pos) { return ((uint64_t)(uint32_t)ref << 32) | (uint64_t)((uint32_t)pos ^ 0x80000000u); }
// bits of the key that a sort has to look at: `any` is the OR of all keys
PS_HD int bamsort_end_bit(uint64_t any) { int b = 0; while (b < 64 && (any >> b) != 0) ++b; return b < 1 ? 1 : b; }

#ifdef PS_BS_DEVICE
#define BS_FN static __device__ __forceinline__
#define BS_LANES(l) for (int l = (int)threadIdx.x, bs_once_ = 0; bs_once_ == 0; ++bs_once_)
#define BS_SYNC() __syncthreads()
#else
#define BS_FN static inline
#define BS_LANES(l) for (int l = 0; l < BS_NL; ++l)
#define BS_SYNC() ((void)0)
#endif

typedef uint32_t __attribute__((may_alias)) bs_u32;
struct __attribute__((aligned(16), may_alias)) BsUnit { uint32_t w[4]; };

struct BsShared {
    uint64_t soff[BS_NL], doff[BS_NL + 1]; uint32_t len[BS_NL];
    __attribute__((aligned(16))) uint8_t stage[BS_STAGE];
};

// the records: bytes and, per record of the input, offset and length; perm: the sorted order; doff: n + 1 destination offsets
struct BsArgs {
    const uint8_t *src; const uint64_t *rec_off; const uint32_t *rec_len;
    const uint32_t *perm; const uint64_t *doff; uint64_t n; uint8_t *out;
};

// the four bytes of the record at source address a .. a + 3 (a may lie up to 3 before the record or reach past its end: those bytes
// are zero), from aligned words inside [lo, hi)
BS_FN uint32_t bs_src_word(const uint8_t *src, int64_t a, int64_t lo, int64_t hi)
{
    const int64_t a0 = a & ~(int64_t)3; const uint32_t sh = (uint32_t)(a & 3) * 8;
    uint32_t x = 0, y = 0;
    if (a0 >= lo && a0 < hi) x = *(const bs_u32 *)(src + a0);
    if (sh == 0) return x;
    if (a0 + 4 >= lo && a0 + 4 < hi) y = *(const bs_u32 *)(src + a0 + 4);
    return (x >> sh) | (y << (32 - sh));
}

// region 1, one lane's share of one record: staging bytes [dl, dl + len) from src[soff, soff + len)
BS_FN void bs_stage_record(const uint8_t *src, uint64_t soff, uint32_t len, uint32_t dl, int lane, uint8_t *stage)
{
    const int64_t lo = (int64_t)(soff & ~(uint64_t)3), hi = (int64_t)((soff + len + 3) & ~(uint64_t)3);
    const uint32_t w1 = (dl + len + 3) >> 2;
    for (uint32_t w = (dl >> 2) + (uint32_t)lane; w < w1; w += BS_NL) {
        const uint32_t x = w << 2;
        const uint32_t v = bs_src_word(src, (int64_t)soff + (int64_t)x - (int64_t)dl, lo, hi);
        if (x >= dl && x + 4 <= dl + len) *(bs_u32 *)(stage + x) = v;
        else for (uint32_t j = 0; j < 4; ++j) if (x + j >= dl && x + j < dl + len) stage[x + j] = (uint8_t)(v >> (8 * j));
    }
}

// region 2, one lane's share: staging -> out[beg, end), staging byte x standing for out[beg_al + x]
BS_FN void bs_store_units(const uint8_t *stage, uint64_t beg, uint64_t end, uint64_t beg_al, int lane, uint8_t *out)
{
    const uint32_t n_units = (uint32_t)((end - beg_al + 15) >> 4);              // <= BS_STAGE / 16
    for (uint32_t u = (uint32_t)lane; u < n_units; u += BS_NL) {
        const uint64_t at = beg_al + ((uint64_t)u << 4);
        if (at >= beg && at + 16 <= end) *(BsUnit *)(out + at) = *(const BsUnit *)(stage + ((size_t)u << 4));
        else for (uint32_t j = 0; j < 16; ++j) if (at + j >= beg && at + j < end) out[at + j] = stage[((size_t)u << 4) + j];
    }
}

// region 3, one lane's share of a record that goes straight through: out[o0, o0 + len) from src[soff, soff + len)
BS_FN void bs_direct_record(const uint8_t *src, uint64_t soff, uint32_t len, uint64_t o0, int lane, uint8_t *out)
{
    const int64_t lo = (int64_t)(soff & ~(uint64_t)3), hi = (int64_t)((soff + len + 3) & ~(uint64_t)3);
    const uint64_t o1 = o0 + len, al = o0 & ~(uint64_t)15;
    const uint32_t n_units = (uint32_t)((o1 - al + 15) >> 4);
    for (uint32_t u = (uint32_t)lane; u < n_units; u += BS_NL) {
        const uint64_t at = al + ((uint64_t)u << 4);
        BsUnit v;
        for (int k = 0; k < 4; ++k) v.w[k] = bs_src_word(src, (int64_t)soff + (int64_t)(at + 4 * (uint64_t)k) - (int64_t)o0, lo, hi);
        if (at >= o0 && at + 16 <= o1) *(BsUnit *)(out + at) = v;
        else for (uint32_t j = 0; j < 16; ++j) if (at + j >= o0 && at + j < o1) out[at + j] = (uint8_t)(v.w[j >> 2] >> (8 * (j & 3)));
    }
}

// group g0 / 64 of the sorted order: records [g0, min(n, g0 + 64))
BS_FN void bamsort_gather_group(BsShared &sh, const BsArgs &a, uint64_t g0)
{
    if (g0 >= a.n) return;
    const int cnt = (int)(a.n - g0 < BS_NL ? a.n - g0 : BS_NL);
    BS_LANES(l) {
        if (l < cnt) {
            const uint32_t r = a.perm[g0 + (uint64_t)l];
            const uint64_t d0 = a.doff[g0 + (uint64_t)l], room = a.doff[g0 + (uint64_t)l + 1] - d0;     // the record's length by construction; a lane never writes past it
            sh.soff[l] = a.rec_off[r]; sh.len[l] = a.rec_len[r] < room ? a.rec_len[r] : (uint32_t)room; sh.doff[l] = d0;
            if (l == cnt - 1) sh.doff[cnt] = d0 + room;
        }
    }
    BS_SYNC();
    int s = 0;
    while (s < cnt) {                                                          // every pass takes at least one record
        const uint64_t beg = sh.doff[s], beg_al = beg & ~(uint64_t)15;
        int e = s;
        while (e < cnt && sh.doff[e + 1] - beg_al <= BS_STAGE) ++e;            // the same for every lane
        if (e == s) {
            BS_LANES(l) bs_direct_record(a.src, sh.soff[s], sh.len[s], beg, l, a.out);
            s = s + 1;
            continue;
        }
        for (int r = s; r < e; ++r)
            BS_LANES(l) bs_stage_record(a.src, sh.soff[r], sh.len[r], (uint32_t)(sh.doff[r] - beg_al), l, sh.stage);
        BS_SYNC();
        BS_LANES(l) bs_store_units(sh.stage, beg, sh.doff[e], beg_al, l, a.out);
        BS_SYNC();
        s = e;
    }
}

// ---- the staging of the device route: two page-locked halves of one PIECE each.  Plain host functions, so that the check program
// runs the very code that run_route runs.
const size_t BS_PIECE_DEFAULT = (size_t)64 << 20, BS_PIECE_MIN = 256;

// PS_BAM_SORT_PIECE=<bytes> (tests): the size of one half.  Unset, empty, not a number or <= 0: the default; never more than the default
// (the knob cannot grow the page-locked allocation), never less than 256; rounded down to a multiple of 64, so that the second half and
// the column sub-arrays keep their alignment.
static inline size_t bamsort_piece_bytes(const char *value)
{
    if (!value || !value[0]) return BS_PIECE_DEFAULT;
    const long long v = atoll(value);
    if (v <= 0 || v >= (long long)BS_PIECE_DEFAULT) return BS_PIECE_DEFAULT;
    return v < (long long)BS_PIECE_MIN ? BS_PIECE_MIN : (size_t)v & ~(size_t)63;
}

// The four per-record columns go up `per` records at a time, as four sub-arrays of one half: the source offset (8 bytes per record),
// then the length and the order's two columns (4 bytes each) -- 20 bytes per record in all.
static inline size_t bamsort_columns_per_piece(size_t piece) { return piece / 20; }
struct BsColumnsAt { size_t off, len, ref, pos; };      // byte offsets inside the half
static inline BsColumnsAt bamsort_columns_at(size_t per) { return BsColumnsAt{0, 8 * per, 12 * per, 16 * per}; }

// The upload's cut: the parts go up back to back in pieces that ignore part and record boundaries.  The cursor names the next source
// byte; one cut is the run of bytes of the cursor's part that still fits into `room` bytes of the half (none for an empty part), and
// taking it moves the cursor on, to the next part where this one is used up.  The caller stops at room 0 or behind the last part.
struct BsCursor { size_t part = 0; uint64_t in_part = 0; };
struct BsCut { size_t part; uint64_t in_part; size_t take; };
static inline BsCut bamsort_next_cut(BsCursor &c, uint64_t part_bytes, size_t room)
{
    const uint64_t left = part_bytes - c.in_part;
    const BsCut cut{c.part, c.in_part, left < room ? (size_t)left : room};
    c.in_part += cut.take;
    if (c.in_part == part_bytes) { ++c.part; c.in_part = 0; }
    return cut;
}

// ---- the host side of the device route (ps_bamsort.hip); BamSortJob: ps_bam.h
struct BamSortJob;
struct BamSortStats { uint32_t on_device = 0; uint64_t n_records = 0, bytes = 0, n_calls_device = 0, n_calls_host = 0, n_resident = 0; double ms_upload = 0, ms_sort = 0, ms_gather = 0, ms_download = 0; };
// The switch of ps_bam_sort_device / PS_BAM_SORT_GPU: device >= 0 registers the route with ps_bam.cpp's coordinate sort, -1 takes it
// out again and gives the device and page-locked buffers back; either way the counters start again.  Throws when there is no such device.
void bam_sort_set_device(int device);
void bam_sort_info(BamSortStats &out);
// One call of the route on `device`, whatever the switch says.  False, counted as a host call and nothing done: 2^32 records or
// more, or more device memory needed than PS_BAM_SORT_MAX_MB (default 32768) -- decided before the first device call.  Calls are
// serialised: they share one set of staging and device buffers.  st (may be null): this call alone.
bool bam_sort_device_run(BamSortJob &job, int device, BamSortStats *st);

}  // namespace ps
