// ps_stage.hip -- the small device passes between the search launches (gfx950), written to the budget of ps_budget.h.
//
// Two batches are in flight per device (ps_pipeline.h, Work): while one batch's search launch is resident on every CU,
// the other batch runs its selection and locate stages and prepares its next search.  A resident first-tier launch leaves
// PS_STAGE_VGPRS registers per lane and no LDS on a CU, so a kernel of the other stream starts beside it only if it asks
// for no more -- the library scan and radix-sort kernels these passes replace (17-20 KB of LDS, up to 100 VGPRs) waited
// for the whole launch to drain.  Everything here is one wave per workgroup, registers and cross-lane moves only.
#include <hip/hip_runtime.h>
#include <stdexcept>
#include "ps_kernels.h"
#include "ps_budget.h"

namespace ps {

// ---- stable counting sort of 8-bit keys: queue position -> read (the hand-out order of a search launch) ---------------
// The reads are cut into n_wg contiguous chunks, one wave each.  A wave keeps its 256 bin counters in registers: lane l
// holds bins l, 64 + l, 128 + l and 192 + l.  k_sort_hist counts a chunk, k_sort_scan turns the bin-major table
// [bin][chunk] into exclusive offsets inside every bin (and the bins' totals), k_sort_scatter adds the bins' own offsets
// and places the reads: tile by tile in input order, the lanes of a tile that share a key ranked by a ballot, so equal
// keys keep their input order (the leading-base locality inside an effort class).
struct BinCounters { uint32_t c[4]; };

// adds n to the counter of bin k (both wave-uniform) and returns its value before
__device__ __forceinline__ uint32_t bins_fetch_add(BinCounters &b, int lane, int k, uint32_t n)
{
    const int owner = k & 63, j = k >> 6;
    uint32_t before;
    if (j == 0) { before = (uint32_t)__builtin_amdgcn_readlane((int)b.c[0], owner); if (lane == owner) b.c[0] += n; }
    else if (j == 1) { before = (uint32_t)__builtin_amdgcn_readlane((int)b.c[1], owner); if (lane == owner) b.c[1] += n; }
    else if (j == 2) { before = (uint32_t)__builtin_amdgcn_readlane((int)b.c[2], owner); if (lane == owner) b.c[2] += n; }
    else { before = (uint32_t)__builtin_amdgcn_readlane((int)b.c[3], owner); if (lane == owner) b.c[3] += n; }
    return before;
}
// one tile of up to 64 keys: every distinct key of the tile in turn (a wave-uniform loop); returns this lane's place
__device__ __forceinline__ uint32_t bins_take_tile(BinCounters &b, int lane, bool valid, int key)
{
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    unsigned long long todo = __ballot(valid);
    uint32_t place = 0;
    while (todo) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
        const int k = __builtin_amdgcn_readlane(key, src);
        const bool mine = valid && key == k;
        const unsigned long long m = __ballot(mine);
        const uint32_t before = bins_fetch_add(b, lane, k, (uint32_t)__popcll(m));
        if (mine) place = before + (uint32_t)__popcll(m & lane_lt);
        todo &= ~m;
    }
    return place;
}
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64); if (lane >= o) v += u; }
    return v;
}

__global__ void __launch_bounds__(64) k_sort_hist(const uint8_t *key, int n, int chunk, int n_wg, uint32_t *table)
{
    const int lane = threadIdx.x, wg = blockIdx.x;
    const long long beg = (long long)wg * chunk, end = beg + chunk < n ? beg + chunk : n;
    BinCounters b = {{0, 0, 0, 0}};
    for (long long at = beg; at < end; at += 64) {
        const long long i = at + lane;
        const bool valid = i < end;
        (void)bins_take_tile(b, lane, valid, valid ? (int)key[i] : 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) table[(size_t)(64 * j + lane) * n_wg + wg] = b.c[j];
}
// one wave per bin: exclusive sums along the bin's row of the table, the bin's total to totals[bin]
__global__ void __launch_bounds__(64) k_sort_scan(uint32_t *table, int n_wg, uint32_t *totals)
{
    const int lane = threadIdx.x;
    uint32_t *row = table + (size_t)blockIdx.x * n_wg;
    const int per = (n_wg + 63) / 64, lo = lane * per, hi = lo + per < n_wg ? lo + per : n_wg;
    uint32_t sum = 0;
    for (int t = lo; t < hi; ++t) sum += row[t];
    const uint32_t incl = wave_inclusive_sum(sum, lane);
    uint32_t run = incl - sum;
    for (int t = lo; t < hi; ++t) { const uint32_t v = row[t]; row[t] = run; run += v; }
    if (lane == 63) totals[blockIdx.x] = incl;
}
__global__ void __launch_bounds__(64) k_sort_scatter(const uint8_t *key, int n, int chunk, int n_wg, const uint32_t *table, const uint32_t *totals, int32_t *order)
{
    const int lane = threadIdx.x, wg = blockIdx.x;
    const long long beg = (long long)wg * chunk, end = beg + chunk < n ? beg + chunk : n;
    BinCounters b;
    uint32_t below = 0;                                   // reads in the bins of the rows before row j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t t = totals[64 * j + lane], incl = wave_inclusive_sum(t, lane);
        b.c[j] = below + (incl - t) + table[(size_t)(64 * j + lane) * n_wg + wg];
        below += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    for (long long at = beg; at < end; at += 64) {
        const long long i = at + lane;
        const bool valid = i < end;
        const uint32_t place = bins_take_tile(b, lane, valid, valid ? (int)key[i] : 0);
        if (valid && place < (uint32_t)n) order[place] = (int32_t)i;
    }
}

size_t order_sort_tmp_words(int n) { (void)n; return (size_t)256 * PS_SORT_MAX_WG + 256; }
void launch_order_sort(const uint8_t *key, int n, uint32_t *tmp, int32_t *order, hipStream_t s)
{
    if (n <= 0) return;
    long long wgs = ((long long)n + 4095) / 4096;                        // 64-bit: n may be just below 2^31
    if (wgs > PS_SORT_MAX_WG) wgs = PS_SORT_MAX_WG;
    long long per = ((long long)n + wgs - 1) / wgs;
    per = (per + 63) / 64 * 64;
    const int chunk = (int)per, n_wg = (int)(((long long)n + per - 1) / per);
    uint32_t *table = tmp, *totals = tmp + (size_t)256 * PS_SORT_MAX_WG;
    hipLaunchKernelGGL(k_sort_hist, dim3(n_wg), dim3(64), 0, s, key, n, chunk, n_wg, table);
    hipLaunchKernelGGL(k_sort_scan, dim3(256), dim3(64), 0, s, table, n_wg, totals);
    hipLaunchKernelGGL(k_sort_scatter, dim3(n_wg), dim3(64), 0, s, key, n, chunk, n_wg, table, totals, order);
}

// ---- draws before every read of the tie-break stream -------------------------------------------------------------------
// e_before[g] / h_before[g] = reads of class 1 / class 2 in front of read g (input order).  The host has the classes and
// hands over the two counts in front of every group of 64 reads (grp[2 * (g / 64)], + 1); a wave takes one group at a
// time and adds the rank inside it with two ballots.
__global__ void __launch_bounds__(256) k_class_ranks(const uint8_t *cls, long long n, const uint32_t *grp, uint32_t *e_before, uint32_t *h_before)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    const long long n_groups = (n + 63) >> 6, n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long q = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; q < n_groups; q += n_waves) {
        const long long g = (q << 6) + lane;
        const int c = g < n ? (int)(cls[g] & 3) : 0;
        const unsigned long long m1 = __ballot(c == 1), m2 = __ballot(c == 2);
        if (g < n) {
            e_before[g] = grp[2 * q] + (uint32_t)__popcll(m1 & lane_lt);
            h_before[g] = grp[2 * q + 1] + (uint32_t)__popcll(m2 & lane_lt);
        }
    }
}
void launch_class_ranks(const uint8_t *cls, long long n, const uint32_t *grp, uint32_t *e_before, uint32_t *h_before, hipStream_t s)
{
    if (n <= 0) return;
    long long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_class_ranks, dim3((unsigned int)blocks), dim3(256), 0, s, cls, n, grp, e_before, h_before);
}

}  // namespace ps
