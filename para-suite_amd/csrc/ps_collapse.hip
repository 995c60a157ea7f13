// ps_collapse.hip -- the device stages of the collapsed search (gfx950): the groups of identical reads of a bin, one
// representative per group gathered for the search launch, its result copied to the group afterwards.  The grouping rule is
// ps_collapse.h; search_bin() (ps_search.hip) runs these stages in front of the first tier.
//
// The stages of one batch run beside the other lane's resident search launch, so every kernel here keeps to ps_budget.h: at most
// PS_STAGE_VGPRS registers and no LDS (tests/test_collapse_budget_cpu.py).  What needs a running value along the reads -- the
// last head in front of a sorted position, the representatives in front of a read -- is done the way the hand-out order's
// counting sort does it (ps_stage.hip): the reads are cut into at most PS_SORT_MAX_WG chunks of one wave each, a first kernel
// leaves one number per chunk, the second starts from the numbers of the chunks in front of its own.
#include <hip/hip_runtime.h>
#include "ps_kernels.h"
#include "ps_budget.h"
#include "ps_collapse.h"

namespace ps {

__device__ __forceinline__ int wave_max_all(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_all(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// stage 1: the 64-bit key of every read
__global__ void __launch_bounds__(256) k_collapse_keys(const uint32_t *bases, const uint32_t *nmask, const int32_t *lens, int n, int n_bw, int n_mw, int len,
                                                       int hash_bits, uint64_t *key)
{
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x)
        key[r] = collapse_key(bases, nmask, lens, (size_t)n, (size_t)r, n_bw, n_mw, len, hash_bits);
}

// stage 2, between two passes of the LSD sort over the key's bytes: the pass that ended left order[place] = position in the
// sequence it sorted, so the reads now stand as perm_out[j] = perm_in[order[j]] (perm_in null: the identity, order null: nothing
// sorted yet); the next pass sorts digit[j] = byte `shift / 8` of the key of the read at j.  Every pass is stable, so equal
// keys end in ascending local index.
__global__ void __launch_bounds__(256) k_collapse_step(const uint64_t *key, const int32_t *perm_in, const int32_t *order, int32_t *perm_out, int n, int shift,
                                                       uint8_t *digit)
{
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        int src = order ? order[j] : (int)j;
        if ((unsigned)src >= (unsigned)n) src = (int)j;                 // never taken: an index read from memory is not followed outside the arrays
        int r = perm_in ? perm_in[src] : src;
        if ((unsigned)r >= (unsigned)n) r = (int)j;
        if (perm_out) perm_out[j] = r;
        if (digit) digit[j] = (uint8_t)(key[r] >> shift);
    }
}

// stage 3: heads in sorted order (ps_collapse.h: the head rule), one wave per chunk; last_head[chunk] = the chunk's last head, -1: none
__global__ void __launch_bounds__(64) k_collapse_heads(const uint32_t *bases, const uint32_t *nmask, const int32_t *lens, int n, int n_bw, int n_mw,
                                                       const int32_t *perm, int chunk, uint8_t *head, int32_t *last_head)
{
    const int lane = threadIdx.x, wg = blockIdx.x;
    const long long beg = (long long)wg * chunk, end = beg + chunk < n ? beg + chunk : n;
    int last = -1;
    for (long long j = beg + lane; j < end; j += 64) {
        const bool h = collapse_is_head(bases, nmask, lens, (size_t)n, perm, (size_t)j, n_bw, n_mw);
        head[j] = h ? 1 : 0;
        if (h) last = (int)j;
    }
    last = wave_max_all(last);
    if (lane == 0) last_head[wg] = last;
}

// stage 4: rep_of[read] = the read at the last head at or in front of the read's sorted position
__global__ void __launch_bounds__(64) k_collapse_reps(const int32_t *perm, const uint8_t *head, const int32_t *last_head, int n, int chunk, int32_t *rep_of)
{
    const int lane = threadIdx.x, wg = blockIdx.x;
    const long long beg = (long long)wg * chunk, end = beg + chunk < n ? beg + chunk : n;
    int carry = -1;
    for (int t = lane; t < wg; t += 64) { const int v = last_head[t]; carry = v > carry ? v : carry; }
    carry = wave_max_all(carry);
    for (long long at = beg; at < end; at += 64) {
        const long long j = at + lane;
        const bool valid = j < end;
        int v = (valid && head[j]) ? (int)j : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o, 64); if (lane >= o && u > v) v = u; }
        if (carry > v) v = carry;
        if (v < 0) v = 0;                                               // never taken: sorted position 0 is a head
        if (valid) {
            const int r = perm[j], rep = perm[v];
            if ((unsigned)r < (unsigned)n) rep_of[r] = (unsigned)rep < (unsigned)n ? rep : r;
        }
        carry = __builtin_amdgcn_readlane(v, 63);
    }
}

// stage 5: the representatives in BIN order (the leading-base order of the bin is what the launch's hand-out order falls back to).
// n_reps[chunk] = representatives of the chunk; then slot[rep] = its place among them, reps[place] = rep, *m = their number
__global__ void __launch_bounds__(64) k_collapse_count(const int32_t *rep_of, int n, int chunk, uint32_t *n_reps)
{
    const int lane = threadIdx.x, wg = blockIdx.x;
    const long long beg = (long long)wg * chunk, end = beg + chunk < n ? beg + chunk : n;
    uint32_t c = 0;
    for (long long r = beg + lane; r < end; r += 64) c += rep_of[r] == (int32_t)r ? 1u : 0u;
    c = wave_sum_all(c);
    if (lane == 0) n_reps[wg] = c;
}
__global__ void __launch_bounds__(64) k_collapse_compact(const int32_t *rep_of, const uint32_t *n_reps, int n, int chunk, int n_wg, int32_t *slot, int32_t *reps, uint32_t *m)
{
    const int lane = threadIdx.x, wg = blockIdx.x;
    const unsigned long long lane_lt = (1ull << lane) - 1ull;
    const long long beg = (long long)wg * chunk, end = beg + chunk < n ? beg + chunk : n;
    uint32_t at_rep = 0;
    for (int t = lane; t < wg; t += 64) at_rep += n_reps[t];
    at_rep = wave_sum_all(at_rep);
    for (long long at = beg; at < end; at += 64) {
        const long long r = at + lane;
        const bool is_rep = r < end && rep_of[r] == (int32_t)r;
        const unsigned long long mask = __ballot(is_rep);
        const uint32_t place = at_rep + (uint32_t)__popcll(mask & lane_lt);
        if (is_rep && place < (uint32_t)n) { slot[r] = (int32_t)place; reps[place] = (int32_t)r; }
        at_rep += (uint32_t)__popcll(mask);
    }
    if (wg == n_wg - 1 && lane == 0) *m = at_rep;
}

// stage 6: the representatives' words and lengths, word-major with stride m
__global__ void __launch_bounds__(256) k_collapse_gather(const uint32_t *bases, const uint32_t *nmask, const int32_t *lens, int n, int n_bw, int n_mw,
                                                         const int32_t *reps, int m, uint32_t *out_bases, uint32_t *out_nmask, int32_t *out_lens)
{
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (long long)gridDim.x * blockDim.x) {
        const int r = reps[q];
        if ((unsigned)r >= (unsigned)n) continue;
        for (int w = 0; w < n_bw; ++w) out_bases[(size_t)w * m + q] = bases[(size_t)w * n + r];
        for (int w = 0; w < n_mw; ++w) out_nmask[(size_t)w * m + q] = nmask[(size_t)w * n + r];
        if (lens) out_lens[q] = lens[r];
    }
}

// behind the search of the m representatives: every read's slot of the bin's hit lists, counts and states from its representative.
// One lane per (read, hit): the aln_cap lanes of a read write one contiguous stretch
__global__ void __launch_bounds__(256) k_collapse_expand(const AlnRec *t_alns, const int32_t *t_n_aln, const uint8_t *t_status, int aln_cap, int m,
                                                         const int32_t *rep_of, const int32_t *slot, int n, AlnRec *alns, int32_t *n_aln, uint8_t *status)
{
    const long long total = (long long)n * aln_cap;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / aln_cap), j = (int)(i - (long long)r * aln_cap);
        const int rep = rep_of[r];
        if ((unsigned)rep >= (unsigned)n) continue;
        const int q = slot[rep];
        if ((unsigned)q >= (unsigned)m) continue;
        const int na = t_n_aln[q];
        if (j == 0) { n_aln[r] = na; status[r] = t_status[q]; }
        if (j < na) alns[(size_t)r * aln_cap + j] = t_alns[(size_t)q * aln_cap + j];
    }
}

static inline dim3 grid_for(long long n) { long long b = (n + 255) / 256; return dim3((unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b))); }

int collapse_sort_passes(int hash_bits) { const int bits = hash_bits < 1 ? 1 : (hash_bits > 64 ? 64 : hash_bits); return (bits + 7) / 8; }

void launch_collapse_groups(const CollapseArgs &a, hipStream_t s)
{
    const int n = a.n;
    if (n <= 0) return;
    // the chunks of launch_order_sort (ps_stage.hip): whole waves' worth of reads, at most PS_SORT_MAX_WG of them
    long long wgs = ((long long)n + 4095) / 4096;
    if (wgs > PS_SORT_MAX_WG) wgs = PS_SORT_MAX_WG;
    long long per = ((long long)n + wgs - 1) / wgs;
    per = (per + 63) / 64 * 64;
    const int chunk = (int)per, n_wg = (int)(((long long)n + per - 1) / per);
    const int hash_bits = a.hash_bits < 1 ? 1 : (a.hash_bits > 64 ? 64 : a.hash_bits);
    hipLaunchKernelGGL(k_collapse_keys, grid_for(n), dim3(256), 0, s, a.bases, a.nmask, a.lens, n, a.n_bw, a.n_mw, a.len, hash_bits, a.key);
    const int passes = collapse_sort_passes(hash_bits);
    const int32_t *perm = nullptr;                                      // how the reads stand: null = bin order
    for (int p = 0; p <= passes; ++p) {
        int32_t *out = p ? a.perm[(p - 1) & 1] : nullptr;
        hipLaunchKernelGGL(k_collapse_step, grid_for(n), dim3(256), 0, s, a.key, perm, p ? a.order : nullptr, out, n, 8 * p, p < passes ? a.digit : nullptr);
        if (p) perm = out;
        if (p < passes) launch_order_sort(a.digit, n, a.sort_tmp, a.order, s);
    }
    uint8_t *head = a.digit;                                            // the digits are spent
    int32_t *last_head = reinterpret_cast<int32_t *>(a.part);
    uint32_t *n_reps = a.part + PS_SORT_MAX_WG;
    hipLaunchKernelGGL(k_collapse_heads, dim3(n_wg), dim3(64), 0, s, a.bases, a.nmask, a.lens, n, a.n_bw, a.n_mw, perm, chunk, head, last_head);
    hipLaunchKernelGGL(k_collapse_reps, dim3(n_wg), dim3(64), 0, s, perm, head, last_head, n, chunk, a.rep_of);
    hipLaunchKernelGGL(k_collapse_count, dim3(n_wg), dim3(64), 0, s, a.rep_of, n, chunk, n_reps);
    hipLaunchKernelGGL(k_collapse_compact, dim3(n_wg), dim3(64), 0, s, a.rep_of, n_reps, n, chunk, n_wg, a.slot, a.reps, a.m);
}

void launch_collapse_gather(const CollapseArgs &a, int m, uint32_t *out_bases, uint32_t *out_nmask, int32_t *out_lens, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_collapse_gather, grid_for(m), dim3(256), 0, s, a.bases, a.nmask, a.lens, a.n, a.n_bw, a.n_mw, a.reps, m, out_bases, out_nmask, out_lens);
}

void launch_collapse_expand(const CollapseArgs &a, int m, const AlnRec *t_alns, const int32_t *t_n_aln, const uint8_t *t_status, int aln_cap,
                            AlnRec *alns, int32_t *n_aln, uint8_t *status, hipStream_t s)
{
    if (a.n <= 0 || aln_cap <= 0) return;
    hipLaunchKernelGGL(k_collapse_expand, grid_for((long long)a.n * aln_cap), dim3(256), 0, s, t_alns, t_n_aln, t_status, aln_cap, m, a.rep_of, a.slot, a.n,
                       alns, n_aln, status);
}

}  // namespace ps
