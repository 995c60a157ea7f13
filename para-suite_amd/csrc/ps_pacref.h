// ps_pacref.h -- device-side access to record bases and reference bases (the index's packed forward strand + its hole
// table), shared by the error-profile and the clustering kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ps {

__device__ __forceinline__ int bam_nibble(const uint8_t *seq, uint64_t base) { return (seq[base >> 1] >> ((~base & 1u) << 2)) & 15; }   // base `base` of 4-bit packed bases, high nibble first
__device__ __forceinline__ int prof_read_code(const uint8_t *seq, uint64_t base)     // BAM nibble -> 0..3, -1 otherwise
{
    const int nib = bam_nibble(seq, base);
    return nib == 1 ? 0 : (nib == 2 ? 1 : (nib == 4 ? 2 : (nib == 8 ? 3 : -1)));
}
struct ProfRef {              // reference bases of one record with its holes
    const uint8_t *pac; const int64_t *hole_off; const int32_t *hole_len; int n_holes, h;
    __device__ void seek(int64_t p)           // first hole that ends behind p
    {
        int lo = 0, hi = n_holes;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (hole_off[mid] + hole_len[mid] <= p) lo = mid + 1; else hi = mid; }
        h = lo;
    }
    __device__ int at(int64_t p) const
    {
        int k = h;
        while (k < n_holes && hole_off[k] + hole_len[k] <= p) ++k;
        if (k < n_holes && hole_off[k] <= p) return -1;
        return (pac[p >> 2] >> ((~p & 3) << 1)) & 3;
    }
    // the same as text, for the modes that write sequence (ps_fetch): the base as a letter -- its complement with `comp` --
    // and inside a hole the hole's upper-cased character, which has no complement
    const uint8_t *hole_chr = nullptr;
    __device__ int letter_at(int64_t p, bool comp) const
    {
        int k = h;
        while (k < n_holes && hole_off[k] + hole_len[k] <= p) ++k;
        if (k < n_holes && hole_off[k] <= p) return -(int)hole_chr[k];     // < 0: from a hole
        const int code = (pac[p >> 2] >> ((~p & 3) << 1)) & 3;
        return (0x54474341u >> ((comp ? 3 - code : code) << 3)) & 0xff;   // "ACGT"
    }
};

}  // namespace ps
