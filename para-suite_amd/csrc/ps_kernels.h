// ps_kernels.h -- launch interface of the gfx950 kernels (ps_kernels.hip, ps_index.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "ps_types.h"
#include "ps_budget.h"

namespace ps {

static const int PS_MAX_CIGAR = 16;

struct WidthArgs {
    IndexView ix;
    int n_reads, len, seed_len, use_seed;
    const int32_t *lens;     // per-read lengths (nullptr: all len)
    const uint32_t *bases; const uint32_t *nmask;
    uint32_t *w; uint32_t *cwb; uint32_t *cswb;   // compact width bytes, 4 positions per word, [word][n_reads]
    KStats *stats;
};

// Effort estimate (scheduling only, never a result): a read's search effort follows the score of its best hit, which is unknown
// before the search; two greedy scans (from either end of the read) give a cheap estimate of it -- k_effort, ps_kernels.hip
struct EffortArgs {
    IndexView ix;
    int n_reads, len;
    const int32_t *lens;
    const uint32_t *bases; const uint32_t *nmask;
    uint32_t s_pk[5];        // substitution costs as the search uses them (Model::s_mm_pk)
    int c_restart;           // charged where a scan has to start a new piece
    uint32_t w_pin;          // a substitution is believed where the interval is at most this wide (the scan has pinned its locus down)
    uint8_t *est;            // out: estimated score of the best hit, clipped to 255
    uint16_t *est_ab;        // optional (profiling): the two scans' totals (7 bits each) and whether each had to start over (bit 7)
};

// expected search nodes of a read from its estimated final budget and its D(i) bounds (ps_effort.hip); out: the sort key of the hand-out order
struct EffortModelArgs {
    int n_reads, len;
    const int32_t *lens; const uint8_t *units_by_len;
    const uint32_t *bases; const uint32_t *nmask; const uint32_t *cwb;
    const uint8_t *est;
    uint32_t s_pk[5]; uint32_t inv_c_min;
    int max_units, u_tight, seed_units, use_seed, seed_len;
    int max_gapo, indel_end_skip, u_gapo_ins, u_gapo_del;   // gap openings: one insertion child, four deletion children where the search allows an indel
    int depth;               // levels modelled (beyond ~19 symbols a random string no longer occurs in a genome of this size)
    float rows;              // BWT rows: a string of d symbols has min(1, rows / 4^d) expected occurrences
    int log_scale;           // key = 255 - log2(expected nodes) * log_scale
    uint8_t *key; float *pred;      // pred: optional (profiling)
};

struct RefineItem { int32_t read; bwtint rb; int32_t ref_shift; int32_t strand; };
struct RefineArgs {
    IndexView ix;
    int n_items, len, n_reads;             // len: the longest read (sizes the H/E rows)
    const int32_t *lens;                   // per-read lengths (nullptr: all len)
    const uint32_t *bases; const uint32_t *nmask;
    const RefineItem *items;
    uint32_t *cigar; int32_t *n_cigar;     // [n_items][PS_MAX_CIGAR]
    uint8_t *zbuf; size_t z_per_block;     // traceback scratch, 64 lanes interleaved per block
    int32_t *hebuf; size_t he_per_block;   // H and E rows, [row][j][lane]: refine_he_words(len) words per block
};
inline size_t refine_he_words(int len) { return (size_t)(len + 2) * 64 * 2; }

// dynamic LDS above the 48 KiB default needs the kernel's opt-in.  A request above a CU's 160 KiB, or one the runtime refuses,
// throws here with the kernel's name and the byte count -- it must not fail the launch and surface at the next error check
// as someone else's error
static const size_t PS_LDS_PER_CU = 160 * 1024;
void set_dynamic_lds(const void *kernel, const char *name, size_t bytes);

void launch_width(const WidthArgs &a, hipStream_t s);
void launch_effort(const EffortArgs &a, hipStream_t s);
void launch_effort_model(const EffortModelArgs &a, hipStream_t s);
// false: model outside the packed ranges.  stats: the narrow tiers' kernel with per-lane counters (KStats, read_iters); the timed kernel carries none
// fills the jump table of an index (ps_core.h): `levels` levels, jump_words(levels) words at `table`
void launch_jump_build(const IndexView &ix, uint32_t *table, int levels, hipStream_t s);
bool launch_backtrack(const BtArgs &a, const BtArgs *d_args /* device copy, filled here */, BtArgs *h_stage /* page-locked, one per stream: the source of that upload */,
                      int n_blocks, int lm_stride, hipStream_t s, bool stats);
void launch_index_check(const IndexView &ix, unsigned long long *out /* device: rows visited, symbol mismatches, sample mismatches, longest arc */, hipStream_t s);
void launch_sa2pos(const IndexView &ix, const bwtint *rows, bwtint *out, int n, KStats *stats, hipStream_t s);
void launch_refine(const RefineArgs &a, int n_blocks, hipStream_t s);
// ps_stage.hip: the hand-out order (order[queue position] = read, a STABLE sort of the 8-bit keys; tmp: order_sort_tmp_words(n) words) and
// the tie-break stream's prefix counts (grp: the class-1 / class-2 reads in front of every group of 64 reads, from the host)
size_t order_sort_tmp_words(int n);
void launch_order_sort(const uint8_t *key, int n, uint32_t *tmp, int32_t *order, hipStream_t s);
void launch_class_ranks(const uint8_t *cls, long long n, const uint32_t *grp, uint32_t *e_before, uint32_t *h_before, hipStream_t s);

// ps_collapse.hip: the groups of identical reads of a bin (ps_collapse.h has the rule).  In: the bin's packed reads.  Scratch, all on the
// device: key, perm[2], order, rep_of, slot, reps: n elements each; digit: n bytes; sort_tmp: order_sort_tmp_words(n) words; part:
// 2 * PS_SORT_MAX_WG words; m: one word.  Out: rep_of[read] = its group's representative (a representative names itself), reps[q] = the
// q-th representative in bin order, slot[representative] = q, *m = their number
struct CollapseArgs {
    int n, n_bw, n_mw, len, hash_bits;
    const int32_t *lens;     // per-read lengths (nullptr: all len)
    const uint32_t *bases; const uint32_t *nmask;
    uint64_t *key; int32_t *perm[2]; uint8_t *digit; int32_t *order; uint32_t *sort_tmp; uint32_t *part;
    int32_t *rep_of, *slot, *reps; uint32_t *m;
};
int collapse_sort_passes(int hash_bits);                      // LSD passes over the key's bytes
void launch_collapse_groups(const CollapseArgs &a, hipStream_t s);
// the representatives' words and lengths, word-major with stride m (out_lens: only read when a.lens is set)
void launch_collapse_gather(const CollapseArgs &a, int m, uint32_t *out_bases, uint32_t *out_nmask, int32_t *out_lens, hipStream_t s);
// every read's hit list, count and state from its representative's (t_*: the search's output over the m representatives, stride aln_cap)
void launch_collapse_expand(const CollapseArgs &a, int m, const AlnRec *t_alns, const int32_t *t_n_aln, const uint8_t *t_status, int aln_cap,
                            AlnRec *alns, int32_t *n_aln, uint8_t *status, hipStream_t s);

}  // namespace ps
