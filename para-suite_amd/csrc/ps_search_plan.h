// ps_search_plan.h -- the parts of a search launch (ps_search.hip) with no device in them: the environment knobs of the search
// stage, the launch geometry (which the reservation of a lane's workspace shares), and the budget-by-length table of a ragged
// launch.  Nothing from HIP is included: tests/test_search_plan_cpu.py builds this header with the host compiler.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include "ps_budget.h"
#include "ps_core.h"
#include "ps_error.h"
#include "ps_model.h"

namespace ps {

// Every knob a search reads (DESIGN.md section 4j has the table).  Read once per batch_search, not per context: bench.py and the
// tests change PS_CAP between two searches of one context; the context-lifetime knobs (PS_N_BIG, PS_POOL_CAP, ...) are Ctx::Ctx's.
struct SearchKnobs {
    int order = 1, order_min = 4096, order_restart = 0 /* 0: an average mismatch of the model */, order_wpin = 16, order_cap = 255, order_scale = 8;
    int max_per_cu = PS_SEARCH_WAVES;   // workgroups per CU the kernel's registers allow (ps_kernels.hip: PS_BT_WAVES)
    bool cap = true; int cap_bias = 0;  // the first tier spares entries by the estimate; tests: estimates too low by that much, so that the restart path runs
    bool skip = true;                   // barren steps inside the jump table's levels are crossed in one iteration (ps_narrow.h: nt_skip)
    int chase_min2 = PS_CHASE_MIN2;     // lanes of a wave that must want the second chase step of an iteration (65: never)
    bool chase = true;                  // ... and below them a barren step takes its match child's step in the same iteration (ps_narrow.h: nt_chase)
    int fetch_min = 8, hit_min = 1;     // tuning: the context's values unless set at search time
    bool collapse = false;              // identical reads of a bin are searched once (ps_collapse.h); a context may state its own (ps_ctx_set_collapse)
    int collapse_hash_bits = 64;        // tests: bits of the grouping key that are kept, so that different reads share a key
};
inline SearchKnobs search_knobs_from_env(int ctx_fetch_min, int ctx_hit_min)
{
    SearchKnobs k; int v = 0;
    k.fetch_min = ctx_fetch_min; k.hit_min = ctx_hit_min;
    if (env_int("PS_ORDER", v)) k.order = v;                       // 0: no hand-out order, 2: by the estimated best score alone (A/B runs)
    if (env_int("PS_ORDER_MIN", v)) k.order_min = std::max(1, v);  // below that every read has a lane to itself at once: no order to choose (tests: the small launches of the fuzz sweep too)
    if (env_int("PS_ORDER_RESTART", v)) k.order_restart = std::max(1, v);
    if (env_int("PS_ORDER_WPIN", v)) k.order_wpin = std::max(1, v);
    if (env_int("PS_ORDER_CAP", v)) k.order_cap = std::max(1, std::min(255, v));
    if (env_int("PS_ORDER_SCALE", v)) k.order_scale = std::max(1, std::min(12, v));
    if (env_int("PS_MAX_PER_CU", v)) k.max_per_cu = v;
    if (env_int("PS_CAP", v)) k.cap = v != 0;
    if (env_int("PS_CAP_BIAS", v)) k.cap_bias = std::max(0, std::min(200, v));
    if (env_int("PS_SKIP", v)) k.skip = v != 0;
    if (env_int("PS_CHASE", v)) k.chase = v != 0;
    if (env_int("PS_CHASE_MIN2", v)) k.chase_min2 = std::max(1, std::min(65, v));
    if (env_int("PS_FETCH_MIN", v)) k.fetch_min = std::max(1, v);
    if (env_int("PS_HIT_MIN", v)) k.hit_min = std::max(1, v);
    if (env_int("PS_COLLAPSE", v)) k.collapse = v != 0;
    if (env_int("PS_COLLAPSE_HASH_BITS", v)) k.collapse_hash_bits = std::max(1, std::min(64, v));
    return k;
}

// Geometry of a search launch.  Workgroups of 256 lanes: as many per CU as their LDS state (lm_bytes per lane) lets in, at
// most max_per_cu, on every CU (or bt_blocks of them, stated); no more than the reads fill; and no more lanes than 64 GiB of
// narrow stack (16 B x pool_cap per lane) or 32 GiB of wide stack (32 B x pool_cap + the bucket heads) hold.  A narrow launch
// below the largest narrow stack also gets large slots of 65,535 entries for the reads that outgrow their slice.
struct SearchPlan { int blocks = 0, lanes = 0; size_t pool_bytes = 0, head_words = 0; uint32_t n_big = 0; size_t big_bytes = 0; };
static const uint32_t PS_BIG_CAP = 65535;          // entries of a large slot: the most a narrow stack links
inline SearchPlan plan_search(int64_t n_reads, int lm_bytes_per_lane, uint32_t pool_cap, bool wide, int cus, int bt_blocks, int max_per_cu, int n_big)
{
    int per_cu = (int)(PS_CU_LDS / ((size_t)256 * lm_bytes_per_lane));
    if (per_cu < 1) throw Error("read length / score range too large for the per-lane LDS state");
    if (bt_blocks <= 0 && max_per_cu < 1) throw Error("PS_MAX_PER_CU must be at least 1");
    int64_t blocks = std::min<int64_t>(bt_blocks > 0 ? bt_blocks : (int64_t)cus * std::min(per_cu, max_per_cu), (n_reads + 255) / 256);
    // bound the lanes by stack memory (the widest tier keeps 64 MB per lane)
    const size_t entry = wide ? sizeof(Entry) : sizeof(Entry16), per_lane = (size_t)pool_cap * entry + (wide ? PS_MAX_BUCKETS * 4 : 0);
    const size_t max_lanes = ((size_t)(wide ? 32 : 64) << 30) / per_lane;
    if ((size_t)blocks * 256 > max_lanes) blocks = (int64_t)std::max<size_t>(1, max_lanes / 256);
    SearchPlan p;
    p.blocks = (int)blocks; p.lanes = p.blocks * 256;
    p.pool_bytes = (size_t)p.lanes * pool_cap * entry;
    p.head_words = wide ? (size_t)p.lanes * PS_MAX_BUCKETS : 0;
    if (!wide && pool_cap < PS_BIG_CAP && n_big > 0) {
        p.n_big = (uint32_t)std::min<int64_t>(n_big, std::max<int64_t>(64, n_reads));
        p.big_bytes = (size_t)p.n_big * PS_BIG_CAP * sizeof(Entry16);
    }
    return p;
}
// What a lane of work allocates ahead of its first search: the first tier's launch of the flagship model (4 workgroups per CU)
// with reads for every lane -- whatever PS_MAX_PER_CU says, as ever: below 4 a launch takes less than was reserved.  Nothing when
// the first tier is the wide one: that is sized by the launch.
inline SearchPlan plan_search_reserve(uint32_t pool_cap, int cus, int bt_blocks, int n_big)
{
    if (pool_cap > PS_BIG_CAP) return SearchPlan();
    return plan_search(INT32_MAX, (int)PS_SEARCH_LDS_PER_LANE, pool_cap, false, cus, bt_blocks, PS_SEARCH_WAVES, n_big);
}

// ragged launch: the budget (in units) of a read of every length 0..255
inline void budget_units_by_len(const Options &o, uint8_t tab[256])
{
    for (int l = 0; l < 256; ++l) { const int u = budget_diffs(o, l) * (o.profile ? o.unit : 1); tab[l] = (uint8_t)(u > 255 ? 255 : u); }
}

}  // namespace ps
