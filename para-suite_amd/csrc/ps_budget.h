// ps_budget.h -- what a kernel may ask for if it is to start BESIDE a resident first-tier search launch.
//
// Two batches are in flight per device: while one batch's search launch (k_backtrack_n, persistent, every CU full) runs,
// the other batch goes through selection, locate and the preparation of its next search on a stream of its own.  A kernel
// of that stream whose workgroup does not fit into what the search launch leaves on a CU is not started until the launch
// drains -- a second or so for a stage that takes milliseconds.  What is left, from the search kernel's own numbers:
//
//   registers  a SIMD holds 512 VGPRs per lane; the search kernel is compiled for PS_SEARCH_WAVES = 4 waves per SIMD
//              (ps_kernels.hip, PS_BT_WAVES) and is allocated 112 of them (111 used, granule 8): 512 - 4 x 112 = 64;
//              4 of a SIMD's 8 wave slots stay free.
//   LDS        a CU holds 163,840 B; a first-tier launch keeps 4 workgroups x 256 lanes x lm_bytes(50, 32, 25) = 156 B
//              there (50-bp reads, 32-base seed, 25 score buckets: the profile-cost flagship), 159,744 B: 4,096 B are
//              left on paper -- and none if the hardware rounds a workgroup's 39,936 B up to a coarser allocation unit.
//              The stage kernels therefore use NO LDS, static or dynamic (every launch wrapper passes 0): PS_STAGE_LDS is the
//              bound on paper, 0 what the test asserts.
//
// tests/test_stage_budget_cpu.py compiles the device code with the resource remark and holds every stage kernel to
// these two numbers, and the numbers to the search kernel's allocation and to lm_bytes().
#pragma once
#include <cstddef>

namespace ps {

static const int PS_SIMD_VGPRS = 512;              // per lane, wave64, gfx950
static const int PS_SEARCH_WAVES = 4;              // resident waves per SIMD of the narrow search kernel
static const int PS_SEARCH_VGPRS = 112;            // its allocation (k_backtrack_n<false, true>)
static const int PS_STAGE_VGPRS = PS_SIMD_VGPRS - PS_SEARCH_WAVES * PS_SEARCH_VGPRS;                      // 64

static const size_t PS_CU_LDS = 160 * 1024;
static const size_t PS_SEARCH_LDS_PER_LANE = 156;  // lm_bytes(50, 32, 25, false)
static const size_t PS_STAGE_LDS = PS_CU_LDS - (size_t)PS_SEARCH_WAVES * 256 * PS_SEARCH_LDS_PER_LANE;    // 4,096

static const int PS_SORT_MAX_WG = 2048;            // chunks (one wave each) of the hand-out order's counting sort (ps_stage.hip)

}  // namespace ps
