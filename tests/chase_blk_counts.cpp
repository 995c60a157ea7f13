// chase_blk_counts.cpp -- TEST HARNESS ONLY (tests/test_chase_cpu.py builds it with the host compiler).
// The three prefix counts of an Occ block (16 words: running counts, low plane, high plane) at r = 0..192: every symbol by
// blk_count4b, and each symbol alone by blk_count1 (ps_core.h) and blk_count1b (ps_narrow.h: the chase's).
#include "../para-suite_amd/csrc/ps_core.h"
#include "../para-suite_amd/csrc/ps_narrow.h"
using namespace ps;

extern "C" void cb_blk_counts(const uint32_t *words, int r, uint32_t out4[4], uint32_t out1[4], uint32_t out1b[4])
{
    Blk b; for (int j = 0; j < 16; ++j) b.x[j] = words[j];
    blk_count4b(b, r, out4);
    for (int c = 0; c < 4; ++c) { out1[c] = blk_count1(b, r, c); out1b[c] = blk_count1b(b, r, c); }
}
