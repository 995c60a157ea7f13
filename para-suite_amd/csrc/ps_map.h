// ps_map.h -- the whole `map` step behind one call (ps_map.hip): the streaming pass and the route made of several.  Everything
// here throws ps::Error; the status codes are ps_capi.hip's.
#pragma once
#include <thread>
#include "ps_pipeline.h"

namespace ps {

// Threads that free what a call leaves behind (written pieces, closed contexts): the call does not wait for the last of them.
// They are joined by the next pass, by ps_release_host_cache and when the process exits.
void trash_add(std::thread &&t);
void trash_collect();

static const char *const PS_PG_LINE = "@PG\tID:parasuite-hip\tPN:parasuite-hip\tVN:0.1";

struct MapArgs { int threads; const char *mm, *error_profile, *indel_profile, *ref_fa, *reads; const ps_search_opts *search = nullptr; };    // what every mapping call is given (search: ps_map_opts and ps_map_route_opts; null: the defaults)
void map_to_sam(const MapArgs &a, const char *out_sam);
void map_profiled(const MapArgs &a, const char *out_sam, int min_mapq, int max_read_len, const char *profile_prefix);
void map_to_bam(const MapArgs &a, const char *out_bam, int min_mapq, bool sort_by_coordinate, bool write_index, BamStats *stats);
void map_route(const ps_route_opts *o, ps_route_stats *stats_out);
void map_route_opts(const ps_route_opts2 *o, ps_route_stats *stats_out);       // the same with --ref-refine, --unaligned and the search options

// The resident scope (ps_resident.h keeps the books, ps_map.hip the contexts): between begin and end the four calls above take
// their contexts from the scope's entries and leave them open.  begin makes no device call.
void resident_begin(const ps_resident_opts *o);
void resident_end();
void resident_info(ps_resident_stats &out);
void resident_invalidate(const char *ref_fa);      // ps_index is about to write the index files of ref_fa: its entries are closed

}  // namespace ps
