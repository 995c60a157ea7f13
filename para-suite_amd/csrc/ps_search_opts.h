// ps_search_opts.h -- the public ps_search_opts (include/parasuite_hip.h) as the search part of a context's options (ps_model.h):
// defaults, the range check and the conversion.  Header only, no HIP and no call into the library: the `bwa` shim and the CPU test
// tier compile it on their own.
#pragma once
#include "../../include/parasuite_hip.h"
#include "ps_model.h"

namespace ps {

inline void search_opts_default(ps_search_opts &s)
{
    s.struct_size = (uint32_t)sizeof(ps_search_opts);
    s.max_gap_opens = 1; s.max_gap_extensions = -1; s.indel_end_skip = 5; s.max_del_occ = 10;
    s.seed_len = 32; s.max_seed_diff = 2; s.max_entries = 2000000;
    s.s_mm = 3; s.s_gapo = 11; s.s_gape = 4; s.max_top2 = 30; s.max_alt_hits = 3;
}
// the caller's struct as this library's: the fields behind the caller's struct_size keep their defaults.  false: a size that is no
// whole number of fields, or one larger than this library knows (options it would have to ignore)
inline bool search_opts_read(const ps_search_opts *in, ps_search_opts &s, std::string &err)
{
    search_opts_default(s);
    if (!in) return true;
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz % sizeof(int32_t) != 0 || sz > sizeof(ps_search_opts)) {
        err = "ps_search_opts: struct_size " + std::to_string(sz) + " must be a multiple of 4 from 4 to " + std::to_string(sizeof(ps_search_opts));
        return false;
    }
    std::memcpy(&s, in, sz);
    s.struct_size = (uint32_t)sizeof(ps_search_opts);
    return true;
}
// The accepted ranges: a value is taken where the result is exactly upstream's rule, anything else is refused here, before any launch,
// with the field and its limit.  What also depends on -n / -X and the read length (the number of score buckets) is make_model's.
inline bool search_opts_check(const ps_search_opts *in, bool profile_mode, std::string &err)
{
    ps_search_opts s;
    if (!search_opts_read(in, s, err)) return false;
    const long long ANY = 0x7fffffffLL;
    auto range = [&](const char *field, const char *flag, long long v, long long lo, long long hi) {
        if (v >= lo && v <= hi) return true;
        err = std::string("ps_search_opts: ") + field + " (" + flag + ") is " + std::to_string(v) + ", accepted: " +
              (lo < -ANY ? "at most " + std::to_string(hi) : std::to_string(lo) + (hi == ANY ? std::string(" and up") : " to " + std::to_string(hi)));
        return false;
    };
    const int k_max = 4095 / (profile_mode ? 8 : 1);                   // max_seed_diff * u_tight in the header's 12 bits; profile costs count a difference as 8 units
    return range("max_gap_opens", "aln -o", s.max_gap_opens, 0, PS_MAX_GAPO) &&
           range("max_gap_extensions", "aln -e", s.max_gap_extensions, -ANY - 1, PS_MAX_GAPE) &&
           range("indel_end_skip", "aln -i", s.indel_end_skip, 0, ANY) &&
           range("max_del_occ", "aln -d", s.max_del_occ, 0, 255) &&
           range("seed_len", "aln -l", s.seed_len, 1, ANY) &&
           range("max_seed_diff", "aln -k", s.max_seed_diff, 0, k_max) &&
           range("max_entries", "aln -m", s.max_entries, 1, PS_MAX_ENTRIES) &&
           range("s_mm", "aln -M", s.s_mm, 0, 255) && range("s_gapo", "aln -O", s.s_gapo, 0, 255) && range("s_gape", "aln -E", s.s_gape, 0, 255) &&
           range("max_top2", "aln -R", s.max_top2, 0, ANY) &&
           range("max_alt_hits", "samse -n", s.max_alt_hits, 0, ANY);
}
// checked options -> the search part.  -e: below 1 is upstream's k-difference mode (6 extensions, each a difference), from 1 on that many
// extensions that do not count as differences.  -i: no read is longer than PS_MAX_LEN = 250, so 255 and everything above mean "no gap"
inline SearchPart search_part_of(const ps_search_opts &s)
{
    SearchPart p;
    p.max_gapo = s.max_gap_opens;
    if (s.max_gap_extensions >= 1) { p.max_gape = s.max_gap_extensions; p.mode_gape = 0; } else { p.max_gape = 6; p.mode_gape = 1; }
    p.indel_end_skip = s.indel_end_skip > 255 ? 255 : s.indel_end_skip;
    p.max_del_occ = s.max_del_occ; p.max_entries = s.max_entries;
    p.seed_len = s.seed_len; p.max_seed_diff = s.max_seed_diff; p.max_top2 = s.max_top2;
    p.s_mm = s.s_mm; p.s_gapo = s.s_gapo; p.s_gape = s.s_gape;
    p.n_occ = s.max_alt_hits;
    return p;
}
// NULL: the defaults.  false: err names the field and its limit
inline bool search_part_from(const ps_search_opts *in, bool profile_mode, SearchPart &p, std::string &err)
{
    ps_search_opts s;
    if (!search_opts_check(in, profile_mode, err) || !search_opts_read(in, s, err)) return false;
    p = search_part_of(s);
    return true;
}
// the context's search part from the caller's struct (NULL: the defaults), checked under the cost part in force
inline bool set_search(OptionParts &parts, const ps_search_opts *in, std::string &err)
{
    SearchPart p;
    if (!search_part_from(in, parts.opt.profile != 0, p, err)) return false;
    parts.set_search(p);
    return true;
}

}  // namespace ps
