// bwa_args.h -- the command lines of the `bwa` shim (bwa_shim.cpp) and the .sai stub that carries `aln`'s arguments to `samse`.
// Header only, no HIP and no call into the library: the CPU test tier compiles it on its own.
//
// `aln` / `parasuite` take upstream's search options -o -e -i -d -l -k -m -M -O -E -R (ps_search_opts) besides -t -n/-X -p -g -f,
// `samse` takes -n and -f.  Options upstream has and this library cannot honour are refused by name -- an aligner that maps with
// other parameters than the ones it was given is no drop-in: -q above 0 (read trimming), -N, -B, -b -0 -1 -2 (BAM input), -c, -I,
// -L, -Y, and samse -r.  So is anything unknown.
#pragma once
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <istream>
#include <sstream>
#include <string>
#include <vector>
#include "ps_search_opts.h"

namespace bwa_args {

static const char *const SAI_MAGIC_1 = "PSSAI1";     // before the search options: read with the defaults
static const char *const SAI_MAGIC_2 = "PSSAI2";     // + one line with the eleven `aln` search options

struct Aln {
    std::string threads = "1", mm, ep, ip, out;
    std::vector<std::string> pos;                    // <ref> <reads>
    ps_search_opts search;
    Aln() { ps::search_opts_default(search); }
};
struct Samse {
    std::string out;
    std::vector<std::string> pos;                    // <ref> <in.sai> <reads>
    bool have_n = false; int n_alt = 3;              // -n: max_alt_hits
};
struct Sai {                                         // what `aln` left for `samse`
    std::string sub, threads, mm, ep, ip, ref, fq;
    ps_search_opts search;                           // max_alt_hits: the default, samse's -n sets it
    Sai() { ps::search_opts_default(search); }
};

inline bool to_int(const std::string &s, int &v)
{
    if (s.empty()) return false;
    char *end = nullptr; errno = 0;
    const long x = std::strtol(s.c_str(), &end, 10);
    if (errno || *end || x < INT_MIN || x > INT_MAX) return false;
    v = (int)x;
    return true;
}

// argv[2..] of `bwa aln` (cmd "aln") or `bwa parasuite`.  false: err is the message for stderr
inline bool parse_aln(const std::string &cmd, int argc, const char *const *argv, Aln &a, std::string &err)
{
    a = Aln();
    a.mm = cmd == "aln" ? "0.04" : "-1";
    const std::string who = "[bwa " + cmd + "] ";
    struct IntOpt { const char *flag; int32_t *dst; };
    const IntOpt ints[] = {{"-o", &a.search.max_gap_opens}, {"-e", &a.search.max_gap_extensions}, {"-i", &a.search.indel_end_skip},
                           {"-d", &a.search.max_del_occ}, {"-l", &a.search.seed_len}, {"-k", &a.search.max_seed_diff},
                           {"-m", &a.search.max_entries}, {"-M", &a.search.s_mm}, {"-O", &a.search.s_gapo}, {"-E", &a.search.s_gape},
                           {"-R", &a.search.max_top2}};
    static const char *const refused_flag[] = {"-N", "-b", "-0", "-1", "-2", "-c", "-I", "-L", "-Y"};
    for (int i = 2; i < argc; ++i) {
        const std::string o = argv[i];
        auto val = [&](std::string &dst) { if (i + 1 >= argc) { err = who + "option " + o + " needs a value"; return false; } dst = argv[++i]; return true; };
        std::string *text = o == "-t" ? &a.threads : (o == "-n" || o == "-X") ? &a.mm : o == "-p" ? &a.ep : o == "-g" ? &a.ip : o == "-f" ? &a.out : nullptr;
        if (text) { if (!val(*text)) return false; continue; }
        const IntOpt *io = nullptr;
        for (const IntOpt &c : ints) if (o == c.flag) io = &c;
        if (io) {
            std::string v; int x = 0;
            if (!val(v)) return false;
            if (!to_int(v, x)) { err = who + "option " + o + " needs an integer, got '" + v + "'"; return false; }
            *io->dst = x;
            continue;
        }
        if (o == "-q") {                             // read trimming: 0 is "none", which is what the library does
            std::string v; int x = 0;
            if (!val(v)) return false;
            if (!to_int(v, x)) { err = who + "option -q needs an integer, got '" + v + "'"; return false; }
            if (x > 0) { err = who + "option -q " + v + " is not supported: parasuite-hip does not trim reads (only -q 0)"; return false; }
            continue;
        }
        if (o == "-B") { err = who + "option -B is not supported: parasuite-hip reads no barcodes"; return false; }
        bool refused = false;
        for (const char *f : refused_flag) refused = refused || o == f;
        if (refused) { err = who + "option " + o + " is not supported by parasuite-hip"; return false; }
        if (o.size() > 1 && o[0] == '-') { err = who + "unknown option " + o; return false; }
        a.pos.push_back(o);
    }
    if (a.pos.size() != 2 || a.out.empty()) { err = who + "need <ref> <reads> -f <out.sai>"; return false; }
    if (cmd == "parasuite" && a.ep.empty()) { err = "[bwa parasuite] -p <error profile> is required"; return false; }
    return true;
}

inline std::string sai_text(const std::string &cmd, const Aln &a)
{
    const ps_search_opts &s = a.search;
    std::ostringstream f;
    f << SAI_MAGIC_2 << '\n' << cmd << '\n' << a.threads << '\n' << a.mm << '\n' << a.ep << '\n' << a.ip << '\n' << a.pos[0] << '\n' << a.pos[1] << '\n'
      << s.max_gap_opens << ' ' << s.max_gap_extensions << ' ' << s.indel_end_skip << ' ' << s.max_del_occ << ' ' << s.seed_len << ' ' << s.max_seed_diff << ' '
      << s.max_entries << ' ' << s.s_mm << ' ' << s.s_gapo << ' ' << s.s_gape << ' ' << s.max_top2 << '\n';
    return f.str();
}

inline bool read_sai(std::istream &f, const std::string &path, Sai &s, std::string &err)
{
    s = Sai();
    std::string magic;
    std::getline(f, magic); std::getline(f, s.sub); std::getline(f, s.threads); std::getline(f, s.mm);
    std::getline(f, s.ep); std::getline(f, s.ip); std::getline(f, s.ref); std::getline(f, s.fq);
    if (magic == SAI_MAGIC_1) return true;
    if (magic != SAI_MAGIC_2) { err = "[bwa samse] " + path + " was not written by this bwa"; return false; }
    ps_search_opts &o = s.search;
    int32_t *dst[11] = {&o.max_gap_opens, &o.max_gap_extensions, &o.indel_end_skip, &o.max_del_occ, &o.seed_len, &o.max_seed_diff,
                        &o.max_entries, &o.s_mm, &o.s_gapo, &o.s_gape, &o.max_top2};
    std::string line, tok;
    std::getline(f, line);
    std::istringstream ls(line);
    for (int32_t *d : dst) {
        int x = 0;
        if (!(ls >> tok) || !to_int(tok, x)) { err = "[bwa samse] " + path + ": the line of search options is damaged"; return false; }
        *d = x;
    }
    return true;
}

// argv[2..] of `bwa samse`
inline bool parse_samse(int argc, const char *const *argv, Samse &a, std::string &err)
{
    a = Samse();
    for (int i = 2; i < argc; ++i) {
        const std::string o = argv[i];
        if (o == "-f" || o == "-n" || o == "-r") {
            if (i + 1 >= argc) { err = "[bwa samse] option " + o + " needs a value"; return false; }
            const std::string v = argv[++i];
            if (o == "-f") a.out = v;
            else if (o == "-r") { err = "[bwa samse] option -r is not supported: parasuite-hip writes no read group"; return false; }
            else if (!to_int(v, a.n_alt)) { err = "[bwa samse] option -n needs an integer, got '" + v + "'"; return false; }
            else a.have_n = true;
        }
        else if (o.size() > 1 && o[0] == '-') { err = "[bwa samse] unknown option " + o; return false; }
        else a.pos.push_back(o);
    }
    if (a.pos.size() != 3 || a.out.empty()) { err = "[bwa samse] need <ref> <in.sai> <reads> -f <out.sam>"; return false; }
    return true;
}

}  // namespace bwa_args
