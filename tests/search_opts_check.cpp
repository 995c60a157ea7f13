// search_opts_check.cpp -- the host-only pieces behind ps_search_opts as a plain executable (tests/test_search_opts_cpu.py builds it
// with the host compiler, AddressSanitizer and UBSan): the product's conversion ps_search_opts -> Options -> Model (csrc/ps_search_opts.h, ps_model.h),
// the merge of a context's two option parts, and the `bwa` shim's command lines and .sai stub (csrc/bwa_args.h).
//
//   models            stdin, one case per line: stock|profile len cost_arg struct_size f1 .. f12 [P0 .. P15 ins del]
//                     -> "ok wide <hex of the Model>" or "error <message>"   (cost_arg: -n's text, or -X's number)
//   order             stdin, the same lines -> the merged options after search,cost and after cost,search, one line each
//   aln|parasuite ... the shim's argv -> "ok" and the .sai stub it would write, or "error <message>"
//   samse ...         the shim's argv -> "ok out=.. n=.. have_n=.. pos=..|..|.." or "error <message>"
//   sai               stdin: a stub -> "ok sub=.. threads=.. mm=.. ep=.. ip=.. ref=.. fq=.. search=<12 fields>" or "error <message>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "ps_search_opts.h"
#include "bwa_args.h"

using namespace ps;

struct Case { bool profile = false; int len = 0; std::string cost_arg; ps_search_opts so; double P[16], ins = 0, del = 0; };

static bool read_case(const std::string &line, Case &c)
{
    std::istringstream in(line);
    std::string mode;
    if (!(in >> mode >> c.len >> c.cost_arg >> c.so.struct_size)) return false;
    c.profile = mode == "profile";
    int32_t *f[12] = {&c.so.max_gap_opens, &c.so.max_gap_extensions, &c.so.indel_end_skip, &c.so.max_del_occ, &c.so.seed_len, &c.so.max_seed_diff,
                      &c.so.max_entries, &c.so.s_mm, &c.so.s_gapo, &c.so.s_gape, &c.so.max_top2, &c.so.max_alt_hits};
    for (int32_t *p : f) if (!(in >> *p)) return false;
    if (c.profile) { for (double &p : c.P) if (!(in >> p)) return false; if (!(in >> c.ins >> c.del)) return false; }
    return true;
}
static Options cost_of(const Case &c)
{
    Options o;
    if (c.profile) profile_costs(o, c.P, c.ins, c.del, std::atoi(c.cost_arg.c_str())); else set_stock_n(o, c.cost_arg.c_str());
    return o;
}
static std::string fields(const Options &o)
{
    std::ostringstream s;
    s << o.max_diff << ' ' << o.fnr << ' ' << o.profile << ' ' << o.x_avg_mm << " | " << o.max_gapo << ' ' << o.max_gape << ' ' << o.mode_gape << ' ' << o.indel_end_skip << ' '
      << o.max_del_occ << ' ' << o.max_entries << ' ' << o.seed_len << ' ' << o.max_seed_diff << ' ' << o.max_top2 << ' ' << o.s_mm << ' ' << o.s_gapo << ' ' << o.s_gape << ' ' << o.n_occ;
    return s.str();
}
static std::string search_fields(const ps_search_opts &s)
{
    std::ostringstream o;
    o << s.max_gap_opens << ' ' << s.max_gap_extensions << ' ' << s.indel_end_skip << ' ' << s.max_del_occ << ' ' << s.seed_len << ' ' << s.max_seed_diff << ' '
      << s.max_entries << ' ' << s.s_mm << ' ' << s.s_gapo << ' ' << s.s_gape << ' ' << s.max_top2 << ' ' << s.max_alt_hits;
    return o.str();
}

static int run_models()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        Case c; std::string err;
        if (!read_case(line, c)) { std::printf("error bad case line\n"); continue; }
        OptionParts parts;
        Model m;
        if (!parts.set_cost(cost_of(c), err) || !set_search(parts, &c.so, err) || !make_model(parts.opt, c.len, m, err)) { std::printf("error %s\n", err.c_str()); continue; }
        std::printf("ok %d ", launch_is_wide(m, 16384) ? 1 : 0);
        const unsigned char *b = reinterpret_cast<const unsigned char *>(&m);
        for (size_t j = 0; j < sizeof m; ++j) std::printf("%02x", b[j]);
        std::printf("\n");
    }
    return 0;
}
static int run_order()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        Case c; std::string e1, e2;
        if (!read_case(line, c)) { std::printf("error bad case line\n"); continue; }
        OptionParts a, b;
        const bool ok_a = set_search(a, &c.so, e1) && a.set_cost(cost_of(c), e1);
        const bool ok_b = b.set_cost(cost_of(c), e2) && set_search(b, &c.so, e2);
        std::printf("%s\n%s\n", ok_a ? fields(a.opt).c_str() : ("error " + e1).c_str(), ok_b ? fields(b.opt).c_str() : ("error " + e2).c_str());
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    std::string err;
    if (cmd == "models") return run_models();
    if (cmd == "order") return run_order();
    if (cmd == "aln" || cmd == "parasuite") {
        bwa_args::Aln a;
        if (!bwa_args::parse_aln(cmd, argc, argv, a, err)) { std::printf("error %s\n", err.c_str()); return 0; }
        std::printf("ok\n%s", bwa_args::sai_text(cmd, a).c_str());
        return 0;
    }
    if (cmd == "samse") {
        bwa_args::Samse a;
        if (!bwa_args::parse_samse(argc, argv, a, err)) { std::printf("error %s\n", err.c_str()); return 0; }
        std::printf("ok out=%s n=%d have_n=%d pos=%s|%s|%s\n", a.out.c_str(), a.n_alt, a.have_n ? 1 : 0, a.pos[0].c_str(), a.pos[1].c_str(), a.pos[2].c_str());
        return 0;
    }
    if (cmd == "sai") {
        bwa_args::Sai s;
        if (!bwa_args::read_sai(std::cin, "in.sai", s, err)) { std::printf("error %s\n", err.c_str()); return 0; }
        std::printf("ok sub=%s threads=%s mm=%s ep=%s ip=%s ref=%s fq=%s search=%s\n", s.sub.c_str(), s.threads.c_str(), s.mm.c_str(), s.ep.c_str(), s.ip.c_str(),
                    s.ref.c_str(), s.fq.c_str(), search_fields(s.search).c_str());
        return 0;
    }
    return 2;
}
