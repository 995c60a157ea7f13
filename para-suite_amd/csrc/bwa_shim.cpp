// bwa_shim.cpp -- an executable named `bwa` that accepts exactly the command lines the reference emits
// and forwards them to libparasuite_hip.so, so that the UNMODIFIED parasuite.jar drives the GPU path after
// `parasuite setup --parasuite <dir of this binary>` (Main.java:649-654; PARAsuiteMapping.java:35-41).
//
//   bwa index <ref>                                              PARAsuiteMapping.java:48-53
//   bwa parasuite -t T -X mm -p EP -g IP <ref> <fq> -f P.sai     PARAsuiteMapping.java:63-77
//   bwa aln -t T -n mm <ref> <fq> -f P.sai                       BWAMapping.java:51-61
//   bwa samse <ref> P.sai <fq> -f P.sam                          PARAsuiteMapping.java:85-92
// and, beyond those, upstream's search options of `aln` (-o -e -i -d -l -k -m -M -O -E -R) and `samse -n`; what upstream has and
// the library cannot honour is refused by name (bwa_args.h).
//
// Seeding and SAM generation are fused in the library, so `parasuite`/`aln` only record their arguments in
// the .sai file (a text stub only this shim reads; the Java deletes it afterwards, PARAsuiteMapping.java:135-138)
// and `samse` does the work.  Exit status 0/1 and messages on stderr are what Mapping.executeCommand expects
// (Mapping.java:167-172).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "../../include/parasuite_hip.h"
#include "bwa_args.h"

static int usage()
{
    std::fprintf(stderr, "Program: bwa (parasuite-hip shim, %s)\nUsage: bwa index|aln|parasuite|samse ...\n", ps_version());
    return 1;
}

int main(int argc, char **argv)
{
    if (argc < 2) return usage();
    const std::string cmd = argv[1];
    if (cmd == "index") {
        if (argc < 3) return usage();
        return ps_index(argv[argc - 1]) ? 1 : 0;
    }
    if (cmd == "aln" || cmd == "parasuite") {
        bwa_args::Aln a; std::string err;
        if (!bwa_args::parse_aln(cmd, argc, argv, a, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        if (ps_search_opts_check(&a.search, cmd == "parasuite")) return 1;        // out of range: the library has named the field and its limit
        std::ofstream f(a.out);
        f << bwa_args::sai_text(cmd, a);
        return f.good() ? 0 : 1;
    }
    if (cmd == "samse") {
        bwa_args::Samse a; bwa_args::Sai s; std::string err;
        if (!bwa_args::parse_samse(argc, argv, a, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        std::ifstream f(a.pos[1]);
        if (!bwa_args::read_sai(f, a.pos[1], s, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
        if (s.ref != a.pos[0] || s.fq != a.pos[2]) { std::fprintf(stderr, "[bwa samse] reference/reads differ from the ones given to `bwa %s`\n", s.sub.c_str()); return 1; }
        if (a.have_n) s.search.max_alt_hits = a.n_alt;
        const bool profile = s.sub == "parasuite";
        return ps_map_opts(std::atoi(s.threads.c_str()), s.mm.c_str(), profile ? s.ep.c_str() : nullptr, profile ? s.ip.c_str() : nullptr,
                           s.ref.c_str(), s.fq.c_str(), a.out.c_str(), &s.search) ? 1 : 0;
    }
    return usage();
}
