// parasuite_args.h -- the command lines of `parasuite` (parasuite_cli.cpp): the argv of `java -jar parasuite.jar <mode> ...`
// (src/src/main/Main.java) turned into a plain plan -- the mode, the fields of the ONE library call to make, or the text of a
// usage error.  Header only, no HIP and no call into the library: the CPU test tier compiles it on its own.
//
// The rules are Main.java's as it is written, flag for flag (INTEGRATION.md section M has the table and the deviations): numbers go
// through Integer.parseInt, Boolean.parseBoolean and Double.parseDouble (ps_java.h); what the Java answers with a help text and
// exit 1 is a usage error here.  The banner, the log4j file <prefix>.log and the help texts are not reproduced.
#pragma once
#include <string>
#include <vector>
#include "ps_java.h"

namespace parasuite_args {

enum Call { kUsage, kNotice, kMapRoute, kCombine, kBenchmark, kErrorProfile, kClusters, kSimulate, kExtractWeak, kExtractNames, kFetch };
inline const char *call_name(Call c)
{
    static const char *const n[] = {"usage", "notice", "ps_map_route_opts", "ps_combine_genome_transcript", "ps_benchmark_reads", "ps_error_profile_full",
                                    "ps_pileup_clusters", "ps_simulate_reads", "ps_extract_weak_reads", "ps_extract_read_names", "ps_fetch_sequences"};
    return n[c];
}

struct Plan {
    Call call = kUsage;                    // kUsage: `text` to stderr, exit 1.  kNotice: `text` to stderr, exit 0.  Else the call below
    std::string mode, text;
    std::vector<std::string> notes;        // lines for stderr before the call is made
    // map
    std::string reads, ref, ref_refine, out_prefix, transcripts, error_profile, indel_profile;
    std::string bwa_mm = "2", parasuite_mm = "-1", bt_mm = "1", user_command;      // bt_mm, user_command: parsed and unused
    int32_t threads = 1, max_read_len = 101, mapq_genomic = 10, mapq_transcript = 1;
    bool refine = false, keep_unaligned = false;
    // the other modes: `mapping` is the SAM or BAM a mode reads, `out` the file (or prefix) it writes
    std::string mapping, out, genome_bam, transcript_bam, reads_fq, snp_vcf, sites;
    int32_t min_coverage = 0, mapq_threshold = 10;
    bool infer_qualities = false, bed = false, have_seed = false;
    uint64_t seed = 0;
    std::string t2c_profile, t2c_positions, quality_dist;     // simulate; its error and indel profile are the two above
    double bound_prob = 0;
};

inline const char *modes_text()
{
    return "usage: parasuite <mode> ...\n"
           "  map            -q READS -r REF -o PREFIX [-t TRANSCRIPTS] [-p THREADS] [-l MAXLEN] [--gm Q] [--tm Q] [--refine] [--ref-refine REF]\n"
           "                 [--unaligned] [--mode BWA] [--bwa-mm N] [--parasuite-mm X] [--parasuite-ep PROFILE --parasuite-indel PROFILE]\n"
           "  comb           -g GENOMIC.bam -t TRANSCRIPT.bam -o OUT.bam\n"
           "  benchmark      MAPPING OUT.stats READS.fastq [--only-bound]\n"
           "  error          MAPPING REF MAXLEN [-q true|false] [-p true|false]\n"
           "  clust          MAPPING REF OUT SNP_VCF MIN_COVERAGE\n"
           "  simulate       TRANSCRIPTS OUT_PREFIX ERROR_PROFILE T2C_PROFILE T2C_POSITIONS QUALITIES INDELS RBP_BOUND [-I path] [--seed N]\n"
           "  setup          --parasuite|--bwa|--bt2|--bowtie PATH\n"
           "  extract        -i BAM -o FASTQ [-t MAPQ]\n"
           "  extractAligned -a BAM -o OUT\n"
           "  fetch          -i SITES -r REF -o OUT\n"
           "  fetchBed       -i SITES.bed -r REF -o OUT\n"
           "  benchmarkClusters is not built\n";
}
inline std::string mode_usage(const std::string &mode)     // the line(s) of modes_text() that belong to a mode
{
    const std::string all = modes_text(), key = "  " + mode + " ";
    const size_t at = all.find(key);
    if (at == std::string::npos) return all;
    size_t end = all.find('\n', at);
    while (end != std::string::npos && all.compare(end + 1, 17, "                 ") == 0) end = all.find('\n', end + 1);
    return "usage: parasuite" + all.substr(at + 1, end - at);
}

// argv[1..] as Main.main sees its args.  Never fails: what is wrong with a command line is a kUsage plan
inline Plan parse(int argc, const char *const *argv)
{
    std::vector<std::string> a;
    for (int i = 1; i < argc; ++i) a.push_back(argv[i]);
    Plan p;
    auto usage = [&](const std::string &msg) { p.call = kUsage; p.text = (msg.empty() ? std::string() : "parasuite " + p.mode + ": " + msg + "\n") + mode_usage(p.mode); return p; };
    if (a.empty() || a[0] == "-h" || a[0] == "--help") { p.text = modes_text(); return p; }      // Main.java:45-50
    p.mode = a[0];
    static const char *const modes[] = {"map", "comb", "benchmark", "error", "clust", "simulate", "setup", "extract", "extractAligned", "benchmarkClusters", "fetch", "fetchBed"};
    bool known = false;
    for (const char *m : modes) known = known || p.mode == m;
    if (!known) { p.text = "parasuite: program mode \"" + p.mode + "\" is not known\n" + modes_text(); return p; }
    if (p.mode == "benchmarkClusters") {
        p.text = "parasuite benchmarkClusters: not built: it reads column 15 of a cluster table that `clust` writes with 12 columns\n";
        return p;
    }
    if (a.size() == 1) return usage("");
    const size_t n = a.size();
    int32_t v = 0;

    if (p.mode == "map") {                 // Main.java:131-247
        bool mode_ok = true; std::string mode_text = "BWA";
        for (size_t i = 1; i < n; ++i) {
            const std::string &f = a[i];
            if (f == "--refine") { p.refine = true; continue; }
            if (f == "--unaligned") { p.keep_unaligned = true; continue; }
            std::string *text = f == "-q" ? &p.reads : f == "-t" ? &p.transcripts : f == "-o" ? &p.out_prefix : f == "--parasuite-mm" ? &p.parasuite_mm :
                                f == "--parasuite-ep" ? &p.error_profile : f == "--parasuite-indel" ? &p.indel_profile : f == "--bwa-mm" ? &p.bwa_mm :
                                f == "--bt-mm" ? &p.bt_mm : f == "-c" ? &p.user_command : f == "--ref-refine" ? &p.ref_refine : f == "--mode" ? &mode_text : nullptr;
            int32_t *num = f == "-p" ? &p.threads : f == "-l" ? &p.max_read_len : f == "--gm" ? &p.mapq_genomic : f == "--tm" ? &p.mapq_transcript : nullptr;
            if (!text && !num && f != "-r") return usage("parameter not found: " + f);
            if (i + 1 >= n) return usage("option " + f + " needs a value");
            const std::string &val = a[++i];
            if (f == "-r") { p.ref = val; p.ref_refine = val; }              // :141: -r sets both, so a --ref-refine before it is lost
            else if (text) *text = val;
            else if (!ps::java_parse_int(val, v)) return usage("option " + f + " needs an integer, got '" + val + "'");
            else *num = v;
            if (f == "--mode") {           // :171-188: the upper-cased text must name a mapper; the RAW text is what is compared later (:262-282)
                std::string up = val;
                for (char &c : up) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
                mode_ok = up == "BT" || up == "BT2" || up == "BWA" || up == "USER";      // "PARASUITE" never equals "PARAsuite" 
                if (!mode_ok) return usage("wrong mapping mode '" + val + "': choose one of bt, bt2, bwa, user");
            }
        }
        if (p.reads.empty() || p.out_prefix.empty() || p.ref.empty()) return usage("no valid argument for -q, -r or -o");
        if (mode_text == "BT" || mode_text == "BT2" || mode_text == "USER") { p.text = "parasuite map: the " + mode_text + " mapper stays with the Java toolkit; this command maps with --mode BWA\n"; return p; }
        if (mode_text != "BWA") { p.text = "parasuite map: mapping mode not set: '" + mode_text + "' names no mapper as it is spelled (--mode BWA)\n"; return p; }
        p.call = kMapRoute;
        return p;
    }
    if (p.mode == "comb") {                // :449-470
        for (size_t i = 1; i < n; ++i) {
            std::string *text = a[i] == "-g" ? &p.genome_bam : a[i] == "-t" ? &p.transcript_bam : a[i] == "-o" ? &p.out : nullptr;
            if (!text) return usage("parameter not found: " + a[i]);
            if (i + 1 >= n) return usage("option " + a[i] + " needs a value");
            *text = a[++i];
        }
        if (p.genome_bam.empty() || p.transcript_bam.empty() || p.out.empty()) return usage("-g, -t and -o are required");
        p.call = kCombine;
        return p;
    }
    if (p.mode == "benchmark") {           // :497-521: a fourth argument (--only-bound) is read and never used
        if (n < 4) return usage("wrong number of input files");
        p.mapping = a[1]; p.out = a[2]; p.reads_fq = a[3];
        p.call = kBenchmark;
        return p;
    }
    if (p.mode == "error") {               // :560-593
        if (n < 4) return usage("wrong number of input files");
        p.mapping = a[1]; p.ref = a[2];
        if (!ps::java_parse_int(a[3], v)) return usage("MAX_READ_LENGTH is not a number: '" + a[3] + "'");
        p.max_read_len = v;
        for (size_t i = 4; i < n; ++i) {
            if (a[i] == "-q" || a[i] == "-p") {
                if (i + 1 >= n) return usage("wrong number of input files");
                const bool b = ps::java_parse_boolean(a[i + 1]);
                if (a[i] == "-q") p.infer_qualities = b;
                else if (b) p.notes.push_back("parasuite error: -p true: no plot is drawn");
                ++i;
            } else p.notes.push_back("parasuite error: parameter \"" + a[i] + "\" not found, skipped");     // :578-581
        }
        p.call = kErrorProfile;
        return p;
    }
    if (p.mode == "clust") {               // :610-639
        if (n < 6) return usage("wrong number of input files");
        p.mapping = a[1]; p.ref = a[2]; p.out = a[3]; p.snp_vcf = a[4];
        if (!ps::java_parse_int(a[5], v)) return usage("MIN_COVERAGE is not a number: '" + a[5] + "'");
        p.min_coverage = v;
        p.call = kClusters;
        return p;
    }
    if (p.mode == "simulate") {            // :687-727.  Arguments 6 and 7: the quality file, then the indel file, as the Perl reads them
        if (n < 9) return usage("wrong number of arguments");
        for (size_t i = 1; i <= 8; ++i) if (!a[i].empty() && a[i][0] == '-') return usage("argument " + std::to_string(i) + " starts with '-': " + a[i]);
        p.reads_fq = a[1]; p.out = a[2]; p.error_profile = a[3]; p.t2c_profile = a[4]; p.t2c_positions = a[5]; p.quality_dist = a[6]; p.indel_profile = a[7];
        if (!ps::java_parse_double(a[8], p.bound_prob)) return usage("RBP_BOUND is not a number: '" + a[8] + "'");
        for (size_t i = 9; i < n; ++i) {
            if (a[i] == "-I") { if (i + 1 >= n) return usage("option -I needs a value"); ++i; }          // accepted and unused
            else if (a[i] == "--seed") {
                if (i + 1 >= n) return usage("option --seed needs a value");
                const std::string &s = a[++i];
                uint64_t x = 0; bool ok = !s.empty() && s.size() <= 20;
                for (char c : s) { ok = ok && c >= '0' && c <= '9' && x <= (UINT64_MAX - (uint64_t)(c - '0')) / 10; if (ok) x = x * 10 + (uint64_t)(c - '0'); }
                if (!ok) return usage("option --seed needs an unsigned integer, got '" + s + "'");
                p.seed = x; p.have_seed = true;
            }
        }
        p.call = kSimulate;
        return p;
    }
    if (p.mode == "setup") {               // :647-680: there is no external aligner to locate
        for (size_t i = 1; i < n; ++i) {
            if (a[i] != "--parasuite" && a[i] != "--bwa" && a[i] != "--bt2" && a[i] != "--bowtie") return usage("parameter not found: " + a[i]);
            if (i + 1 >= n) return usage("option " + a[i] + " needs a value");
            ++i;
        }
        p.call = kNotice; p.text = "parasuite setup: nothing to set up: the mapper is part of this program, there is no external aligner to locate\n";
        return p;
    }
    if (p.mode == "extract" || p.mode == "extractAligned") {     // :814-835, :856-871, with the flags' values stepped over (the Java never does)
        const bool weak = p.mode == "extract";
        for (size_t i = 1; i < n; ++i) {
            const std::string &f = a[i];
            const bool in = f == (weak ? "-i" : "-a"), out = f == "-o", thr = weak && f == "-t";
            if (!in && !out && !thr) return usage("input \"" + f + "\" invalid");
            if (i + 1 >= n) return usage("option " + f + " needs a value");
            const std::string &val = a[++i];
            if (in) p.mapping = val;
            else if (out) p.out = val;
            else if (!ps::java_parse_int(val, v)) return usage("option -t needs an integer, got '" + val + "'");
            else p.mapq_threshold = v;
        }
        if (p.mapping.empty() || p.out.empty()) return usage(std::string(weak ? "-i" : "-a") + " and -o are required");
        p.call = weak ? kExtractWeak : kExtractNames;
        return p;
    }
    // fetch, fetchBed (:888-899, :919-930): no default case, other arguments are passed over
    p.bed = p.mode == "fetchBed";
    for (size_t i = 1; i < n; ++i) {
        std::string *text = a[i] == "-i" ? &p.sites : a[i] == "-r" ? &p.ref : a[i] == "-o" ? &p.out : nullptr;
        if (!text) continue;
        if (i + 1 >= n) return usage("option " + a[i] + " needs a value");
        *text = a[++i];
    }
    if (p.sites.empty() || p.ref.empty() || p.out.empty()) return usage("-i, -r and -o are required");
    p.call = kFetch;
    return p;
}

}  // namespace parasuite_args
