// cli_args_check.cpp -- csrc/parasuite_args.h as a plain executable (tests/test_cli_args_cpu.py builds it with the host compiler,
// AddressSanitizer and UBSan): its own argv is the argv of `parasuite`, and it prints the plan as one JSON line --
// {"call": .., "exit": 0|1|null, "mode": .., "text": .., "notes": [..], and every field of the plan}.
#include <cstdio>
#include <string>
#include "parasuite_args.h"

static std::string js(const std::string &s)
{
    std::string o = "\"";
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back((char)c); }
        else if (c < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o.push_back((char)c);
    }
    return o + "\"";
}

int main(int argc, char **argv)
{
    using namespace parasuite_args;
    const Plan p = parse(argc, argv);
    std::string o = "{\"call\": " + js(call_name(p.call)) + ", \"exit\": " + (p.call == kUsage ? "1" : p.call == kNotice ? "0" : "null");
    const std::pair<const char *, const std::string *> texts[] = {
        {"mode", &p.mode}, {"text", &p.text}, {"reads", &p.reads}, {"ref", &p.ref}, {"ref_refine", &p.ref_refine}, {"out_prefix", &p.out_prefix},
        {"transcripts", &p.transcripts}, {"error_profile", &p.error_profile}, {"indel_profile", &p.indel_profile}, {"bwa_mm", &p.bwa_mm},
        {"parasuite_mm", &p.parasuite_mm}, {"bt_mm", &p.bt_mm}, {"user_command", &p.user_command}, {"mapping", &p.mapping}, {"out", &p.out},
        {"genome_bam", &p.genome_bam}, {"transcript_bam", &p.transcript_bam}, {"reads_fq", &p.reads_fq}, {"snp_vcf", &p.snp_vcf}, {"sites", &p.sites},
        {"t2c_profile", &p.t2c_profile}, {"t2c_positions", &p.t2c_positions}, {"quality_dist", &p.quality_dist}};
    for (const auto &t : texts) o += std::string(", \"") + t.first + "\": " + js(*t.second);
    const std::pair<const char *, long long> ints[] = {
        {"threads", p.threads}, {"max_read_len", p.max_read_len}, {"mapq_genomic", p.mapq_genomic}, {"mapq_transcript", p.mapq_transcript},
        {"min_coverage", p.min_coverage}, {"mapq_threshold", p.mapq_threshold}, {"refine", p.refine}, {"keep_unaligned", p.keep_unaligned},
        {"infer_qualities", p.infer_qualities}, {"bed", p.bed}, {"have_seed", p.have_seed}};
    for (const auto &t : ints) o += std::string(", \"") + t.first + "\": " + std::to_string(t.second);
    o += ", \"seed\": " + std::to_string((unsigned long long)p.seed) + ", \"bound_prob\": " + js(ps::java_double_to_string(p.bound_prob)) + ", \"notes\": [";
    for (size_t i = 0; i < p.notes.size(); ++i) o += (i ? ", " : "") + js(p.notes[i]);
    std::printf("%s]}\n", o.c_str());
    return 0;
}
