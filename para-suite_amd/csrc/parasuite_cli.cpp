// parasuite_cli.cpp -- `parasuite <mode> ...`: the argv of `java -jar parasuite.jar <mode> ...` (src/src/main/Main.java) run as ONE
// call into libparasuite_hip.so, without a JVM.  parasuite_args.h turns the command line into a plan; this runs it, prints
// ps_last_error() on failure and returns 0 or 1.  The process makes its library call and returns: it starts no child and never
// replaces its own program.  Host threads of the host-side steps: PARASUITE_THREADS (default 8), as in the samtools shim.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include "../../include/parasuite_hip.h"
#include "parasuite_args.h"

static const char *opt(const std::string &s) { return s.empty() ? nullptr : s.c_str(); }

int main(int argc, char **argv)
{
    using namespace parasuite_args;
    const Plan p = parse(argc, argv);
    if (p.call == kUsage || p.call == kNotice) { std::fputs(p.text.c_str(), stderr); return p.call == kNotice ? 0 : 1; }
    for (const std::string &line : p.notes) std::fprintf(stderr, "%s\n", line.c_str());
    int threads = 8;
    if (const char *e = std::getenv("PARASUITE_THREADS")) threads = std::atoi(e) > 0 ? std::atoi(e) : 8;
    int rc = 1;
    switch (p.call) {
    case kMapRoute: {
        ps_route_opts2 o; std::memset(&o, 0, sizeof o);
        o.struct_size = (uint32_t)sizeof o;
        o.reads_fq = p.reads.c_str(); o.ref_fa = p.ref.c_str(); o.out_prefix = p.out_prefix.c_str(); o.transcripts_fa = opt(p.transcripts);
        o.bwa_mm = p.bwa_mm.c_str(); o.parasuite_mm = p.parasuite_mm.c_str(); o.error_profile = opt(p.error_profile); o.indel_profile = opt(p.indel_profile);
        o.ref_refine = opt(p.ref_refine); o.keep_unaligned = p.keep_unaligned ? 1 : 0;
        o.threads = p.threads; o.refine = p.refine ? 1 : 0; o.max_read_len = p.max_read_len; o.mapq_genomic = p.mapq_genomic; o.mapq_transcript = p.mapq_transcript;
        rc = ps_map_route_opts(&o, nullptr);
        break;
    }
    case kCombine: rc = ps_combine_genome_transcript(p.genome_bam.c_str(), p.transcript_bam.c_str(), p.out.c_str(), 1, 1, threads, nullptr); break;
    case kBenchmark: rc = ps_benchmark_reads(p.mapping.c_str(), p.out.c_str(), p.reads_fq.c_str(), nullptr); break;
    case kErrorProfile: rc = ps_error_profile_full(p.mapping.c_str(), p.ref.c_str(), p.max_read_len, nullptr, p.infer_qualities ? 2 : 0, nullptr); break;
    case kClusters: rc = ps_pileup_clusters(p.mapping.c_str(), p.ref.c_str(), p.out.c_str(), p.snp_vcf.c_str(), p.min_coverage, nullptr, nullptr); break;
    case kSimulate: {
        ps_simulate_opts o; std::memset(&o, 0, sizeof o);
        o.transcripts_fa = p.reads_fq.c_str(); o.out_prefix = p.out.c_str(); o.error_profile = p.error_profile.c_str(); o.t2c_profile = p.t2c_profile.c_str();
        o.t2c_positions = p.t2c_positions.c_str(); o.quality_dist = p.quality_dist.c_str(); o.indel_profile = p.indel_profile.c_str();
        o.bound_prob = p.bound_prob; o.select_read = -1; o.snp_rate = -1; o.snp_report = -1; o.allow_indels = -1;
        o.seed = p.seed;
        if (!p.have_seed) {                // from the clock, and said: the run can be repeated with --seed
            struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts);
            o.seed = (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
            std::fprintf(stderr, "parasuite simulate: --seed %llu\n", (unsigned long long)o.seed);
        }
        rc = ps_simulate_reads(&o, nullptr);
        break;
    }
    case kExtractWeak: {                   // into <BAM>.extract-tmp next to the input, then over the input (Main.java:841-848)
        const std::string tmp = p.mapping + ".extract-tmp";
        rc = ps_extract_weak_reads(p.mapping.c_str(), tmp.c_str(), p.out.c_str(), p.mapq_threshold, threads, nullptr);
        if (rc == 0 && std::rename(tmp.c_str(), p.mapping.c_str()) != 0) {
            std::fprintf(stderr, "parasuite extract: cannot rename %s to %s\n", tmp.c_str(), p.mapping.c_str());
            std::remove(tmp.c_str());
            return 1;
        }
        break;
    }
    case kExtractNames: rc = ps_extract_read_names(p.mapping.c_str(), p.out.c_str(), nullptr); break;
    case kFetch: rc = ps_fetch_sequences(p.ref.c_str(), p.sites.c_str(), p.out.c_str(), p.bed ? 1 : 0, nullptr); break;
    default: break;
    }
    if (rc) std::fprintf(stderr, "parasuite %s: %s\n", p.mode.c_str(), ps_last_error());
    return rc ? 1 : 0;
}
